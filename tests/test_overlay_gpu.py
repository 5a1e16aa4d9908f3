"""vk_stroke_overlay_u8 (csrc/overlay.hip) on the MI355X against the numpy float32 evaluation of its definition (tests/_overlay_ref.py).
No tolerance anywhere: every comparison is of bytes. Shapes: 128 x 256 (dword path, 8 x 4 tiles), 37 x 53 (byte path, a ragged last group and
ragged tiles) and 11 x 12 (dword path inside one tile)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _overlay_ref as R  # noqa: E402

SHAPES = [(128, 256), (37, 53), (11, 12)]
RED, GREEN, BLUE, WHITE = (255.0, 0.0, 0.0), (0.0, 255.0, 64.0), (16.0, 32.0, 255.0), (255.0, 255.0, 255.0)


def _max_counts(H, W):
    """The plan's maxima: 8 sets x 4 strokes x 2 segments = 32 strokes, 64 segments."""
    rng = np.random.default_rng(H * 1000 + W)
    sets = []
    for s in range(8):
        strokes = []
        for k in range(4):
            pts = rng.uniform(-0.2, 1.2, (3, 2)) * (W, H)
            segs = [(float(pts[0, 0]), float(pts[0, 1]), float(pts[1, 0]), float(pts[1, 1])), (float(pts[1, 0]), float(pts[1, 1]), float(pts[2, 0]), float(pts[2, 1]))]
            strokes.append((tuple(float(c) for c in rng.integers(0, 256, 3)), float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.0, 3.0)), segs))
        sets.append(strokes)
    return sets


def _cases(H, W):
    """name -> (sets, set_of_frame). Coordinates scale with the frame so that every shape sees every situation."""
    diag = [(-10.0, H / 3.0, W + 10.0, 2.0 * H / 3.0), (W / 2.0, -5.0, W / 3.0, H + 5.0)]
    a = (RED, 0.7, 2.0, [(2.0, 2.0, W - 3.0, H - 3.0)])
    b = (BLUE, 0.6, 2.5, [(W - 3.0, 2.5, 3.0, H - 2.0)])
    c = {
        "crossing_the_borders": ([[(GREEN, 0.8, 1.5, diag)]], [0]),
        "wholly_outside": ([[(RED, 1.0, 2.0, [(-30.0, -30.0, -10.0, -5.0), (W + 5.0, 2.0, W + 40.0, H + 0.0)]), (BLUE, 1.0, 3.0, [(W / 2.0, H + 9.0, W / 2.0, H + 9.0)])]], [0]),
        "fringe_from_outside": ([[(WHITE, 1.0, 2.0, [(-1.0, 3.0, -1.0, H - 3.0)]), (RED, 0.5, 1.25, [(3.0, H + 1.0, W - 3.0, H + 1.0)])]], [0]),
        "disc": ([[(BLUE, 0.9, 3.3, [(W / 2.0 + 0.25, H / 2.0, W / 2.0 + 0.25, H / 2.0)])]], [0]),
        # centres 3-4-5 apart from the disc's centre are exactly 5 away: coverage exactly 0.5 (r = 5) and exactly 0 (r = 4.5)
        "integer_exact_distances": ([[(RED, 1.0, 5.0, [(5.5, 5.5, 5.5, 5.5)]), (GREEN, 1.0, 4.5, [(W - 5.5, H - 5.5, W - 5.5, H - 5.5)]),
                                      (BLUE, 1.0, 1.0, [(0.5, 0.5, W - 0.5, 0.5), (0.5, 0.5, 0.5, H - 0.5)])]], [0]),
        "r_zero": ([[(WHITE, 1.0, 0.0, [(1.0, 1.3, W - 1.0, H - 1.7), (W / 2.0, H / 2.0, W / 2.0, H / 2.0), (0.5, H - 0.5, W - 0.5, H - 0.5)])]], [0]),
        "alpha_zero": ([[(RED, 0.0, 3.0, diag)]], [0]),
        "alpha_one": ([[(RED, 1.0, 3.0, diag), (GREEN, 1.0, 0.75, [(W / 4.0, H / 2.0, 3.0 * W / 4.0, H / 2.0)])]], [0]),
        "overlap_a_then_b": ([[a, b]], [0]),
        "overlap_b_then_a": ([[b, a]], [0]),
        "maximum_counts": (_max_counts(H, W), [7, 0, 3]),
        "seven_frames_mixed_sets": ([[a], [b, (GREEN, 0.5, 1.0, diag)], [], [(WHITE, 0.25, 4.0, [(W / 2.0, H / 2.0, W / 2.0, H / 2.0)])]], [0, -1, 3, 1, -1, 2, 8]),
    }
    return c


CASE_NAMES = sorted(_cases(16, 16))


@functools.lru_cache(maxsize=None)
def _frames(H, W, n):
    return np.random.default_rng(H * 7 + W + n).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(H, W, name):
    """(frames, sets, set_of_frame, expected), computed once and shared; the arrays are read-only."""
    sets, which = _cases(H, W)[name]
    frames = _frames(H, W, len(which))
    want = R.overlay(frames, sets, which)
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, sets, which, want


def _differ(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}" if len(bad) else ""


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_bytes_equal_the_numpy_definition(H, W, name):
    from vista_amd import ops
    frames, sets, which, want = _reference(H, W, name)
    x = torch.from_numpy(np.array(frames)).cuda()
    got = ops.stroke_overlay(x, sets, which)
    assert got.dtype == torch.uint8 and got.shape == x.shape and got.data_ptr() != x.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want), _differ(got.cpu().numpy(), want)
    assert np.array_equal(x.cpu().numpy(), frames), "out of place leaves the input alone"
    again = ops.stroke_overlay(x, sets, torch.tensor(which, dtype=torch.int32, device="cuda"))
    assert torch.equal(again, got), "two runs are bitwise equal"
    y = x.clone()
    assert ops.stroke_overlay(y, sets, which, out=y) is y and torch.equal(y, got), "in place equals out of place"
    if name in ("alpha_zero", "wholly_outside"):
        assert np.array_equal(want, frames)
    elif name != "maximum_counts" or H > 11:
        assert not np.array_equal(want, frames), "the case draws something"


@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_a_frame_of_a_batch_equals_the_single_frame_call_and_order_matters(H, W):
    from vista_amd import ops
    for name in ("seven_frames_mixed_sets", "maximum_counts"):
        frames, sets, which, want = _reference(H, W, name)
        x = torch.from_numpy(np.array(frames)).cuda()
        for k, s in enumerate(which):
            one = ops.stroke_overlay(x[k:k + 1], sets, [s])
            assert np.array_equal(one[0].cpu().numpy(), want[k]), (name, k)
            if not 0 <= s < len(sets) or not sets[s]:
                assert np.array_equal(want[k], frames[k]), "-1, a set past the plan and an empty set copy the frame"
    ab, ba = _reference(H, W, "overlap_a_then_b")[3], _reference(H, W, "overlap_b_then_a")[3]
    assert not np.array_equal(ab, ba), "strokes composite in list order"


def test_the_byte_path_takes_any_alignment_and_a_longer_rollout_than_one_plan():
    from vista_amd import drive, ops
    H, W = 37, 53
    frames, sets, which, want = _reference(H, W, "seven_frames_mixed_sets")
    flat = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(np.array(frames)).cuda().view(-1)
    x = flat[1:].view(frames.shape)
    assert x.data_ptr() % 2 == 1 and np.array_equal(ops.stroke_overlay(x, sets, which).cpu().numpy(), want)
    # draw_hud over seven rounds (T = 5: 17 frames): more segments than one plan holds, drawn in runs of rounds
    H, W, T = 128, 256, 5
    full = {"goal": [0.4, 0.6], "trajectory": [1.0, 0.5, 2.0, 1.0, 3.0, 1.5, 4.0, 2.0], "command": 1, "speed": [2.0, 3.0, 4.0, 5.0], "angle": [0.1, -0.5, 1.0, 0.05]}
    actions = [full, {}, full, full, {"command": 3}, full, full]
    n = drive.round_range(len(actions) - 1, T)[1]
    frames = _frames(H, W, n)
    got = drive.draw_hud(torch.from_numpy(np.array(frames)).cuda(), actions, T)
    sets = [drive.hud_strokes(a, H, W) for a in actions]
    assert ops.stroke_counts(sets)[2] > ops.OVERLAY_MAX_SEGMENTS
    want = np.stack([R.draw(frames[i], sets[drive.frame_round(i, T)]) for i in range(n)])
    assert np.array_equal(got.cpu().numpy(), want), _differ(got.cpu().numpy(), want)
    assert np.array_equal(want[T:T + 2], frames[T:T + 2]) and not np.array_equal(want[0], frames[0])


def test_every_invalid_argument_returns_einval_without_a_launch():
    from vista_amd import _lib, ops
    lib, p = _lib.load(), ops._p
    H, W, n = 16, 24, 2
    x = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((n, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    which = torch.zeros(4, dtype=torch.int32, device="cuda")
    good = [[(RED, 1.0, 2.0, [(2.0, 2.0, 20.0, 12.0)])]]

    def call(plan=None, a=x, b=out, w=which, n_=n, H_=H, W_=W, null_plan=False):
        plan = ops.stroke_plan(good) if plan is None else plan
        vp = lambda t: t if t is None or isinstance(t, ctypes.c_void_p) else p(t)  # noqa: E731
        return lib.vk_stroke_overlay_u8(vp(a), vp(b), vp(w), None if null_plan else ctypes.byref(plan), n_, H_, W_, ops._stream())

    def edited(**fields):
        plan = ops.stroke_plan(good)
        for path, value in fields.items():
            table, field = path.split("__")
            if table == "plan":
                setattr(plan, field, value)
            elif field.startswith("color"):
                getattr(plan, table)[0].color[int(field[5:])] = value
            else:
                setattr(getattr(plan, table)[0], field, value)
        return plan
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad = {
        "null in": dict(a=None), "null out": dict(b=None), "null set_of_frame": dict(w=None), "null plan": dict(null_plan=True),
        "misaligned in, W % 4 == 0": dict(a=off(x, 1)), "misaligned out, W % 4 == 0": dict(b=off(out, 2)), "misaligned set_of_frame": dict(w=off(which, 2)),
        "n = 0": dict(n_=0), "n < 0": dict(n_=-1), "n > 65535": dict(n_=65536), "H = 0": dict(H_=0), "W = 0": dict(W_=0), "W < 0": dict(W_=-4),
        "sets over the maximum": dict(plan=edited(plan__n_sets=9)), "strokes over the maximum": dict(plan=edited(plan__n_strokes=33)),
        "segments over the maximum": dict(plan=edited(plan__n_segments=65)), "negative set count": dict(plan=edited(plan__n_sets=-1)),
        "negative stroke count": dict(plan=edited(plan__n_strokes=-1)), "negative segment count": dict(plan=edited(plan__n_segments=-1)),
        "alpha < 0": dict(plan=edited(stroke__alpha=-0.01)), "alpha > 1": dict(plan=edited(stroke__alpha=1.01)), "alpha nan": dict(plan=edited(stroke__alpha=nan)),
        "r < 0": dict(plan=edited(stroke__r=-1.0)), "r inf": dict(plan=edited(stroke__r=inf)), "r nan": dict(plan=edited(stroke__r=nan)),
        "inv_len2 < 0": dict(plan=edited(seg__inv_len2=-1.0)), "inv_len2 inf": dict(plan=edited(seg__inv_len2=inf)), "inv_len2 nan": dict(plan=edited(seg__inv_len2=nan)),
        "colour > 255": dict(plan=edited(stroke__color1=256.0)), "colour < 0": dict(plan=edited(stroke__color2=-1.0)),
        "coordinate inf": dict(plan=edited(seg__bx=inf)), "coordinate nan": dict(plan=edited(seg__ay=nan)), "coordinate beyond 2^20": dict(plan=edited(seg__ax=2.0e6)),
        "segment run leaves the table": dict(plan=edited(stroke__seg_count=2)), "negative segment run": dict(plan=edited(stroke__seg_begin=-1)),
        "stroke run leaves the table": dict(plan=edited(set__stroke_begin=1)), "negative stroke run": dict(plan=edited(set__stroke_count=-1)),
    }
    for what, kw in bad.items():
        assert call(**kw) == -22, what
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((x == 7).all()), "nothing was launched"
    assert call() == 0 and call(W_=23, a=off(x, 1), b=off(out, 1)) == 0, "the same arguments are fine; 23 columns take any alignment"
    torch.cuda.synchronize()
    with pytest.raises(_lib.VistaHipError, match="-22"):
        ops.stroke_overlay(x, [[(RED, 1.5, 2.0, [(2.0, 2.0, 20.0, 12.0)])]], [0, 0])
    with pytest.raises(ValueError):
        ops.stroke_overlay(x, good, [0])
    with pytest.raises(TypeError):
        ops.stroke_overlay(x.float(), good, [0, 0])
