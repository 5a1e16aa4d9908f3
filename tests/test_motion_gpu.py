"""Motion scores on the MI355X: the three kernels of csrc/flow.hip under guard bands (tests/_guard.py), in both libraries, against the plain
numpy restatement of tests/_motion_ref.py -- vectors, both SADs and every sum bit for bit -- then `evaluate.main` with the VISTA_EVAL_MOTION
hook on the tiny world of tests/test_frontdoor_gpu.py: online, offline over the saved pictures, unset, and together with VISTA_EVAL_CLIP."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import _guard as G
from tests import _motion_ref as R
from tests.test_fidelity_gpu import _flags, _per_frame, _pictures, _records, scenes  # noqa: F401  (the two-scene dataset, by import)
from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)
from tests.test_perceptual_gpu import CLIP_KEYS, PARENT_KEYS

pytestmark = pytest.mark.gpu
LIBS = ("bf16", "fp16")


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------------
def _smooth(n, Hh, Ww, seed):
    """n frames cut from one smooth texture at drifting offsets: real motion, and windows that clamp on every side at the smallest sizes."""
    big = R.texture(Hh + 24, Ww + 24, seed)
    offs = [(12, 12), (9, 17), (15, 6), (3, 20)]
    return np.ascontiguousarray(np.stack([big[y:y + Hh, x:x + Ww] for y, x in offs[:n]]))


CASES = {
    "32x32": lambda: _smooth(2, 32, 32, 11),             # one level-2 block: every window clamped on all sides
    "32x64": lambda: _smooth(2, 32, 64, 12),
    "64x32": lambda: _smooth(2, 64, 32, 13),
    "96x160x3": lambda: _smooth(3, 96, 160, 14),         # a 3 x 5 coarse grid; two pairs
    "noise": lambda: R.noise_frames(2, 64, 96),          # no structure the pyramid could follow: near-ties everywhere
    "coarse_noise": lambda: R.coarse_noise_frames(3, 64, 64),   # few grey levels: exact ties, the lexicographic choice decides
    "flat": lambda: np.full((3, 32, 64, 3), 77, np.uint8),      # all ties: every vector zero
    "entering": lambda: R.entering_object(),             # a bright object crossing the border: the clamp
}
for _v in R.TRANSLATIONS:
    CASES["move_%d_%d" % _v] = functools.partial(R.translated_pair, _v)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per case and shared; the arrays are read-only."""
    frames = CASES[name]()
    levels = R.pyramid(frames)
    flow, sad = R.block_flow(frames)
    sums = R.pair_sums(flow, sad)
    for a in (frames, flow, sad, sums, *levels):
        a.setflags(write=False)
    return frames, levels, flow, sad, sums


def run_kernels(lib, frames_np):
    """The three entry points through the C ABI, every tensor in an arena -> (levels, flow, sad, sums) as numpy."""
    from vista_amd import ops
    n, Hh, Ww, _ = frames_np.shape
    with G.guarded(ops):
        frames = G.put(torch.from_numpy(np.array(frames_np)), label="frames")
        nbytes = lib.vk_flow_pyramid_bytes(n, Hh, Ww)
        assert nbytes == n * Hh * Ww * 21 // 16
        pyr = G.empty((nbytes,), torch.uint8, label="pyr")
        flow = G.empty((n - 1, Hh // 8, Ww // 8, 2), torch.int16, label="flow")
        sad = G.empty((n - 1, Hh // 8, Ww // 8, 2), torch.uint16, label="sad")
        sums = G.empty((n - 1, 5), torch.int64, label="sums")
        s = ops._stream()
        assert lib.vk_flow_luma_pyramid_u8(ops._p(frames), ops._p(pyr), n, Hh, Ww, s) == 0
        assert lib.vk_block_flow_u8(ops._p(pyr), ops._p(flow), ops._p(sad), n, Hh, Ww, s) == 0
        assert lib.vk_flow_pair_sums(ops._p(flow), ops._p(sad), None, ops._p(sums), n - 1, (Hh // 8) * (Ww // 8), s) == 0
        G.verify()
        levels = [t.cpu().numpy() for t in ops.flow_pyramid_levels(pyr, n, Hh, Ww)]
        return levels, flow.cpu().numpy(), sad.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("libname", LIBS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_flow_equals_the_reference_bit_for_bit(name, libname):
    from vista_amd import _lib
    frames, want_levels, want_flow, want_sad, want_sums = reference(name)
    levels, flow, sad, sums = run_kernels(_lib.load(libname), frames)
    for lvl, (got, want) in enumerate(zip(levels, want_levels)):
        assert np.array_equal(got, want), f"pyramid level {lvl}: {int((got != want).sum())} bytes differ"
    bad = (flow != want_flow).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} vectors differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{flow[bad][0].tolist()} for {want_flow[bad][0].tolist()}"
    assert np.array_equal(sad, want_sad), f"{int((sad != want_sad).sum())} SADs differ"
    assert np.array_equal(sums, want_sums), (sums.tolist(), want_sums.tolist())
    if name == "flat":
        assert not flow.any() and not sad.any() and not sums.any()
    if name == "entering":
        assert flow[0, 3, 0].tolist() == [0, 6] and not flow[0, :2].any() and not flow[0, 6:].any(), "the object is followed in from the border"
    if name.startswith("move_"):
        vector = tuple(int(v) for v in name.split("_")[1:])
        inside = R.interior_blocks(R.TRANSLATION_SHAPE, vector)
        assert inside.sum() >= 96
        assert (flow[0][inside] == vector).all() and not sad[0][inside][:, 0].any(), "every interior block returns the translation with SAD 0"


def test_the_python_layer_two_fields_and_repeatability():
    """ops / motion on the 96 x 160 case: the same bits as the C ABI and the reference, twice; the end-point sums of two fields; one frame."""
    from vista_amd import motion, ops
    frames, _levels, want_flow, want_sad, want_sums = reference("96x160x3")
    other = np.ascontiguousarray(frames[::-1])
    flow_o, sad_o = R.block_flow(other)
    with G.guarded(ops):
        a, b = G.put(torch.from_numpy(np.array(frames)), label="pred"), G.put(torch.from_numpy(other), label="real")
        flow, sad = motion.block_flow(a)
        flow2, sad2 = motion.block_flow(a)
        fo, so = motion.block_flow(b)
        sums, sums_two = ops.flow_pair_sums(flow, sad), ops.flow_pair_sums(flow, sad, fo)
        G.verify()
    assert flow.dtype == torch.int16 and sad.dtype == torch.uint16 and sums.dtype == torch.int64 and flow.is_cuda
    assert np.array_equal(flow.cpu().numpy(), want_flow) and np.array_equal(sad.cpu().numpy(), want_sad)
    assert torch.equal(flow, flow2) and torch.equal(sad.view(torch.int16), sad2.view(torch.int16)), "two calls, identical bytes"
    assert np.array_equal(fo.cpu().numpy(), flow_o) and np.array_equal(so.cpu().numpy(), sad_o)
    assert np.array_equal(sums.cpu().numpy(), want_sums)
    assert np.array_equal(sums_two.cpu().numpy(), R.pair_sums(want_flow, want_sad, flow_o)) and sums_two[:, 4].any()
    rep = motion.clip_motion(a, b)
    want = motion.report_from_sums(R.pair_sums(want_flow, want_sad, flow_o), 96, 160, R.pair_sums(flow_o, sad_o))
    for key in ("rms", "moving", "warp_err", "diff", "rms_real", "moving_real", "warp_err_real", "diff_real", "epe"):
        assert np.array_equal(getattr(rep, key), getattr(want, key), equal_nan=True), key
    assert np.isnan(rep.rms[0]) and rep.rms.shape == (3,)
    same = motion.clip_motion(a, a)
    assert not same.epe[1:].any() and np.array_equal(same.rms, same.rms_real, equal_nan=True)
    alone = motion.clip_motion(a)
    assert alone.epe is None and alone.rms_real is None and np.array_equal(alone.rms, rep.rms, equal_nan=True)
    # n = 1: empty results, no launch (nothing is allocated through ops either)
    with G.guarded(ops) as g:
        flow1, sad1 = motion.block_flow(a[:1])
        assert len(g.arenas) == 0
    assert flow1.shape == sad1.shape == (0, 12, 20, 2) and flow1.dtype == torch.int16 and sad1.dtype == torch.uint16
    one = motion.clip_motion(a[:1], b[:1])
    assert one.rms.shape == (1,) and np.isnan(one.rms[0]) and np.isnan(one.epe[0])


def test_refusals_leave_the_outputs_untouched():
    from vista_amd import _lib, motion, ops
    lib = _lib.load()
    frames_np = reference("32x64")[0]
    plus = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)   # noqa: E731
    assert lib.vk_flow_pyramid_bytes(2, 32, 64) == 2 * 32 * 64 * 21 // 16
    for n, Hh, Ww in ((0, 32, 64), (2, 48, 64), (2, 32, 40), (2, 0, 64), (2, 32, -32), (65536, 32, 32), (64, 4096, 8192)):
        assert lib.vk_flow_pyramid_bytes(n, Hh, Ww) == -22, (n, Hh, Ww)
    with G.guarded(ops):
        frames = G.put(torch.from_numpy(np.array(frames_np)), label="frames")
        pyr_in = G.put(torch.zeros(2 * 32 * 64 * 21 // 16 + 4, dtype=torch.uint8), label="pyr as an input")
        pyr = G.empty((2 * 32 * 64 * 21 // 16 + 4,), torch.uint8, label="pyr")
        flow, sad = G.empty((1, 4, 8, 2), torch.int16, label="flow"), G.empty((1, 4, 8, 2), torch.uint16, label="sad")
        flow_in = G.put(torch.zeros(1, 4, 8, 2, dtype=torch.int16), label="flow as an input")
        sad_in = G.put(torch.zeros(1, 4, 8, 2, dtype=torch.int16), label="sad as an input")
        sums = G.empty((2, 5), torch.int64, label="sums")
        p, s = ops._p, ops._stream()
        for args in ((None, p(pyr), 2, 32, 64), (p(frames), None, 2, 32, 64), (plus(frames, 1), p(pyr), 2, 32, 64), (p(frames), plus(pyr, 2), 2, 32, 64),
                     (p(frames), p(pyr), 0, 32, 64), (p(frames), p(pyr), -1, 32, 64), (p(frames), p(pyr), 2, 48, 64), (p(frames), p(pyr), 2, 32, 72),
                     (p(frames), p(pyr), 2, 0, 64), (p(frames), p(pyr), 65536, 32, 64), (p(frames), p(pyr), 64, 4096, 8192)):
            assert lib.vk_flow_luma_pyramid_u8(*args, s) == -22, args[2:]
        for args in ((None, p(flow), p(sad), 2, 32, 64), (p(pyr_in), None, p(sad), 2, 32, 64), (p(pyr_in), p(flow), None, 2, 32, 64),
                     (plus(pyr_in, 1), p(flow), p(sad), 2, 32, 64), (p(pyr_in), plus(flow, 2), p(sad), 2, 32, 64), (p(pyr_in), p(flow), plus(sad, 2), 2, 32, 64),
                     (p(pyr_in), p(flow), p(sad), 1, 32, 64), (p(pyr_in), p(flow), p(sad), 0, 32, 64), (p(pyr_in), p(flow), p(sad), 2, 40, 64),
                     (p(pyr_in), p(flow), p(sad), 2, 32, 16), (p(pyr_in), p(flow), p(sad), 65536, 32, 64), (p(pyr_in), p(flow), p(sad), 64, 4096, 8192)):
            assert lib.vk_block_flow_u8(*args, s) == -22, args[3:]
        for n, Hh, Ww in R.WRAPPING_SHAPES:   # (products that would wrap 64 or 32 bits: refused from the sides alone; tests/test_motion_cpu.py too)
            assert lib.vk_flow_pyramid_bytes(n, Hh, Ww) == -22, (n, Hh, Ww)
            assert lib.vk_flow_luma_pyramid_u8(p(frames), p(pyr), n, Hh, Ww, s) == -22, (n, Hh, Ww)
            assert lib.vk_block_flow_u8(p(pyr_in), p(flow), p(sad), n, Hh, Ww, s) == -22, (n, Hh, Ww)
        for args in ((None, p(sad_in), None, p(sums), 1, 32), (p(flow_in), None, None, p(sums), 1, 32), (p(flow_in), p(sad_in), None, None, 1, 32),
                     (plus(flow_in, 2), p(sad_in), None, p(sums), 1, 31), (p(flow_in), plus(sad_in, 2), None, p(sums), 1, 31),
                     (p(flow_in), p(sad_in), plus(flow_in, 2), p(sums), 1, 31), (p(flow_in), p(sad_in), None, plus(sums, 4), 1, 32),
                     (p(flow_in), p(sad_in), None, p(sums), 0, 32), (p(flow_in), p(sad_in), None, p(sums), 1, 0), (p(flow_in), p(sad_in), None, p(sums), 65536, 65536)):
            assert lib.vk_flow_pair_sums(*args, s) == -22, args[4:]
        G.verify()   # (every guard intact, every input unchanged)
        for t in (pyr, flow.view(torch.uint8), sad.view(torch.uint8), sums.view(torch.uint8)):
            assert bool((t == G.POISON).all()), "a refused call wrote nothing"
    # the Python layer refuses by name, before any launch
    u8 = torch.zeros(2, 32, 64, 3, dtype=torch.uint8).cuda()
    with pytest.raises(ValueError, match="multiples of 32"):
        motion.block_flow(torch.zeros(2, 48, 64, 3, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.flow_luma_pyramid_u8(torch.zeros(2, 32, 24, 3, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="multiples of 32"):
        motion.block_flow(torch.zeros(1, 40, 64, 3, dtype=torch.uint8).cuda())
    with pytest.raises(TypeError):
        ops.flow_luma_pyramid_u8(u8.float())
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.flow_luma_pyramid_u8(u8.cpu())
    for bad in (u8[0], u8[..., :2], u8.permute(0, 2, 1, 3), u8[:0]):
        with pytest.raises(ValueError):
            ops.flow_luma_pyramid_u8(bad)
    pyr = ops.flow_luma_pyramid_u8(u8)
    with pytest.raises(ValueError, match="no pair"):
        ops.block_flow_u8(pyr, 1, 32, 64)
    with pytest.raises(ValueError, match="flat, dense"):
        ops.block_flow_u8(pyr[:-4], 2, 32, 64)
    flow, sad = ops.block_flow_u8(pyr, 2, 32, 64)
    with pytest.raises(TypeError):
        ops.flow_pair_sums(flow.int(), sad)
    with pytest.raises(TypeError):
        ops.flow_pair_sums(flow, sad.view(torch.int16))
    with pytest.raises(ValueError, match="one shape"):
        ops.flow_pair_sums(flow, sad[:, :2])
    with pytest.raises(ValueError, match="one shape"):
        ops.flow_pair_sums(flow, sad, flow[:, :2])
    with pytest.raises(ValueError, match="pair up"):
        motion.clip_motion(u8, u8[:1])


# ---- evaluate.main on the tiny world ------------------------------------------------------------------------------------------------------------
MOTION_LISTS = ["flow_rms", "flow_rms_real", "flow_epe", "flow_moving", "warp_err", "warp_err_real"]
MOTION_KEYS = MOTION_LISTS + ["mean_" + k for k in MOTION_LISTS]
MOTION_INFO = {"block": 8, "levels": 3, "coarse_range": 7, "refine_range": 2, "reach_px": 30}


def _motion_part(records):
    return [[r[k] for k in MOTION_KEYS] + [[x["mean_flow_epe"] for x in r["rounds"]]] for r in records]


def test_evaluate_with_the_hook_online_then_offline(world, scenes, model, monkeypatch, capsys):  # noqa: F811
    from vista_amd import evaluate, motion
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)        # (the fixture's pipeline: same config, same checkpoint)
    monkeypatch.setenv("VISTA_EVAL_MOTION", "1")
    save = str(world["dir"] / "evaluate_motion")
    assert evaluate.main(_flags(world, scenes, save)) == 0
    out = capsys.readouterr().out
    assert "mean_flow_epe" in out and "motion " in out and "clip" not in out
    records = _records(save)
    assert len(records) == 2 and all(list(r) == PARENT_KEYS[:-1] + MOTION_KEYS + ["timings"] for r in records)
    assert all(sorted(r["timings"]) == ["condition", "decode", "encode", "load", "metrics", "motion", "sample", "save"] for r in records)
    assert all(list(x) == ["round", "frames", "mean_psnr", "mean_ssim", "mean_flow_epe"] for r in records for x in r["rounds"])
    for r in records:
        n = r["frames_scored"]
        assert n == T and all(len(r[k]) == n and r[k][0] is None and all(v is not None and v >= 0.0 for v in r[k][1:]) for k in MOTION_LISTS)
        pred = list(range(1, n))
        for key in MOTION_LISTS:
            assert r["mean_" + key] == math.fsum(r[key][i] for i in pred) / len(pred), "the conditioning frame is in no mean"
        assert [x["mean_flow_epe"] for x in r["rounds"]] == [r["mean_flow_epe"]]
        # the record's numbers are the module's on the saved pictures (the kernels are held to the reference above)
        pics, real = _pictures(save, "virtual", r["index"], n), _pictures(save, "real", r["index"], n)
        want = motion.clip_motion(torch.from_numpy(pics).cuda(), torch.from_numpy(real).cuda())
        for key, attr in evaluate.MOTION_KEYS.items():
            assert r[key][1:] == getattr(want, attr)[1:].tolist(), key
        assert any(v > 0.0 for v in r["flow_rms_real"][1:]) or any(v > 0.0 for v in r["warp_err_real"][1:]), "the real frames differ"
    online = json.load(open(os.path.join(save, "metrics_summary.json")))
    assert list(online) == ["scenes", "mean_psnr", "mean_ssim", "horizon"] + ["mean_" + k for k in MOTION_LISTS] + ["motion"]
    assert online["motion"] == MOTION_INFO == motion.motion_info()
    assert list(online["horizon"]) == ["frame", "scenes", "psnr", "ssim", "flow_rms", "flow_rms_real", "flow_epe"]
    for key in MOTION_LISTS:
        assert online["mean_" + key] == math.fsum(r["mean_" + key] for r in records) / 2
    for key in ("flow_rms", "flow_rms_real", "flow_epe"):
        assert online["horizon"][key][0] is None
        assert online["horizon"][key][1:] == [math.fsum(r[key][i] for r in records) / 2 for i in range(1, T)]
    # offline: no model, no checkpoint; the same bytes, the same numbers exactly
    monkeypatch.setattr(SU, "init_model", None)
    assert evaluate.main(["--compare", save, "--n_conds", "1", "--n_frames", str(T), "--action", "traj"]) == 0
    offline = _records(save)
    assert _motion_part(offline) == _motion_part(records) and _per_frame(offline) == _per_frame(records)
    assert all(sorted(r["timings"]) == ["load", "metrics", "motion"] for r in offline)
    assert json.load(open(os.path.join(save, "metrics_summary.json"))) == online
    # without the hook the records are the parent's, key for key, and hold the same fidelity numbers
    monkeypatch.setattr(SU, "init_model", lambda spec: model)
    monkeypatch.delenv("VISTA_EVAL_MOTION")
    plain = str(world["dir"] / "evaluate_motion_unset")
    capsys.readouterr()
    assert evaluate.main(_flags(world, scenes, plain) + ["--no_pictures"]) == 0
    assert "flow" not in capsys.readouterr().out
    unset = _records(plain)
    assert all(list(r) == PARENT_KEYS for r in unset) and all(list(x) == ["round", "frames", "mean_psnr", "mean_ssim"] for r in unset for x in r["rounds"])
    assert all(sorted(r["timings"]) == ["condition", "decode", "encode", "load", "metrics", "sample"] for r in unset)
    fidelity_part = lambda rs: [(r["index"], r["psnr"], r["ssim"], r["sse"], r["cond"], r["mean_psnr"], r["mean_ssim"]) for r in rs]   # noqa: E731
    assert fidelity_part(unset) == fidelity_part(records)
    summary = json.load(open(os.path.join(plain, "metrics_summary.json")))
    assert list(summary) == ["scenes", "mean_psnr", "mean_ssim", "horizon"] and list(summary["horizon"]) == ["frame", "scenes", "psnr", "ssim"]


def test_evaluate_with_both_hooks(world, scenes, model, monkeypatch):  # noqa: F811
    from vista_amd import evaluate
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)
    monkeypatch.setenv("VISTA_EVAL_MOTION", "1")
    monkeypatch.setenv("VISTA_EVAL_CLIP", "1")
    save = str(world["dir"] / "evaluate_motion_clip")
    assert evaluate.main(_flags(world, scenes, save) + ["--n_scenes", "1", "--no_pictures"]) == 0
    (rec,) = _records(save)
    assert list(rec) == PARENT_KEYS[:-1] + CLIP_KEYS + MOTION_KEYS + ["timings"], "the motion keys after the clip keys, timings last"
    assert sorted(rec["timings"]) == ["clip", "condition", "decode", "encode", "load", "metrics", "motion", "sample"]
    assert list(rec["rounds"][0]) == ["round", "frames", "mean_psnr", "mean_ssim", "mean_clip_sim", "mean_flow_epe"]
    summary = json.load(open(os.path.join(save, "metrics_summary.json")))
    assert list(summary)[-2:] == ["mean_warp_err_real", "motion"] and list(summary).index("clip") < list(summary).index("mean_flow_rms")
    assert list(summary["horizon"]) == ["frame", "scenes", "psnr", "ssim", "clip_sim", "clip_step", "flow_rms", "flow_rms_real", "flow_epe"]
