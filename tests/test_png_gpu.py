"""The PNG kernels (csrc/png.hip) on the MI355X against the plain restatement of tests/_png_ref.py, through the C ABI with poisoned outputs and
guard bands (tests/_guard.py), from both libraries (the object code is the same; the link is not). Equality is byte for byte: there is no
tolerance. Every deflate result also goes through zlib's inflate.

Filter shapes: 1 x 1, 1 x 7, 5 x 1 (no left neighbour, no row above), 17 x 33 (odd), 40 x 56 (every type winning, and ties). Deflate on arbitrary
byte rows: _png_ref.byte_cases -- short, exact and one-over last segments, run lengths around 3 and 258, runs across rows and segments, every
match length, no run at all, one repeated byte, both length limiters, symbols 16 / 17 / 18, incompressible noise."""
import ctypes
import functools
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _guard as G  # noqa: E402
from tests import _jpeg_ref as J  # noqa: E402
from tests import _png_ref as R  # noqa: E402
from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: E402,F401  (fixtures, by import)

LIBS = ("bf16", "fp16")
PLAN_WORDS = 420
EINVAL = -22


# ---- filter -------------------------------------------------------------------------------------------------------------------------------------
def _showcase_pair():
    a = R.showcase(40, 56)
    return np.stack([a, a[::-1].copy()])


FILTER_CASES = {
    "1x1": lambda: J.noise(2, 1, 1, seed=2),
    "1x7": lambda: J.noise(2, 1, 7, seed=3),
    "5x1": lambda: J.noise(2, 5, 1, seed=4),
    "17x33": lambda: J.smooth_noise(2, 17, 33, seed=5),
    "40x56_every_type_and_ties": _showcase_pair,
}


@functools.lru_cache(maxsize=None)
def filter_reference(name):
    frames = FILTER_CASES[name]()
    rows = R.filter_rows(frames)
    for a in (frames, rows):
        a.setflags(write=False)
    return frames, rows


@pytest.mark.parametrize("libname", LIBS)
@pytest.mark.parametrize("name", sorted(FILTER_CASES))
def test_filter_equals_the_reference_byte_for_byte(name, libname):
    from vista_amd import _lib, ops
    lib = _lib.load(libname)
    frames, want = filter_reference(name)
    n, h, w, _ = frames.shape
    with G.guarded(ops):
        x = G.put(torch.from_numpy(np.array(frames)), label="frames")
        rows = G.empty((n, h, 1 + 3 * w), torch.uint8, label="rows")
        assert lib.vk_png_filter_u8(ops._p(x), ops._p(rows), n, h, w, ops._stream()) == 0
        G.verify()
        got = rows.cpu().numpy()
    assert np.array_equal(got[:, :, 0], want[:, :, 0]), "the filter types"
    assert np.array_equal(got, want)
    if name.startswith("40x56"):
        assert set(want[0, :, 0].tolist()) == {0, 1, 2, 3, 4} and want[0, 0, 0] == 0 and want[0, 2, 0] == 1, "every type wins a row; ties go to the lowest"


# ---- deflate ------------------------------------------------------------------------------------------------------------------------------------
CASES = R.byte_cases()


@functools.lru_cache(maxsize=None)
def deflate_reference(name):
    rows, seg_rows = CASES[name]
    rows.setflags(write=False)
    return rows, seg_rows, R.deflate_rows(rows, seg_rows)


def deflate(lib, rows_np, seg_rows, gap=0, guard=True):
    """The two deflate entry points through the C ABI; `gap` bytes are left between the frames' slices. -> (sizes, adler, offsets, out) as numpy."""
    from vista_amd import ops
    n, h, rb = rows_np.shape
    segs = -(-h // seg_rows)
    ns = n * segs
    rows = G.put(torch.from_numpy(np.array(rows_np)), label="rows") if guard else torch.from_numpy(np.array(rows_np)).cuda()
    mk = (lambda shape, dt, label: G.empty(shape, dt, label=label)) if guard else (lambda shape, dt, label: torch.empty(shape, dtype=dt, device="cuda"))
    sizes, adler, plan = mk((ns,), torch.int32, "sizes"), mk((ns, 2), torch.int32, "adler"), mk((ns, PLAN_WORDS), torch.int32, "plan")
    assert lib.vk_png_deflate_plan(ops._p(rows), ops._p(sizes), ops._p(adler), ops._p(plan), n, h, rb, seg_rows, ns, ops._stream()) == 0
    s = sizes.cpu().numpy().astype(np.int64)
    assert (s > 0).all() and (s < 2 * seg_rows * rb + 600).all(), "every segment was sized"
    off = np.concatenate([[0], np.cumsum(s)[:-1]]) + gap * (np.arange(ns) // segs)
    total = int(off[-1] + s[-1]) + gap
    offsets = G.put(torch.from_numpy(off), label="offsets") if guard else torch.from_numpy(off).cuda()
    out = mk((total,), torch.uint8, "stream")
    if not guard:
        out.fill_(G.POISON)
    assert lib.vk_png_deflate_write(ops._p(rows), ops._p(plan), ops._p(offsets), ops._p(out), total, n, h, rb, seg_rows, ns, ops._stream()) == 0
    return s, adler.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, off, out.cpu().numpy()


@pytest.mark.parametrize("libname", LIBS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_deflate_equals_the_reference_byte_for_byte_and_inflates(name, libname):
    from vista_amd import _lib, ops
    lib = _lib.load(libname)
    rows, seg_rows, want = deflate_reference(name)
    n, h, rb = rows.shape
    segs = -(-h // seg_rows)
    with G.guarded(ops):
        sizes, adler, off, out = deflate(lib, rows, seg_rows, gap=16)
        G.verify()
    used = np.zeros(out.size, bool)
    for f in range(n):
        for k, (part, pair, size) in enumerate(want[f]):
            i = f * segs + k
            assert sizes[i] == len(part), f"frame {f} segment {k}: {sizes[i]} bytes, the reference writes {len(part)}"
            assert tuple(adler[i]) == pair, f"frame {f} segment {k}: Adler sums"
            assert out[off[i]:off[i] + sizes[i]].tobytes() == part, f"frame {f} segment {k}"
            used[off[i]:off[i] + sizes[i]] = True
        first, last = f * segs, (f + 1) * segs - 1
        raw = out[off[first]:off[last] + sizes[last]].tobytes()
        assert zlib.decompress(raw, -15) == rows[f].tobytes(), f"frame {f}: inflate returns the rows"
    assert (out[~used] == G.POISON).all() and (~used).sum() == 16 * n, "the bytes between and past the frames' slices are untouched"


def test_the_cases_are_the_cases_they_claim_to_be():
    """The properties the case names promise, read from the reference's tables (so that a changed generator cannot quietly stop covering them)."""
    def tables(name, seg=0):
        rows, seg_rows = CASES[name]
        return R.segment_tables(rows[0, seg * seg_rows:(seg + 1) * seg_rows].tobytes())
    t = tables("fibonacci_15_bit_limit")
    assert max(R.code_lengths(t["lit_hist"], 99)) > 15 >= max(t["lit_len"])
    t = tables("code_length_7_bit_limit")
    assert max(R.code_lengths(t["cl_hist"], 99)) > 7 >= max(t["cl_len"])
    t = tables("long_zero_stretches")
    assert {16, 17, 18} <= {s for s, _, _ in t["tree"]}
    t = tables("no_run_at_all")
    assert t["dist_len"] == 0 and t["n_match"] == 0
    t = tables("one_repeated_byte")
    assert t["tokens"][0] == (0, 0x55) and all(kind == 1 for kind, _ in t["tokens"][1:])
    t = tables("every_match_length")
    assert sorted(v for kind, v in t["tokens"] if kind) == list(range(3, 259))
    assert all(t["lit_hist"][s] for s in range(257, 286)), "every length code"
    t = tables("run_lengths")
    got, want = [v for kind, v in t["tokens"] if kind], []
    for k in (0, 1, 2, 3, 256, 257, 258, 259, 260, 261, 0, 262, 4, 516, 517, 518, 519, 1):   # the equal bytes behind each run's first literal
        want += [258] * (k // 258) + ([k % 258] if k % 258 >= 3 else [])
    assert got == want and want[3:8] == [258, 258, 258, 258, 3], got
    assert sum(1 for kind, _ in t["tokens"] if not kind) == 18 + 1 + 2 + 1 + 2 + 1 + 2 + 1, "k = 259: one literal behind the match; 260: two; 261: none"
    t = tables("run_across_segments", seg=1)
    assert t["tokens"][0] == (0, 77) and t["tokens"][1] == (1, 79), "a segment's first byte is a literal; the run ends with the segment"
    t = tables("run_across_rows")
    assert (1, 4) in t["tokens"], "9 9 | 9 9 9: the run crosses the row boundary"
    rows, _ = CASES["uniform_noise"]
    assert sum(len(p) for p, _, _ in R.deflate_rows(rows, 16)[0]) > rows.size, "noise grows"


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def _decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB"
        return np.array(im)


def test_encode_png_on_frames_and_on_a_grid_canvas():
    from vista_amd import ops, png
    frames = J.smooth_noise(2, 40, 56, seed=13)
    x = torch.from_numpy(frames).cuda()
    files = png.encode_png(x)
    assert len(files) == 2
    for f in range(2):
        assert files[f] == R.png_file(frames[f]), f"frame {f}: the reference's file"
        assert np.array_equal(_decode(files[f]), frames[f])
    assert png.encode_png(frames) == files, "a numpy array is uploaded and encoded alike"
    assert png.encode_png(x[1])[0] == files[1] == png.encode_png(x[1:2])[0], "one picture; a frame of a batch equals the single-frame call"
    samples = torch.from_numpy(J.smooth_noise(5, 24, 40, seed=14).astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous().cuda()
    canvas = ops.frames_to_u8(samples, real=False, grid=True)
    assert canvas.dim() == 3 and canvas.shape[0] > 2 * 24 and canvas.shape[1] > 2 * 40
    (file,) = png.encode_png(canvas)
    assert file == R.png_file(canvas.cpu().numpy()) and np.array_equal(_decode(file), canvas.cpu().numpy())


def test_write_apng_reads_back_through_read_video_frames(tmp_path):
    from vista_amd import png
    from vista_amd import sample_utils as SU
    frames = J.smooth_noise(4, 24, 40, seed=15)
    frames[2] = frames[1]                                  # a repeated frame stays a frame of its own
    path = png.write_apng(str(tmp_path / "clip.apng"), torch.from_numpy(frames).cuda(), 10)
    assert open(path, "rb").read() == R.apng_file(frames, 10)
    assert np.array_equal(SU.read_video_frames(path), frames)
    still = np.repeat(frames[:1], 3, 0)
    assert np.array_equal(SU.read_video_frames(png.write_apng(str(tmp_path / "still.apng"), still, 10)), still)


def test_refusals_through_ops_and_through_the_c_abi():
    from vista_amd import _lib, ops
    from vista_amd.ops import OperandError
    lib, p = _lib.load(), ops._p
    good = torch.zeros((2, 24, 40, 3), dtype=torch.uint8, device="cuda")
    for bad in (good[:, :, ::2], good[:, :, :, :2], good.float(), good.cpu(), good[:, :0], good[:, :, :0], good[:0]):
        with pytest.raises(OperandError, match="frames"):
            ops.png_filter(bad)
    wide = torch.empty((1, 1, 65536, 3), dtype=torch.uint8, device="cuda")
    for bad in (wide, wide.view(1, 65536, 1, 3)):
        with pytest.raises(OperandError, match="frames"):
            ops.png_filter(bad)
    rows = ops.png_filter(good)
    for bad in (rows[:, :, ::2], rows.int(), rows.cpu(), rows[0], rows[:, :0], rows[:0]):
        with pytest.raises(OperandError, match="rows"):
            ops.png_deflate(bad)
    for seg_rows in (0, -1, 16.0, None, True):
        with pytest.raises(OperandError, match="seg_rows"):
            ops.png_deflate(rows, seg_rows)
    big = torch.empty((1, 2, (1 << 23) + 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(OperandError, match="rows.*16777216"):
        ops.png_deflate(big, 2)
    # ---- the C entry points: VK_EINVAL, outputs still poison ----
    with G.guarded(ops):
        x = G.put(good.cpu(), label="frames")
        r = G.empty((2, 24, 121), torch.uint8, label="rows")
        src = G.put(rows.cpu(), label="rows in")
        sizes = G.empty((4,), torch.int32, label="sizes")
        adler = G.empty((4, 2), torch.int32, label="adler")
        plan = G.empty((4, PLAN_WORDS), torch.int32, label="plan")
        out = G.empty((4096,), torch.uint8, label="stream")
        offsets = G.put(torch.zeros(4, dtype=torch.int64), label="offsets")
        vp = lambda t: t if t is None or isinstance(t, ctypes.c_void_p) else p(t)  # noqa: E731
        at = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)  # noqa: E731

        def a(x_=x, r_=r, n=2, h=24, w=40):
            return lib.vk_png_filter_u8(vp(x_), vp(r_), n, h, w, ops._stream())

        def b(write, src_=src, n=2, h=24, rb=121, seg=16, ns=4, sizes_=sizes, adler_=adler, plan_=plan, off_=offsets, out_=out, out_bytes=4096):
            if write:
                return lib.vk_png_deflate_write(vp(src_), vp(plan_), vp(off_), vp(out_), out_bytes, n, h, rb, seg, ns, ops._stream())
            return lib.vk_png_deflate_plan(vp(src_), vp(sizes_), vp(adler_), vp(plan_), n, h, rb, seg, ns, ops._stream())
        for why, kw in {"null frames": dict(x_=None), "null rows": dict(r_=None), "n = 0": dict(n=0), "n < 0": dict(n=-1), "H = 0": dict(h=0),
                        "W = 0": dict(w=0), "H = 65536": dict(h=65536), "W = 65536": dict(w=65536), "2^31 bytes": dict(n=1, h=65535, w=65535)}.items():
            assert a(**kw) == EINVAL, why
        for why, kw in {"null rows": dict(src_=None), "null plan": dict(plan_=None), "plan misaligned": dict(plan_=at(plan, 2)), "n = 0": dict(n=0),
                        "H = 0": dict(h=0), "row_bytes = 0": dict(rb=0), "seg_rows = 0": dict(seg=0), "seg_rows < 0": dict(seg=-16),
                        "a segment count that does not match": dict(ns=3), "another": dict(seg=8),
                        "a segment beyond 2^24 bytes": dict(n=1, h=2, rb=(1 << 23) + 1, seg=2, ns=1),
                        "2^31 bytes": dict(n=128, h=2, rb=1 << 23, seg=1, ns=256)}.items():
            assert b(False, **kw) == EINVAL and b(True, **kw) == EINVAL, why
        for why, kw in {"null sizes": dict(sizes_=None), "null adler": dict(adler_=None), "sizes misaligned": dict(sizes_=at(sizes, 2)),
                        "adler misaligned": dict(adler_=at(adler, 2))}.items():
            assert b(False, **kw) == EINVAL, why
        for why, kw in {"null offsets": dict(off_=None), "null out": dict(out_=None), "offsets misaligned": dict(off_=at(offsets, 4)),
                        "out_bytes = 0": dict(out_bytes=0), "out_bytes = 2^31": dict(out_bytes=2 ** 31)}.items():
            assert b(True, **kw) == EINVAL, why
        G.verify()
        for t in (r, sizes, adler, plan, out):
            assert bool((t.view(torch.uint8) == G.POISON).all()), "a refused call wrote nothing"
        # and the accepted call, with offsets that would leave the buffer: out_bytes too small, nothing beyond it is stored
        assert b(False) == 0 and b(True, out_bytes=10) == 0
        G.verify()
        assert bool((out[10:] == G.POISON).all()) and bool((out[:10] != G.POISON).any())


def _save_both_ways(monkeypatch, tmp_path, samples, inputs):
    from vista_amd import frontdoor
    roots = {}
    for mode in ("hip", None):
        monkeypatch.delenv("VISTA_PNG", raising=False)
        if mode:
            monkeypatch.setenv("VISTA_PNG", mode)
        roots[mode] = str(tmp_path / (mode or "pillow"))
        frontdoor.save_pictures(roots[mode], "NUSCENES", 0, virtual=samples, real=inputs)
    return roots


def test_front_door_on_the_tiny_model_writes_the_same_pixels_under_the_hook_and_the_parents_bytes_without(world, model, monkeypatch, tmp_path):
    from PIL import Image
    from vista_amd import ops, pipeline, sample
    from vista_amd import sample_utils as SU
    monkeypatch.setitem(sys.modules, "imageio", None)     # (where imageio is importable the video is an mp4 in both modes)
    monkeypatch.delenv("VISTA_VIDEO", raising=False)
    torch.manual_seed(7)
    samples, _, inputs = sample.run(model, world["frames"], None, height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02, eager=True)
    roots = _save_both_ways(monkeypatch, tmp_path, samples, inputs)
    monkeypatch.delenv("VISTA_PNG", raising=False)
    for side, x, real in (("virtual", samples, False), ("real", inputs, True)):
        u8 = ops.frames_to_u8(x.float(), real=real).cpu().numpy()
        grid = ops.frames_to_u8(x.float(), real=real, grid=True).cpu().numpy()
        for sub in ("images", "grids", "videos"):
            names = sorted(os.listdir(os.path.join(roots["hip"], side, sub)))
            assert names == sorted(os.listdir(os.path.join(roots[None], side, sub))), "the same file names in both modes"
            for name in names:
                hip, plain = (os.path.join(roots[m], side, sub, name) for m in ("hip", None))
                if sub == "videos":
                    assert name.endswith(".apng") and np.array_equal(SU.read_video_frames(hip), SU.read_video_frames(plain))
                    assert np.array_equal(SU.read_video_frames(hip), u8)
                    assert open(hip, "rb").read() == R.apng_file(u8, 10)
                else:
                    assert np.array_equal(np.asarray(Image.open(hip)), np.asarray(Image.open(plain))), (side, sub, name)
                    assert open(hip, "rb").read()[:2 + 8 + 25 + 8] .endswith(b"IDAT" + R.ZLIB_HEADER), "IHDR, then one IDAT with the pinned header"
        assert len(os.listdir(os.path.join(roots["hip"], side, "images"))) == x.shape[0]
        assert open(os.path.join(roots["hip"], side, "grids", "NUSCENES_000000.png"), "rb").read() == R.png_file(grid)
        # without the hook: the bytes Pillow writes from the host copy, as before the hook existed
        for i in range(x.shape[0]):
            buf = io.BytesIO()
            Image.fromarray(u8[i]).save(buf, format="PNG")
            assert open(os.path.join(roots[None], side, "images", f"NUSCENES_000000_{i:04}.png"), "rb").read() == buf.getvalue()
        buf = io.BytesIO()
        Image.fromarray(grid).save(buf, format="PNG")
        assert open(os.path.join(roots[None], side, "grids", "NUSCENES_000000.png"), "rb").read() == buf.getvalue()
    monkeypatch.setenv("VISTA_PNG", "hip")
    monkeypatch.setattr(pipeline, "_to_u8", lambda *a, **k: pytest.fail("under the hook the 8-bit frames stay on the GPU"))
    SU.perform_save_locally(str(tmp_path / "again" / "virtual"), samples, "images", "NUSCENES", 1)
