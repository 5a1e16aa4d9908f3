"""The JPEG kernels (csrc/jpeg.hip) on the MI355X against the float64 restatement of tests/_jpeg_ref.py, through the C ABI with poisoned outputs
and guard bands (tests/_guard.py), from both libraries (the object code is the same; the link is not).

Shapes: 16 x 16 (one MCU), 24 x 40 and 40 x 56 (ragged both ways, several frames), 1 x 1 and 40 x 1 (padding only), 16 x 192 (72 blocks in an
interval: more than a wave), 32 x 704 (264: more than a workgroup's 256 lanes, so a second chunk with carried bits), 160 x 16 (ten intervals: the
RSTm counter wraps). Stage A may differ from float64 only at ties; stage B, given the kernel's own coefficients, is exact to the byte."""
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
from tests import _guard as G  # noqa: E402
from tests import _jpeg_ref as R  # noqa: E402

LIBS = ("bf16", "fp16")
TIE, CAP, ROOM_DB = 1e-3, 0.01, 0.05   # |quotient - half-integer| of a permitted difference; its share per case; what that share may cost in PSNR

# name -> (frames, quality)
CASES = {
    "one_mcu_noise_q100": lambda: (R.noise(1, 16, 16), 100),
    "ragged_24x40_q50": lambda: (R.smooth_noise(2, 24, 40), 50),
    "ragged_40x56_q1": lambda: (R.smooth_noise(3, 40, 56, seed=3), 1),
    "ragged_40x56_q90": lambda: (R.smooth_noise(3, 40, 56, seed=3), 90),
    "padding_1x1": lambda: (R.noise(1, 1, 1, seed=5), 90),
    "padding_40x1": lambda: (R.noise(1, 40, 1, seed=6), 90),
    "two_waves_16x192_noise_q100": lambda: (R.noise(1, 16, 192, seed=7), 100),
    "two_chunks_32x704_noise_q100": lambda: (R.noise(1, 32, 704, seed=8), 100),
    "ten_intervals_160x16_q50": lambda: (R.smooth_noise(1, 160, 16, seed=9), 50),
    "checkerboard_q100": lambda: (R.checkerboard(1, 16, 16), 100),
    "mcu_checker_q100": lambda: (R.mcu_checker(1, 32, 48), 100),
    "black_q90": lambda: (np.zeros((1, 16, 16, 3), np.uint8), 90),
    "step_ties_q95": lambda: (R.step(1, 32, 48), 95),
}
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(frames, quality, float64 coefficients, quotients, PSNR of the float64 stream per frame): computed once, shared, read-only."""
    frames, q = CASES[name]()
    coef, quot = R.coefficients(frames, q)
    H, W = frames.shape[1:3]
    psnr = tuple(R.psnr(R.decode(R.jpeg_file(c, W, H, q)), f) for c, f in zip(coef, frames))
    for a in (frames, coef, quot):
        a.setflags(write=False)
    return frames, q, coef, quot, psnr


def geometry(frames):
    n, H, W, _ = frames.shape
    return n, H, W, -(-H // 16), -(-W // 16)


def stage_a(lib, frames, quality, guard=None):
    """vk_jpeg_dct_quant_u8 through the C ABI -> the coefficient tensor (inside arenas where a guard session is given)."""
    from vista_amd import ops
    n, H, W, mh, mw = geometry(frames)
    x = torch.from_numpy(np.array(frames))
    x = G.put(x, label="frames") if guard else x.cuda()
    shape = (n, 6 * mh * mw, 64)
    coef = G.empty(shape, torch.int16, label="coef") if guard else torch.empty(shape, dtype=torch.int16, device="cuda")
    q = ops.jpeg_quant(quality)
    assert lib.vk_jpeg_dct_quant_u8(ops._p(x), ops._p(coef), ctypes.byref(q), n, H, W, ops._stream()) == 0
    return coef


def stage_b(lib, coef, n, mh, mw, gap=0, guard=None):
    """The two entropy entry points through the C ABI; `gap` bytes are left between the frames' slices. -> (sizes, offsets, out) as numpy."""
    from vista_amd import ops
    blocks = n * 6 * mh * mw
    sizes = G.empty((n * mh,), torch.int32, label="sizes") if guard else torch.empty(n * mh, dtype=torch.int32, device="cuda")
    assert lib.vk_jpeg_interval_sizes(ops._p(coef), ops._p(sizes), n, mh, mw, blocks, ops._stream()) == 0
    s = sizes.cpu().numpy().astype(np.int64)
    assert (s > 0).all(), "every interval was written"
    off = np.concatenate([[0], np.cumsum(s)[:-1]]) + gap * (np.arange(n * mh) // mh)
    total = int(off[-1] + s[-1]) + gap
    offsets = torch.from_numpy(off).cuda()
    out = G.empty((total,), torch.uint8, label="scan") if guard else torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    assert lib.vk_jpeg_entropy_write(ops._p(coef), ops._p(offsets), ops._p(out), total, n, mh, mw, blocks, ops._stream()) == 0
    return s, off, out.cpu().numpy()


def judge_stage_a(name, got, want, quot):
    d = got != want
    share = d.mean()
    near = np.abs(np.abs(quot[d]) % 1.0 - 0.5)
    print(f"MJPEGPARITY stage_a {name}: {int(d.sum())} of {d.size} coefficients differ ({100 * share:.3f} %), farthest from a tie "
          f"{near.max() if d.any() else 0.0:.2e}, max |coef| {int(np.abs(got.astype(int)).max())}")
    assert (near < TIE).all(), f"a coefficient differs where the float64 quotient is {near.max():.3g} from a half-integer"
    assert (np.abs(got[d].astype(int) - want[d].astype(int)) == 1).all()
    assert share <= CAP


@pytest.mark.parametrize("libname", LIBS)
@pytest.mark.parametrize("name", NAMES)
def test_stage_a_equals_float64_but_for_ties_and_stage_b_is_exact(name, libname):
    from vista_amd import _lib, ops
    lib = _lib.load(libname)
    frames, q, want, quot, _ = reference(name)
    n, H, W, mh, mw = geometry(frames)
    with G.guarded(ops) as g:
        coef = stage_a(lib, frames, q, guard=g)
        G.verify()
        got = coef.cpu().numpy()
        judge_stage_a(name, got, want, quot)
        assert (got[..., 0] >= -1024).all() and (np.abs(got[..., 1:].astype(int)) <= 1023).all() and (got[..., 0] <= 1023).all()
        sizes, off, out = stage_b(lib, coef, n, mh, mw, gap=16, guard=g)
        G.verify()
    used = np.zeros(out.size, bool)
    for f in range(n):
        parts = R.intervals(got[f], mh, mw)
        for r, part in enumerate(parts):
            i = f * mh + r
            assert sizes[i] == len(part), f"frame {f} interval {r}: {sizes[i]} bytes, the reference coder writes {len(part)}"
            assert out[off[i]:off[i] + sizes[i]].tobytes() == part, f"frame {f} interval {r}"
            if r < mh - 1:
                assert out[off[i] + sizes[i] - 2:off[i] + sizes[i]].tobytes() == bytes([0xFF, 0xD0 + r % 8]), f"frame {f}: RST{r % 8} follows interval {r}"
            used[off[i]:off[i] + sizes[i]] = True
    assert (out[~used] == G.POISON).all() and (~used).sum() == 16 * n, "the bytes between and past the frames' slices are untouched"
    print(f"MJPEGPARITY stage_b {name}: {int(sizes.sum())} bytes in {len(sizes)} intervals equal the bit-serial coder's")


def test_three_zero_runs_of_sixteen_every_category_and_a_second_chunk():
    """Coefficient arrays no picture gives: a block whose only AC coefficient is the last of the zigzag (ZRL, ZRL, ZRL, then run 14), DC steps
    across the whole range, every magnitude category, and a second chunk that starts inside a byte."""
    from vista_amd import _lib
    lib = _lib.load()
    mh, mw = 2, 44                                        # 264 blocks per interval
    coef = np.zeros((1, 6 * mh * mw, 64), np.int16)
    coef[0, 0, 63] = 5
    coef[0, 1, 63] = -1023
    coef[0, 2, 0], coef[0, 3, 0] = 1023, -1024
    for k in range(1, 11):
        coef[0, 10 + k, k * 6] = (1 << k) - 1
        coef[0, 30 + k, 63 - k * 3] = -(1 << (k - 1))
    rng = np.random.default_rng(11)
    coef[0, 264:] = rng.integers(-1023, 1024, (264, 64)) * (rng.random((264, 64)) < 0.5)
    sizes, off, out = stage_b(lib, torch.from_numpy(coef).cuda(), 1, mh, mw)
    parts = R.intervals(coef[0], mh, mw)
    assert [int(s) for s in sizes] == [len(p) for p in parts]
    assert out.tobytes() == b"".join(parts)
    assert b"\xff\x00" in parts[1], "the dense interval needs stuffing"
    # a foreign array: values stage A cannot write are coded as the nearest it can (DC, predictor and AC alike), the contract of the header
    wild = coef.copy()
    wild[0, 5, 0], wild[0, 11, 0], wild[0, 17, 0], wild[0, 4, 7], wild[0, 9, 63] = 32767, -32768, 1500, 32767, -32768
    tame = wild.astype(np.int32)
    tame[..., 0] = np.clip(tame[..., 0], -1024, 1023)
    tame[..., 1:] = np.clip(tame[..., 1:], -1023, 1023)
    sizes, off, out = stage_b(lib, torch.from_numpy(wild).cuda(), 1, mh, mw)
    assert out.tobytes() == b"".join(R.intervals(tame[0].astype(np.int16), mh, mw)) and not np.array_equal(wild, tame)


@pytest.mark.parametrize("name", NAMES)
def test_encode_jpeg_end_to_end(name):
    from vista_amd import ops, video
    frames, q, _, _, ref_psnr = reference(name)
    n, H, W, mh, mw = geometry(frames)
    x = torch.from_numpy(np.array(frames)).cuda()
    jpegs = video.encode_jpeg(x, q)
    coef = ops.jpeg_dct_quant(x, q).cpu().numpy()
    assert len(jpegs) == n
    for f in range(n):
        assert jpegs[f] == R.jpeg_file(coef[f], W, H, q), f"frame {f}: header + the reference coder's scan of the kernel's coefficients + EOI"
        got = R.decode(jpegs[f])
        assert got.shape == (H, W, 3)
        p = R.psnr(got, frames[f])
        print(f"MJPEGPARITY end_to_end {name} frame {f}: {len(jpegs[f])} bytes, PSNR {p:.3f} dB, float64 stream {ref_psnr[f]:.3f} dB")
        assert p >= ref_psnr[f] - ROOM_DB
    assert video.encode_jpeg(x, q) == jpegs, "two calls give identical bytes"
    assert video.encode_jpeg(np.array(frames), q) == jpegs, "a numpy array is uploaded and encoded alike"
    if n > 1:
        assert video.encode_jpeg(x[1:2], q)[0] == jpegs[1], "a frame of a batch equals the single-frame call"


def test_refusals_through_ops_and_through_the_c_abi():
    from vista_amd import _lib, ops
    from vista_amd.ops import OperandError
    lib, p = _lib.load(), ops._p
    good = torch.zeros((2, 24, 40, 3), dtype=torch.uint8, device="cuda")
    # ---- ops ----
    for bad, operand in ((good[:, :, ::2], "frames"), (good[:, :, :, :2], "frames"), (good.float(), "frames"), (good.cpu(), "frames"),
                         (good[:, :0], "frames"), (good[:, :, :0], "frames"), (good[:0], "frames")):
        with pytest.raises(OperandError, match=operand):
            ops.jpeg_dct_quant(bad, 90)
    for quality in (0, 101, 90.0, None):
        with pytest.raises(OperandError, match="quality"):
            ops.jpeg_dct_quant(good, quality)
    wide = torch.empty((1, 1, 65536, 3), dtype=torch.uint8, device="cuda")
    for bad in (wide, wide.view(1, 65536, 1, 3)):
        with pytest.raises(OperandError, match="frames"):
            ops.jpeg_dct_quant(bad, 90)
    coef = ops.jpeg_dct_quant(good, 90)
    for bad, mh, mw, operand in ((coef, 2, 2, "coef"), (coef[:, :-1], 2, 3, "coef"), (coef.int(), 2, 3, "coef"), (coef.cpu(), 2, 3, "coef"),
                                 (coef[:, :, ::2], 2, 3, "coef"), (coef, 0, 3, "mcu_h"), (coef, 2, 4097, "mcu_w")):
        with pytest.raises(OperandError, match=operand):
            ops.jpeg_entropy(bad, mh, mw)
    # ---- the C entry points: VK_EINVAL, outputs still poison ----
    EINVAL = -22
    with G.guarded(ops):
        x = G.put(good.cpu(), label="frames")
        c = G.empty((2, 36, 64), torch.int16, label="coef")
        sizes = G.empty((4,), torch.int32, label="sizes")
        out = G.empty((4096,), torch.uint8, label="scan")
        offsets = G.put(torch.zeros(4, dtype=torch.int64), label="offsets")
        src = G.put(coef.cpu(), label="coef in")

        def quant(quality=90, **edit):
            q = ops.jpeg_quant(90)
            q.quality = quality
            for field, value in edit.items():
                getattr(q, field)[3] = value
            return q

        def a(x_=x, c_=c, q=None, n=2, H=24, W=40, null_q=False):
            vp = lambda t: t if t is None or isinstance(t, ctypes.c_void_p) else p(t)  # noqa: E731
            return lib.vk_jpeg_dct_quant_u8(vp(x_), vp(c_), None if null_q else ctypes.byref(q or quant()), n, H, W, ops._stream())

        def b(write, src_=src, n=2, mh=2, mw=3, blocks=72, sizes_=sizes, off_=offsets, out_=out, out_bytes=4096):
            vp = lambda t: t if t is None or isinstance(t, ctypes.c_void_p) else p(t)  # noqa: E731
            if write:
                return lib.vk_jpeg_entropy_write(vp(src_), vp(off_), vp(out_), out_bytes, n, mh, mw, blocks, ops._stream())
            return lib.vk_jpeg_interval_sizes(vp(src_), vp(sizes_), n, mh, mw, blocks, ops._stream())
        at = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)  # noqa: E731
        bad_a = {"null frames": dict(x_=None), "null coef": dict(c_=None), "null quant": dict(null_q=True), "coef misaligned": dict(c_=at(c, 2)),
                 "n = 0": dict(n=0), "n < 0": dict(n=-1), "H = 0": dict(H=0), "W = 0": dict(W=0), "H = 65536": dict(H=65536), "W = 65536": dict(W=65536),
                 "quality 0": dict(q=quant(0)), "quality 101": dict(q=quant(101)), "a zero divisor": dict(q=quant(luma=0)),
                 "a 9-bit divisor": dict(q=quant(chroma=256)), "2^31 blocks": dict(n=2 ** 31 - 1, H=65535, W=65535)}
        for why, kw in bad_a.items():
            assert a(**kw) == EINVAL, why
        bad_b = {"null coef": dict(src_=None), "coef misaligned": dict(src_=at(src, 2)), "n = 0": dict(n=0), "mcu_h = 0": dict(mh=0), "mcu_w = 0": dict(mw=0),
                 "mcu_h = 4097": dict(mh=4097, blocks=6 * 2 * 4097 * 3), "mcu_w = 4097": dict(mw=4097, blocks=6 * 2 * 2 * 4097),
                 "a block count that does not match": dict(blocks=71), "another": dict(mw=2), "2^31 blocks": dict(n=32768, mh=4096, mw=4096, blocks=-1)}
        for why, kw in bad_b.items():
            assert b(False, **kw) == EINVAL and b(True, **kw) == EINVAL, why
        for why, kw in {"null sizes": dict(sizes_=None), "sizes misaligned": dict(sizes_=at(sizes, 2))}.items():
            assert b(False, **kw) == EINVAL, why
        for why, kw in {"null offsets": dict(off_=None), "null out": dict(out_=None), "offsets misaligned": dict(off_=at(offsets, 4)),
                        "out_bytes = 0": dict(out_bytes=0), "out_bytes = 2^31": dict(out_bytes=2 ** 31)}.items():
            assert b(True, **kw) == EINVAL, why
        G.verify()
        for t in (c, sizes, out):
            assert bool((t.view(torch.uint8) == G.POISON).all()), "a refused call wrote nothing"
        # and the accepted call, with offsets that would leave the buffer: nothing beyond out_bytes is stored
        assert b(False) == 0 and b(True, out_bytes=100) == 0
        G.verify()
        assert bool((out[100:] == G.POISON).all())


def test_front_door_writes_an_avi_under_the_hook_and_what_it_wrote_before_without(monkeypatch, tmp_path):
    from vista_amd import ops, pipeline
    from vista_amd import sample_utils as SU
    frames = R.smooth_noise(3, 24, 40, seed=21)
    samples = torch.from_numpy(frames.astype(np.float32) / 255.0).permute(0, 3, 1, 2).contiguous().cuda()
    u8 = ops.frames_to_u8(samples, real=False).cpu().numpy()
    monkeypatch.delenv("VISTA_VIDEO_QUALITY", raising=False)
    monkeypatch.setenv("VISTA_VIDEO", "mjpeg")
    monkeypatch.setattr(pipeline, "_to_u8", lambda *a, **k: pytest.fail("mjpeg mode takes the 8-bit frames on the GPU, not through the host round trip"))
    root = str(tmp_path / "virtual")
    SU.perform_save_locally(root, samples, "videos", "IMG", 7)
    path = os.path.join(root, "videos", "IMG_000007.avi")
    assert os.listdir(os.path.join(root, "videos")) == ["IMG_000007.avi"]
    got = SU.read_video_frames(path)
    assert got.shape == u8.shape and got.dtype == np.uint8
    avi = R.parse_avi(open(path, "rb").read())
    assert avi["avih"][0] == 100000 and avi["avih"][4] == 3 and avi["strh"]["rate"] == 10 and avi["strf"]["width"] == 40 and avi["strf"]["height"] == 24
    ref = R.encode(u8, 90)
    for f in range(3):
        p, want = R.psnr(got[f], u8[f]), R.psnr(R.decode(ref[f]), u8[f])
        print(f"MJPEGPARITY front_door frame {f}: PSNR {p:.3f} dB, float64 stream {want:.3f} dB")
        assert p >= want - ROOM_DB
    monkeypatch.undo()
    monkeypatch.delenv("VISTA_VIDEO", raising=False)
    monkeypatch.setitem(sys.modules, "imageio", None)     # (where imageio is importable the unset hook writes an mp4 through it, as before)
    root = str(tmp_path / "plain")
    SU.perform_save_locally(root, samples, "videos", "IMG", 7)
    assert os.listdir(os.path.join(root, "videos")) == ["IMG_000007.apng"]
    assert np.array_equal(SU.read_video_frames(os.path.join(root, "videos", "IMG_000007.apng")), u8), "lossless, as before the hook existed"


def test_heat_and_hud_videos_take_the_gpu_tensor_in_both_modes(monkeypatch, tmp_path):
    """reward.save_heat_videos and the HUD video of drive hand save_video the 8-bit GPU tensor: an .avi under the hook, and without it the
    animated PNG that the host copy of the same bytes gives."""
    import types
    from vista_amd import drive, ops, reward
    from vista_amd import sample_utils as SU
    n, H, W = 3, 32, 48
    inputs = torch.from_numpy(R.smooth_noise(n, H, W, seed=31).astype(np.float32) / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous().cuda()
    fmap = torch.rand((n, H // 8, W // 8), generator=torch.Generator().manual_seed(3)).cuda()
    heat = ops.heat_overlay_u8(inputs.float(), fmap, 1.0, alpha=reward.HEAT_ALPHA).cpu().numpy()
    hud = drive.draw_hud(ops.frames_to_u8(inputs, real=True), [{"command": 1, "goal": [0.4, 0.6]}], n)
    monkeypatch.setitem(sys.modules, "imageio", None)
    monkeypatch.delenv("VISTA_VIDEO_QUALITY", raising=False)
    for mode, ext in (("mjpeg", ".avi"), (None, ".apng")):
        monkeypatch.delenv("VISTA_VIDEO", raising=False)
        if mode:
            monkeypatch.setenv("VISTA_VIDEO", mode)
        root = str(tmp_path / ext[1:])
        paths = reward.save_heat_videos(root, inputs, [("traj", {}, None), ("steer", None, "no record")], [types.SimpleNamespace(map=fmap)], "IMG", 2,
                                        heat_max=1.0)
        assert paths == [os.path.join(root, "heat", "traj", "videos", "IMG_000002" + ext)]
        got_heat = SU.read_video_frames(paths[0])
        got_hud = SU.read_video_frames(SU.save_video(os.path.join(root, "hud"), hud, 10))
        for got, src in ((got_heat, heat), (got_hud, hud.cpu().numpy())):
            assert got.shape == src.shape
            if mode is None:
                assert np.array_equal(got, src), "lossless, as from the host copy"
            else:
                ref = R.encode(src, 90)
                for f in range(n):
                    assert R.psnr(got[f], src[f]) >= R.psnr(R.decode(ref[f]), src[f]) - ROOM_DB
