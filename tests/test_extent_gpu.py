"""The storage-independent kernels (image I/O, reward / plan statistics, heat and stroke overlays, frame fidelity, CLIP preprocessing, the
first-stage sampler and the ensemble variance) on poisoned outputs inside guard bands (tests/_guard.py): each picks a vector or a byte path
from a size, so each runs at a shape on either side of its switch and at its ragged tiles, on embedded operands, and is held to the reference
its own module already uses:
  bitwise   where that reference is exact: Pillow's integers, numpy float32 expressions without a transcendental, tests/_overlay_ref.py, the
            integer squared differences, the kernel a kernel extends (candidate_frame_stats == ensemble_frame_stats per candidate);
  at that module's own bound where its reference is float64 or torch fp32 with an exp (SSIM: tests/_fidelity_ref.py; the statistics:
            1e-5 against tests/_plan_ref.py / torch float64; clip_preprocess_patches: 1.2e-2 against oracle/clip_oracle.py; gaussian_sample:
            tests/test_vae_gpu.py's allclose), AND bitwise equal to the same call on plain allocations: guarding changes no arithmetic and no path.
Every test ends with verify(): every guard byte of every output, intermediate and workspace intact, every operand unchanged. The Lanczos tables
load_img_batch caches come from numpy, not from the allocation factories: they are the one kernel-visible memory here outside an arena.
copy_row_boxes keeps its own sentinels (tests/test_reshard_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import _fidelity_ref as FR
from tests import _guard
from tests import _overlay_ref as OR
from tests import _plan_ref as PR
from tests.test_frontdoor_gpu import _numpy_make_grid, _numpy_u8, _unit_samples
from tests.test_reward_frontdoor_gpu import _frames_and_map, _numpy_overlay

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(autouse=True)
def ops():
    from vista_amd import ops
    with _guard.guarded(ops):
        yield ops
        _guard.verify()


def _members(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 3 + 1


# ---- image I/O ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("oh,ow", [(24, 32), (21, 27)], ids=["w%4==0", "odd_width"])
def test_load_img_batch_equals_live_pillow(oh, ow, ops):
    Image = pytest.importorskip("PIL.Image")
    src = np.random.default_rng(37 * 53 + ow).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    left, top, cw, ch = 5, 3, 41, 29                                        # a crop box off the origin
    want = torch.stack([torch.from_numpy(np.array(Image.fromarray(f).crop((left, top, left + cw, top + ch)).resize((ow, oh), resample=Image.LANCZOS)))
                        .permute(2, 0, 1).to(F32).div(255) * 2.0 - 1.0 for f in src])
    got = ops.load_img_batch(_guard.put(torch.from_numpy(src), label="frames"), oh, ow, box=(left, top, cw, ch))
    assert got.shape == (2, 3, oh, ow) and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    _guard.verify()


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("n,H,W", [(3, 5, 7), (2, 8, 16)])
def test_frames_to_u8_and_its_grid_equal_numpy_float32(n, H, W, real, ops):
    x = _unit_samples(n, H, W, seed=n * H + W)
    if real:
        x = x * 2.0 - 1.0
    xg = _guard.put(x, label="frames")
    got = ops.frames_to_u8(xg, real=real).cpu().numpy()
    want = _numpy_u8(x, real).transpose(0, 2, 3, 1)
    assert np.array_equal(got, want), int((got != want).sum())
    grid = ops.frames_to_u8(xg, real=real, grid=True).cpu().numpy()         # pad = 2
    want = _numpy_u8(torch.from_numpy(_numpy_make_grid(x.numpy())), real).transpose(1, 2, 0)
    assert grid.shape == want.shape and np.array_equal(grid, want), int((grid != want).sum())
    _guard.verify()


# ---- reward / plan statistics -------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((p is None and q is None) or (p is not None and q is not None and torch.equal(p, q)) for p, q in zip(a, b))


@pytest.mark.parametrize("want_map", [True, False])
@pytest.mark.parametrize("h,w", [(5, 7), (6, 6)], ids=["hw35", "hw36"])
def test_ensemble_frame_stats(h, w, want_map, ops):
    x = _members((3, 3, 4, h, w), seed=h * w)
    xg = _guard.put(x, label="members")
    frame_sum, fmap = ops.ensemble_frame_stats(xg, want_map=want_map)
    var = x.double().var(0, unbiased=True)
    rel_sum = ((frame_sum.cpu() - var.sum(dim=(1, 2, 3))).abs() / var.sum(dim=(1, 2, 3))).max().item()
    assert frame_sum.shape == (3,) and rel_sum <= 1e-5, rel_sum
    if want_map:
        rel_map = ((fmap.cpu().double() - var.mean(dim=1)).abs() / var.mean(dim=1)).max().item()
        assert fmap.shape == (3, h, w) and rel_map <= 1e-5, rel_map
    else:
        assert fmap is None
    with _guard.plain(ops):
        assert _same(ops.ensemble_frame_stats(x.cuda(), want_map=want_map), (frame_sum, fmap)), "not the bits of the call on plain allocations"
    _guard.verify()


@pytest.mark.parametrize("want_map", [True, False])
@pytest.mark.parametrize("h,w", [(5, 7), (6, 6)], ids=["hw35", "hw36"])
def test_candidate_frame_stats(h, w, want_map, ops):
    K, t0 = 3, 1
    x = _members((K, 3, 3, 4, h, w), seed=h * w + 1)
    xg = _guard.put(x, label="candidates")
    frame_sum, total, best, fmap = ops.candidate_frame_stats(xg, t0, want_map=want_map)
    assert frame_sum.shape == (K, 2) and total.shape == (K,) and best.dim() == 0 and (fmap is None) == (not want_map)
    for k in range(K):
        one_sum, one_map = ops.ensemble_frame_stats(xg[k][:, t0:], want_map=want_map)
        assert _same((frame_sum[k], fmap[k] if want_map else None), (one_sum, one_map)), f"candidate {k}: not ensemble_frame_stats' bits"
        assert float(total[k]) == float(frame_sum[k, 0]) + float(frame_sum[k, 1]), "total: the frame sums added left to right"
    ref_sum, _, ref_best, ref_map = PR.candidate_frame_stats(x, t0, want_map=True)
    assert ((frame_sum.cpu() - ref_sum).abs() / ref_sum).max().item() <= 1e-5 and int(best) == PR.select(total.tolist()) == int(ref_best)
    if want_map:
        assert ((fmap.cpu().double() - ref_map.double()).abs() / ref_map.double()).max().item() <= 1e-5
    with _guard.plain(ops):
        assert _same(ops.candidate_frame_stats(x.cuda(), t0, want_map=want_map), (frame_sum, total, best, fmap))
    _guard.verify()


def test_heat_overlay_equals_numpy_float32(ops):
    n, H, W, cell, vmax, alpha = 2, 8, 12, 4, 0.37, 0.6
    frames, fmap = _frames_and_map(n, H, W, cell, seed=H + W, vmax=vmax)
    got = ops.heat_overlay_u8(_guard.put(frames, label="frames"), _guard.put(fmap, label="map"), vmax, alpha=alpha).cpu().numpy()
    want = _numpy_overlay(frames, fmap, cell, vmax, alpha)
    assert got.shape == (n, H, W, 3) and np.array_equal(got, want), int((got != want).sum())
    _guard.verify()


# ---- frame fidelity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(11, 11), (27, 45), (26, 44)], ids=["one_window", "w%4!=0_ragged_tiles", "w%4==0"])
@pytest.mark.parametrize("content", ["noise_pm3", "bright_250_255"])
def test_frame_fidelity(H, W, content, ops):
    n = 2
    a, b = FR.make_case(content, (n, H, W))
    da, db = _guard.put(torch.from_numpy(a), label="a"), _guard.put(torch.from_numpy(b), label="b")
    sse, ssim_sum = ops.frame_fidelity_u8(da, db)
    assert sse.shape == ssim_sum.shape == (n, 3) and np.array_equal(sse.cpu().numpy(), FR.sse_ref(a, b))
    ssim = (ssim_sum.cpu().numpy() / ((H - 10) * (W - 10))).mean(axis=1)
    err = float(np.abs(ssim - FR.ssim_ref64(a, b)).max())
    assert err <= FR.ssim_bound(H, W), (err, FR.ssim_bound(H, W))
    with _guard.plain(ops):
        assert _same(ops.frame_fidelity_u8(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()), (sse, ssim_sum))
    _guard.verify()


# ---- stroke overlay -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("W", [68, 67], ids=["dword_path", "byte_path"])
def test_stroke_overlay_equals_the_numpy_definition(W, in_place, ops):
    H = 17                                                                  # 16 x 64 tiles: a ragged second tile along both axes
    frames = np.random.default_rng(H + W).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    sets, which = [[((255.0, 0.0, 64.0), 0.7, 2.0, [(58.5, 3.0, 66.5, 16.5)])]], [0, -1]    # one stroke across the tile edges x = 64 and y = 16
    want = OR.overlay(frames, sets, which)
    assert not np.array_equal(want[0, 16, 64:], frames[0, 16, 64:]) and not np.array_equal(want[0, :16, :64], frames[0, :16, :64])
    if in_place:
        x = _guard.scratch(torch.from_numpy(frames).cuda(), "frames (out == in)")
        got = ops.stroke_overlay(x, sets, which, out=x)
        assert got is x
    else:
        x = _guard.put(torch.from_numpy(frames), label="frames")
        got = ops.stroke_overlay(x, sets, which)
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    _guard.verify()


# ---- CLIP preprocessing ---------------------------------------------------------------------------------------------------------------------------
def test_clip_preprocess_patches_small(ops):
    from oracle import clip_oracle as CO
    n, H, W, size, patch = 2, 20, 36, 28, 14
    img = torch.tanh(torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(5)) * 1.5)
    got = ops.clip_preprocess_patches(_guard.put(img, label="img"), out_hw=size, patch=patch)
    assert got.shape == (n * 5, 640)
    bits = got.view(torch.int16).view(n, 5, 640)
    assert not bits[:, 0].any() and not bits[:, :, 588:].any(), "the class-token rows and the K-pad columns of the zeros output stay zero, bit for bit"
    want = CO.preprocess(img, size).unfold(2, patch, patch).unfold(3, patch, patch).permute(0, 2, 3, 1, 4, 5).reshape(n, 4, 588)
    err = (got.float().cpu().view(n, 5, 640)[:, 1:, :588] - want).abs().max().item()
    assert err <= 1.2e-2, err
    with _guard.plain(ops):
        assert torch.equal(ops.clip_preprocess_patches(img.cuda(), out_hw=size, patch=patch), got)
    _guard.verify()


# ---- first-stage sampler, ensemble variance -------------------------------------------------------------------------------------------------------
def test_gaussian_sample_at_a_size_not_a_multiple_of_four(ops):
    g = torch.Generator().manual_seed(3)
    mom = torch.randn(3, 6, 5, 7, generator=g)                              # 3 x 3 x 35 = 315 outputs
    mom[0, 3:] = 50.0    # logvar clamps at 20
    mom[1, 3:] = -50.0   # and at -30
    noise = torch.randn(3, 3, 5, 7, generator=g)
    mean, logvar = mom[:, :3], mom[:, 3:].clamp(-30, 20)
    mg, ng = _guard.put(mom, label="moments"), _guard.put(noise, label="noise")
    out, mode = ops.gaussian_sample(mg, ng, 0.18215), ops.gaussian_sample(mg, None, 2.0)
    assert torch.allclose(out.cpu(), (mean + torch.exp(0.5 * logvar) * noise) * 0.18215, rtol=1e-5, atol=1e-6)
    assert torch.allclose(mode.cpu(), mean * 2.0, rtol=1e-6, atol=0)
    with _guard.plain(ops):
        assert torch.equal(ops.gaussian_sample(mom.cuda(), noise.cuda(), 0.18215), out) and torch.equal(ops.gaussian_sample(mom.cuda(), None, 2.0), mode)
    _guard.verify()


@pytest.mark.parametrize("E,n", [(3, 77), (2, 1001)])
def test_ensemble_variance_sum_at_a_size_not_a_multiple_of_four(E, n, ops):
    x = _members((E, n), seed=E + n)
    ref = float(x.double().var(dim=0, unbiased=True).sum())
    got = ops.ensemble_variance_sum(_guard.put(x, label="members"))
    assert abs(got - ref) <= 1e-5 * abs(ref)
    with _guard.plain(ops):
        assert ops.ensemble_variance_sum(x.cuda()) == got
    _guard.verify()
