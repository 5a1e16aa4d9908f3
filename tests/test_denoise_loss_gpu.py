"""The denoising-loss front door on the MI355X: the three entry points of csrc/loss.hip inside guard arenas (tests/_guard.py: poisoned outputs,
guard bands around every tensor), StandardDiffusionLoss fed the draws a CPU run of the reference made (tests/golden/diffusion_loss_tiny.pt), and
`vista_amd.denoise_loss` end to end on the tiny seeded pipeline of the other front-door tests.

Yardsticks: the noising is bitwise torch's fp32 expression on the CPU; everything else is held to tests/_loss_ref.py (float64). The statistics and
the losses take the CPU test's bound (R.LOSS_BOUND: 8 x the reference's own measured distance from float64); the high-pass takes 16 x the distance
of the reference's own fp32 torch.fft path from float64 on the same planes (max |y - y64| / rms(x) per plane). Measured figures:
profiles/diffusion_loss_parity.txt. Nothing here reads the reference tree."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _guard as G
from tests import _loss_ref as R
from tests.test_frontdoor_gpu import H, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = torch.float32


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLD, "diffusion_loss_tiny.pt"))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- noising ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10])
@pytest.mark.parametrize("hw,skew", [((8, 16), 0), ((5, 7), 0), ((8, 16), 4)], ids=["hw128", "hw35_scalar", "hw128_skewed"])
@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
def test_noising_is_bitwise_torchs_fp32_expression(n, hw, skew, with_offset, with_mask):
    from vista_amd import ops
    h, w = hw
    x, noise = _randn(n, 4, h, w, seed=1), _randn(n, 4, h, w, seed=2)
    sigma = _randn(n, seed=3).mul(1.6).add(1.0).exp()
    mask = (torch.arange(n) % 3 == 0).float() if with_mask else None
    offset = _randn(n, 4, seed=4) if with_offset else None
    want = R.noised_input_f32(x, noise, sigma, mask, offset, 0.02)
    with G.guarded(ops):
        dx, dn = G.put(x, skew=skew), G.put(noise, skew=skew)
        out = G.empty(x.shape, F32, skew=skew) if skew else None
        got = ops.loss_noise_input(dx, dn, G.put(sigma), None if mask is None else G.put(mask), None if offset is None else G.put(offset),
                                   0.02, out=out)
        assert got.data_ptr() % 16 == skew
        res = got.cpu()
        G.verify()
    assert torch.equal(res, want), int((res != want).sum())


# ---- Fourier high-pass ------------------------------------------------------------------------------------------------------------------------
def _keep(Hh, Ww):
    from vista_amd.modules.diffusionmodules.util import fourier_keep_mask
    return fourier_keep_mask(Hh, Ww)


def _highpass(x, scale, b=None, cond_mask=None):
    from vista_amd import ops
    with G.guarded(ops):
        keep = G.put(_keep(*x.shape[-2:]))
        y = ops.fourier_highpass(G.put(x), keep, scale, b=None if b is None else G.put(b), cond_mask=None if cond_mask is None else G.put(cond_mask))
        res = y.cpu()
        G.verify()
    return res


@pytest.mark.parametrize("scale", [0.0, 0.5])
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 3, 8, 16), (2, 3, 5, 7), (2, 3, 1, 1), (2, 3, 1, 12), (1, 4, 72, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_highpass_against_float64_within_16x_the_reference_fft_path(shape, scale, golden):
    """Golden shapes: the planes and the reference's outputs come from the golden; 72 x 128 (too large to commit): unit-normal planes, and the
    reference's figure is that of the fp32 torch.fft path recomputed here on the CPU."""
    Hh, Ww = shape[-2:]
    entry = [f for f in golden["fourier_filter"] if (f["H"], f["W"], f["scale"]) == (Hh, Ww, scale)]
    x = entry[0]["x"] if entry else _randn(*shape, seed=9)
    y_ref32 = entry[0]["y"] if entry else R.fourier_filter(x, scale, dtype=F32)
    y64 = R.fourier_filter(x, scale)
    ref_err = R.filter_error(y_ref32, y64, x).max().item()
    got = _highpass(x, scale)
    err = R.filter_error(got, y64, x).max().item()
    err_golden = R.filter_error(got, y_ref32.double(), x).max().item()
    print(f"HIGHPASS {Hh}x{Ww} scale={scale}: kernel vs f64 {err:.3e}, reference fp32 vs f64 {ref_err:.3e}, kernel vs reference {err_golden:.3e}")
    assert torch.isfinite(got).all()
    assert err <= R.HIGHPASS_FACTOR * ref_err, (err, ref_err)
    if entry:   # against the golden's reference outputs with the same bound
        assert err_golden <= R.HIGHPASS_FACTOR * ref_err, (err_golden, ref_err)


def test_highpass_of_the_fused_difference_and_masked_frames_are_exactly_zero():
    n, Cn, Hh, Ww = 4, 4, 8, 16
    out, target = _randn(n, Cn, Hh, Ww, seed=5), _randn(n, Cn, Hh, Ww, seed=6)
    m = torch.tensor([1.0, 0.0, 1.0, 0.0])
    mm = m[:, None, None, None]
    for mask in (None, m):
        d = (out - target) if mask is None else (out * (1 - mm) + target * mm) - target   # fp32, as the kernel forms it on load
        got = _highpass(out, 0.0, b=target, cond_mask=mask)
        y64 = R.fourier_filter(d, 0.0)
        ref_err = R.filter_error(R.fourier_filter(d, 0.0, dtype=F32), y64, torch.where(d.abs().sum((-2, -1), keepdim=True) > 0, d, torch.ones_like(d)))
        err = R.filter_error(got, y64, torch.where(d.abs().sum((-2, -1), keepdim=True) > 0, d, torch.ones_like(d)))
        assert err.max().item() <= R.HIGHPASS_FACTOR * ref_err.max().item(), (err.max().item(), ref_err.max().item())
        if mask is not None:
            assert torch.equal(got[0], torch.zeros_like(got[0])) and torch.equal(got[2], torch.zeros_like(got[2]))
            assert got[1].abs().max() > 0


def test_highpass_plane_does_not_depend_on_the_batch():
    x = _randn(5, 4, 8, 16, seed=8)
    assert torch.equal(_highpass(x, 0.0)[3], _highpass(x[3:4].clone(), 0.0)[0])


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------
def _stats(out, target, Tn, mask=None, hf=None, l1=False):
    from vista_amd import ops
    with G.guarded(ops):
        s = ops.loss_stats(G.put(out), G.put(target), Tn, cond_mask=None if mask is None else G.put(mask), hf=None if hf is None else G.put(hf), l1=l1)
        res = s.cpu()
        G.verify()
    return res


def _clip(B, Tn, h, w, seed):
    """A target that moves a little from frame to frame and an output that is off by a tenth of it."""
    target = (_randn(B, 1, 4, h, w, seed=seed) + 0.3 * _randn(B, Tn, 4, h, w, seed=seed + 1).cumsum(1)).reshape(B * Tn, 4, h, w).contiguous()
    return target + 0.1 * _randn(B * Tn, 4, h, w, seed=seed + 2), target


def _close(got, ref, what):
    got, ref = got.double(), ref.double()
    zero = ref == 0
    assert torch.equal(got[zero], ref[zero]), (what, "exact zeros")
    worst = ((got - ref).abs()[~zero] / ref.abs()[~zero]).max().item() if (~zero).any() else 0.0
    print(f"LOSSSTATS {what}: worst relative distance from float64 {worst:.3e} (bound {R.LOSS_BOUND:.3e})")
    assert worst <= R.LOSS_BOUND, (what, worst)


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("B,Tn", [(2, 5), (1, 1), (3, 2)])
@pytest.mark.parametrize("hw", [(8, 16), (5, 7), (8, 8)], ids=["hw128", "hw35", "hw64"])
def test_statistics_against_float64(B, Tn, hw, l1):
    out, target = _clip(B, Tn, *hw, seed=20)
    mask = (torch.arange(B * Tn) % Tn == 0).float() if Tn > 1 else torch.zeros(B * Tn)
    mm = mask[:, None, None, None]
    d32 = (out * (1 - mm) + target * mm) - target
    hf = R.fourier_filter(d32, 0.0).float()   # (the statistics kernel is judged on its own: its hf operand is the yardstick's, rounded)
    got = _stats(out, target, Tn, mask, hf, l1)
    want = R.frame_sums(out, target, Tn, mask, l1, True)
    want[:, 2] = (hf.double().abs() if l1 else hf.double() ** 2).reshape(B * Tn, -1).sum(1)
    _close(got, want, f"B{B} T{Tn} {hw} {'l1' if l1 else 'l2'}")
    if Tn == 1:
        assert torch.equal(got[:, 0], got[:, 1]), "T = 1 has no differences: aux_w is 1 everywhere"
    else:
        assert torch.equal(got[::Tn], torch.zeros_like(got[::Tn])), "frames with m = 1 give exactly 0 in all three sums"
    # without a mask and without hf
    plain = _stats(out, target, Tn, None, None, l1)
    want = R.frame_sums(out, target, Tn, None, l1, True)
    want[:, 2] = 0
    _close(plain, want, "no mask, no hf")


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_statistics_zero_norm_gives_unit_weight_not_nan(l1):
    """Predicted dynamics equal the target's (the output is the target plus a constant per clip): every dd is 0, the norm is exactly 0."""
    _, target = _clip(2, 4, 8, 16, seed=30)
    shift = _randn(2, 1, 4, 8, 16, seed=33).expand(2, 4, 4, 8, 16).reshape(8, 4, 8, 16)
    # rounding must not break the equality of the dynamics: quantise so that every sum and difference below is exact in fp32
    target, shift = (target * 64).round() / 64, (shift * 64).round() / 64
    got = _stats(target + shift, target, 4, None, None, l1)
    assert torch.isfinite(got).all() and torch.equal(got[:, 0], got[:, 1]) and bool((got[:, 0] > 0).all())


def test_statistics_of_a_frame_do_not_depend_on_the_batch():
    out, target = _clip(3, 5, 8, 16, seed=40)
    mask = (torch.arange(15) % 5 < 2).float()
    hf = _randn(15, 4, 8, 16, seed=44)
    all3 = _stats(out, target, 5, mask, hf)
    one = _stats(out[5:10].clone(), target[5:10].clone(), 5, mask[5:10].clone(), hf[5:10].clone())
    assert torch.equal(all3[5:10], one)


@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_statistics_at_a_skewed_pointer_equal_the_aligned_ones_bitwise(l1):
    """hw % 4 == 0 with out / target / hf off 16-byte alignment: scalar loads, the same groups and the same order of every sum."""
    from vista_amd import ops
    out, target = _clip(2, 3, 8, 16, seed=50)
    mask = (torch.arange(6) % 3 == 0).float()
    hf = _randn(6, 4, 8, 16, seed=55)
    aligned = _stats(out, target, 3, mask, hf, l1)
    for skews in ((4, 4, 4), (8, 0, 0), (0, 12, 0), (0, 0, 4)):
        with G.guarded(ops):
            o, t, h = (G.put(x, skew=s) for x, s in zip((out, target, hf), skews))
            assert [x.data_ptr() % 16 for x in (o, t, h)] == list(skews)
            got = ops.loss_stats(o, t, 3, cond_mask=G.put(mask), hf=h, l1=l1).cpu()
            G.verify()
        assert torch.equal(got, aligned), skews


# ---- the class --------------------------------------------------------------------------------------------------------------------------------
def _loss_fn(case):
    from vista_amd.modules.diffusionmodules.loss import StandardDiffusionLoss
    P = "vwm.modules.diffusionmodules."
    return StandardDiffusionLoss(
        sigma_sampler_config={"target": P + "sigma_sampling.EDMSampling", "params": {"p_mean": 1.0, "p_std": 1.6, "num_frames": case["num_frames"]}},
        loss_weighting_config={"target": P + "loss_weighting.VWeighting"}, loss_type=case["loss_type"],
        use_additional_loss=case["use_additional_loss"], offset_noise_level=case["offset_noise_level"],
        additional_loss_weight=case["additional_loss_weight"], num_frames=case["num_frames"], replace_cond_frames=case["replace_cond_frames"],
        cond_frames_choices=case["cond_frames_choices"])


def test_the_class_fed_the_references_draws_returns_the_references_losses(golden):
    from vista_amd import ops
    for i, case in enumerate(golden["cases"]):
        seen = {}

        def denoiser(network, noised_input, sigmas, cond, cond_mask):
            seen["noised"], seen["mask"] = noised_input.cpu(), cond_mask.cpu()
            return case["model_output"].cuda()
        with G.guarded(ops):
            got = _loss_fn(case)._forward(None, denoiser, {}, G.put(case["input"]), sigmas=case["sigmas"], cond_mask=case["cond_mask"],
                                          noise=case["noise"], offset=case["offset"])
            G.verify()
        assert torch.equal(seen["noised"], case["noised"]), (i, "the noised input is the reference's, bit for bit")
        assert torch.equal(seen["mask"], case["cond_mask"])
        assert got.dtype == torch.float64 and got.shape == case["loss"].shape
        r = R.rel(got, case["loss"])
        print(f"LOSSCLASS case {i} {case['loss_type']} additional={case['use_additional_loss']} replace={case['replace_cond_frames']} "
              f"T={case['num_frames']} {tuple(case['input'].shape)}: relative distance from the reference {r:.3e} (bound {R.LOSS_BOUND:.3e})")
        assert r <= R.LOSS_BOUND, (i, r)


def test_the_class_draws_in_the_references_order_and_a_perfect_denoiser_scores_exactly_zero(golden):
    case = golden["cases"][3]   # l2, additional terms, replace_cond_frames, 8 x 16
    fn = _loss_fn(case)
    x = case["input"].cuda()
    got = fn._forward(None, lambda net, noised, s, c, m: x.clone(), {}, x)
    assert got.shape == () and float(got) == 0.0
    plain = _loss_fn(golden["cases"][0])
    xs = golden["cases"][0]["input"].cuda()
    vec = plain._forward(None, lambda net, noised, s, c, m: xs.clone(), {}, xs)
    assert vec.shape == (xs.shape[0],) and torch.equal(vec, torch.zeros_like(vec))
    # get_noised_input and get_loss, the reference's two public pieces, on their own
    c0 = golden["cases"][0]
    s_bc = c0["sigmas"][:, None, None, None]
    assert torch.equal(plain.get_noised_input(s_bc.cuda(), c0["noise"].cuda(), xs).cpu(), c0["input"] + c0["noise"] * s_bc)
    w = plain.loss_weighting(c0["sigmas"])[:, None, None, None]
    direct = plain.get_loss(c0["model_output"].cuda(), xs, w)
    assert direct.shape == c0["loss"].shape and R.rel(direct, c0["loss"]) <= R.LOSS_BOUND
    # the draws: sigma sampler (CPU generator), random.choices per clip, randn_like, offset -- two runs after the same seeding agree bitwise
    import random
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        random.seed(5)
        seen = {}

        def denoiser(network, noised_input, sigmas, cond, cond_mask):
            seen.update(noised=noised_input.clone(), sigmas=sigmas.clone(), mask=cond_mask.clone())
            return noised_input * 0.5
        runs.append((fn._forward(None, denoiser, {}, x), seen))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in ("noised", "sigmas", "mask"))
    torch.manual_seed(5)
    want_sigmas = fn.sigma_sampler(x.shape[0])
    assert torch.equal(runs[0][1]["sigmas"].cpu(), want_sigmas)
    assert set(runs[0][1]["mask"].cpu().tolist()) <= {0.0, 1.0}


def test_fourier_filter_front_end_equals_the_golden(golden):
    from vista_amd.modules.diffusionmodules.util import fourier_filter
    for f in golden["fourier_filter"]:
        y64 = R.fourier_filter(f["x"], f["scale"])
        ref_err = R.filter_error(f["y"], y64, f["x"]).max().item()
        got = fourier_filter(f["x"].cuda(), f["scale"]).cpu()
        assert got.dtype == F32 and R.filter_error(got, y64, f["x"]).max().item() <= R.HIGHPASS_FACTOR * ref_err


# ---- operand refusals -------------------------------------------------------------------------------------------------------------------------
def test_operand_refusals_return_einval_and_launch_nothing():
    from vista_amd import _lib, ops
    lib = _lib.load()
    EINVAL = -22
    with G.guarded(ops):
        x = G.put(_randn(2, 4, 8, 16, seed=1))
        s = G.put(torch.ones(2))
        keep = G.put(_keep(8, 16))
        y = G.empty((2, 4, 8, 16), F32)
        sums, ws = G.empty((2, 3), torch.float64), G.empty((2 * 4 * 16,), torch.float64)
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        st = ops._stream()
        noise = lib.vk_loss_noise_input
        assert noise(None, p(x), p(s), None, None, 0.0, p(y), 2, 4, 128, st) == EINVAL
        assert noise(p(x), None, p(s), None, None, 0.0, p(y), 2, 4, 128, st) == EINVAL
        assert noise(p(x), p(x), None, None, None, 0.0, p(y), 2, 4, 128, st) == EINVAL
        assert noise(p(x), p(x), p(s), None, None, 0.0, None, 2, 4, 128, st) == EINVAL
        for n, c, hw in ((0, 4, 128), (2, 0, 128), (2, 4, 0), (-1, 4, 128)):
            assert noise(p(x), p(x), p(s), None, None, 0.0, p(y), n, c, hw, st) == EINVAL
        hp = lib.vk_fourier_highpass
        assert hp(None, None, None, p(keep), 0.0, p(y), 8, 4, 8, 16, st) == EINVAL
        assert hp(p(x), None, None, None, 0.0, p(y), 8, 4, 8, 16, st) == EINVAL
        assert hp(p(x), None, None, p(keep), 0.0, None, 8, 4, 8, 16, st) == EINVAL
        assert hp(p(x), None, p(s), p(keep), 0.0, p(y), 8, 4, 8, 16, st) == EINVAL, "a cond_mask without the second input"
        assert hp(p(x), None, None, p(keep), 0.0, p(x), 8, 4, 8, 16, st) == EINVAL, "in place"
        for planes, ppi, hh, ww in ((0, 4, 8, 16), (8, 0, 8, 16), (8, 4, 0, 16), (8, 4, 8, -1)):
            assert hp(p(x), None, None, p(keep), 0.0, p(y), planes, ppi, hh, ww, st) == EINVAL
        # an oversize plane: the first that does not fit, by either axis (72 x 128 fits; the pointers are never touched)
        assert lib.vk_fourier_highpass_lds_bytes(72, 128) == 16 * 72 * 128 + 16 * 200 and ops.fourier_highpass_fits(72, 128)
        for hh, ww in ((80, 128), (72, 144), (1, 10240), (10240, 1), (4096, 4096)):
            assert not ops.fourier_highpass_fits(hh, ww) and lib.vk_fourier_highpass_lds_bytes(hh, ww) == EINVAL
            assert hp(p(x), None, None, p(keep), 0.0, p(y), 1, 1, hh, ww, st) == EINVAL
        stats = lib.vk_loss_stats
        assert stats(None, p(x), None, None, p(sums), p(ws), 1, 2, 4, 128, 0, st) == EINVAL
        assert stats(p(x), None, None, None, p(sums), p(ws), 1, 2, 4, 128, 0, st) == EINVAL
        assert stats(p(x), p(x), None, None, None, p(ws), 1, 2, 4, 128, 0, st) == EINVAL
        assert stats(p(x), p(x), None, None, p(sums), None, 1, 2, 4, 128, 0, st) == EINVAL
        for b, t, c, hw, l1 in ((0, 2, 4, 128, 0), (1, 0, 4, 128, 0), (1, 2, 0, 128, 0), (1, 2, 4, 0, 0), (1, 2, 4, 128, 2), (1, 2, 65, 128, 0)):
            assert stats(p(x), p(x), None, None, p(sums), p(ws), b, t, c, hw, l1, st) == EINVAL
        torch.cuda.synchronize()
        assert torch.isnan(y).all() and torch.isnan(sums).all() and torch.isnan(ws).all(), "a refused call launches nothing: the outputs keep their poison"
        G.verify()
    with pytest.raises(ops.OperandError, match="does not fit"):
        ops.fourier_highpass(torch.zeros(1, 1, 80, 128, device="cuda"), torch.ones(80, 128, dtype=torch.uint8, device="cuda"), 0.0)
    with pytest.raises(_lib.VistaHipError):
        ops.loss_stats(torch.zeros(2, 4, 8, 16), torch.zeros(2, 4, 8, 16), 2)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def _report(model, world, seed=23, **kw):
    from vista_amd import denoise_loss, sample
    sample.seed_everything(seed)
    return denoise_loss.run(model, world["frames"], None, height=H, width=W, n_frames=T, n_sigmas=2, **kw)


def test_run_twice_is_identical_and_equals_the_float64_restatement_of_the_captured_outputs(world, model):
    from vista_amd import denoise_loss
    captured = {"out": [], "sigma": [], "mask": [], "z": []}
    def capture(mod, args, output):   # (returns None: a hook's return value would replace the output)
        captured["out"].append(output.float().cpu())
        captured["sigma"].append(args[2].cpu())
        captured["mask"].append(args[4].cpu())
    hook = model.denoiser.register_forward_hook(capture)
    encode = model.encode_first_stage
    model.encode_first_stage = lambda x: (captured["z"].append(encode(x)), captured["z"][-1])[1]
    try:
        first = _report(model, world)
    finally:
        hook.remove()
        del model.encode_first_stage
    again = _report(model, world)
    assert first == again and isinstance(first, denoise_loss.LossReport)
    assert first.sigmas == R.sigma_grid(2, 1.0, 1.6) == denoise_loss.sigma_grid(2) and first.cond == [0]
    assert len(captured["out"]) == 2 and len(first.frame_mse) == 2 and all(len(row) == T for row in first.frame_mse)
    z = captured["z"][0].float().cpu()
    per_image = z[0].numel()
    for i in range(2):
        mask, sig = captured["mask"][i], captured["sigma"][i]
        assert mask.tolist() == [1.0] + [0.0] * (T - 1) and torch.equal(sig, torch.full((T,), first.sigmas[i]).float())
        sums = R.frame_sums(captured["out"][i], z, T, mask, False, True)
        want = {"loss": R.assemble(sums, R.weighting("V", sig), per_image, True, 0.1).item(), "mse": (sums[:, 0].sum() / (T * per_image)).item(),
                "dynamics": (sums[:, 1].sum() / (T * per_image)).item(), "structure": (sums[:, 2].sum() / (T * per_image)).item()}
        for k, v in want.items():
            r = R.rel(getattr(first, k)[i], v)
            print(f"LOSSE2E sigma {first.sigmas[i]:.4g} {k}: {getattr(first, k)[i]:.6g} vs float64 {v:.6g}, relative {r:.3e}")
            assert r <= R.LOSS_BOUND, (k, r)
        assert R.rel(first.frame_mse[i], (sums[:, 0] / per_image).tolist()) <= R.LOSS_BOUND
        assert first.frame_mse[i][0] == 0.0 and all(v > 0 for v in first.frame_mse[i][1:]), "the conditioning frame's error is exactly 0"
    plain = _report(model, world, additional=False, weighting="Unit")
    assert plain.mse == first.mse and plain.frame_mse == first.frame_mse and plain.structure == [0.0, 0.0]
    assert R.rel(plain.loss, plain.mse) <= 1e-15, "unit weights, no additional terms: the loss is the mean squared error"


def test_cli_writes_both_files(world, model):
    save = str(world["dir"] / "loss_out")
    cmd = [sys.executable, "-m", "vista_amd.denoise_loss", "--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES",
           "--data_root", world["data_root"], "--anno_file", world["anno"], "--n_frames", str(T), "--height", str(H), "--width", str(W),
           "--n_sigmas", "2", "--rand_gen", "--save", save]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    with open(os.path.join(save, "loss.jsonl")) as f:
        records = [json.loads(line) for line in f]
    with open(os.path.join(save, "loss_summary.json")) as f:
        summary = json.load(f)
    assert len(records) == 1 and summary["scenes"] == 1
    rec = records[0]
    want = _report(model, world)
    assert rec["sigmas"] == want.sigmas and rec["loss"] == want.loss and rec["frame_mse"] == want.frame_mse and rec["cond"] == [0]
    assert rec["frames"] == [world["frames"][0]] and rec["index"] == 0 and rec["seed"] == 23 and rec["noise_seed"] == 0
    assert sorted(rec["timings"]) == ["condition", "encode", "forward", "load", "loss"]
    for k in ("loss", "mse", "dynamics", "structure"):
        assert summary[k] == rec[k] == getattr(want, k)
    assert summary["frame_mse"] == rec["frame_mse"] and summary["sigmas"] == rec["sigmas"]
