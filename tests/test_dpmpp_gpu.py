"""DPM-Solver++(2M) on the MI355X: the two update kernels inside guard arenas (tests/_guard.py) against float64, their refusals, the sampler's
generic path on an analytic denoiser against the float64 recurrence, both paths on the tiny seeded UNet against the CPU oracle run through
tests/_dpmpp_ref.sample_with, graph replay, and `vista_amd.step_sweep` end to end on the tiny pipeline of the other front-door tests.

Bounds: the kernels take the per-element fp32 rounding bounds written out below; the analytic run takes 1e-4 (about 8 fp32 roundings per step x
20 steps x an amplification 1 + 1/r <= 2.5 of the history term on this schedule at n >= 10 = 3e-5 relative, doubled and rounded up); the UNet
runs take measured + 25 % (profiles/dpmpp2m_parity.txt). Nothing here reads the reference tree."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _dpmpp_ref as R
from tests import _guard as G
from tests.test_frontdoor_gpu import H, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
WRAP = 256 * 16 * 256   # elements one pass of the elementwise grid covers (csrc/elementwise.hip: ew_grid caps the grid at 256 * 16 blocks of 256)
U = 2.0 ** -24          # fp32 unit roundoff
EINVAL = -22
P = "vwm.modules.diffusionmodules."
EDM = {"target": P + "discretizer.EDMDiscretization", "params": {"sigma_min": 0.002, "sigma_max": 700.0, "rho": 7.0}}


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _triples():
    """(first, (a, b, c)) x 3 from the shipped 10-step schedule, rounded to fp32 as the kernels receive them: the first step, a second-order step
    and the final step."""
    from vista_amd.modules.diffusionmodules import sampling
    coef = sampling.dpmpp2m_coefficients(R.edm_sigmas_f64(10))
    f32 = lambda t: tuple(float(np.float32(v)) for v in t)   # noqa: E731
    return [(1, f32(coef[0])), (0, f32(coef[4])), (0, f32(coef[-1]))]


# ---- 1. the fused step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn,Hh,Ww,ld", [(29, 1, 9041, 4), (5, 11, 13, 8)], ids=["29x9041x4_wraps", "5x143x8_odd_padded"])
def test_sampler_update_2m_against_float64(Tn, Hh, Ww, ld):
    from vista_amd import ops
    assert (Tn * 4 * Hh * Ww > WRAP) == (ld == 4)
    HW = Hh * Ww
    c_out, c_skip = -0.9, 0.2
    x0, net = _randn(Tn, 4, Hh, Ww, seed=Tn + HW, scale=3.0), _randn(2 * Tn, HW, ld, seed=ld + HW)
    h0, s = _randn(Tn, 4, Hh, Ww, seed=7 + HW, scale=2.0), torch.linspace(1.0, 2.5, Tn)
    d = lambda t: t.double()   # noqa: E731
    untok = lambda z: z[..., :4].reshape(Tn, Hh, Ww, 4).permute(0, 3, 1, 2)   # noqa: E731
    nu, nc = untok(d(net)[:Tn]) * c_out, untok(d(net)[Tn:]) * c_out
    sv = d(s).view(-1, 1, 1, 1)
    du, dc = nu + d(x0) * c_skip, nc + d(x0) * c_skip
    g64 = du + sv * (dc - du)
    g_tol = 4 * U * (nu.abs() + nc.abs() + (d(x0) * c_skip).abs()) * (1 + 2 * sv.abs())   # five roundings of g and their way through the blend
    for first, (a, b, c) in _triples():
        old = torch.zeros_like(g64) if first else d(h0)
        want = a * d(x0) + b * g64 + c * old
        tol = 3 * U * ((a * d(x0)).abs() + (b * g64).abs() + (c * old).abs()) + (abs(b) + abs(c)) * g_tol   # 1.5 * 2^-23 = 3 U: three roundings
        runs = []
        for _ in range(2):
            with G.guarded(ops):
                x = G.scratch(G.put(x0), "x")
                hist = G.empty(x0.shape, F32, label="hist") if first else G.scratch(G.put(h0), "hist")   # first: left poisoned (NaN bytes)
                out = ops.sampler_update_2m(x, G.put(net), G.put(s), hist, c_out, c_skip, a, b, c, first=bool(first))
                assert out is x
                runs.append((x.cpu(), hist.cpu()))
                G.verify()
        (gx, gh), (gx2, gh2) = runs
        assert torch.equal(gx, gx2) and torch.equal(gh, gh2), "two runs, the same bits"
        assert torch.isfinite(gx).all() and torch.isfinite(gh).all()
        ex, eh = ((d(gx) - want).abs() / tol).max().item(), ((d(gh) - g64).abs() / g_tol).max().item()
        print(f"UPDATE2M {Tn}x{HW}x{ld} first={first} (a, b, c)=({a:.4g}, {b:.4g}, {c:.4g}): x err/tol {ex:.3f}, hist err/tol {eh:.3f}")
        assert ex <= 1.0 and eh <= 1.0
        if (a, b, c) == (0.0, 1.0, 0.0):
            assert torch.equal(gx, gh), "the final triple: x' is the denoised value exactly"


# ---- 2. the generic step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [WRAP + 7, 143], ids=["wrap_plus_7", "143"])
def test_dpmpp2m_step_against_float64(n):
    from vista_amd import ops
    x0, den, old = _randn(n, seed=n, scale=3.0), _randn(n, seed=n + 1), _randn(n, seed=n + 2)
    d = lambda t: t.double()   # noqa: E731
    for _first, (a, b, c) in _triples():
        for with_old in (False, True):
            want = a * d(x0) + b * d(den) + (c * d(old) if with_old else 0.0)
            tol = 3 * U * ((a * d(x0)).abs() + (b * d(den)).abs() + ((c * d(old)).abs() if with_old else 0.0))
            with G.guarded(ops):
                dx, dd, do = G.put(x0), G.put(den), (G.put(old) if with_old else None)
                fresh = ops.dpmpp2m_step(dx, dd, do, a, b, c)
                xs = G.scratch(dx, "x")
                same = ops.dpmpp2m_step(xs, dd, do, a, b, c, out=xs)
                assert same is xs and fresh.data_ptr() != dx.data_ptr()
                got, inplace = fresh.cpu(), xs.cpu()
                G.verify()
            assert torch.equal(got, inplace), "out == x gives the same bits"
            err = ((d(got) - want).abs() / tol.clamp_min(1e-300)).max().item()
            print(f"STEP2M n={n} old={with_old} (a, b, c)=({a:.4g}, {b:.4g}, {c:.4g}): err/tol {err:.3f}")
            assert torch.isfinite(got).all() and err <= 1.0
            if (a, b, c) == (0.0, 1.0, 0.0) and not with_old:
                assert torch.equal(got, den)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_einval_without_a_launch_and_the_wrappers_name_the_operand():
    from vista_amd import _lib, ops
    lib = _lib.load()
    Tn, Hh, Ww = 2, 4, 8
    HW = Hh * Ww
    f = C.c_float
    with G.guarded(ops):
        x0 = G.put(_randn(Tn, 4, Hh, Ww, seed=1))
        x = G.scratch(x0, "x")
        net, s = G.put(_randn(2 * Tn, HW, 8, seed=2)), G.put(_randn(Tn, seed=3))
        hist, out = G.empty((Tn, 4, Hh, Ww), F32, label="hist"), G.empty((Tn * 4 * HW,), F32, label="out")
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
        st = ops._stream()
        upd = lambda px, pn, ps, ph, t=Tn, hw=HW, ld=8: lib.vk_sampler_update_2m(px, pn, ps, ph, t, hw, ld, f(1.0), f(0.5), f(0.5), f(0.6), f(-0.1), 0, st)   # noqa: E731
        assert upd(None, p(net), p(s), p(hist)) == EINVAL and upd(p(x), None, p(s), p(hist)) == EINVAL
        assert upd(p(x), p(net), None, p(hist)) == EINVAL and upd(p(x), p(net), p(s), None) == EINVAL
        assert upd(p(x), p(net), p(s), p(hist), t=0) == EINVAL and upd(p(x), p(net), p(s), p(hist), t=-1) == EINVAL
        assert upd(p(x), p(net), p(s), p(hist), hw=0) == EINVAL and upd(p(x), p(net), p(s), p(hist), ld=3) == EINVAL
        assert upd(p(x), p(net), p(s), p(x)) == EINVAL, "hist == x"
        for k in range(4):
            args = [p(x), p(net), p(s), p(hist)]
            args[k] = p((x, net, s, hist)[k], 2)
            assert upd(*args) == EINVAL, f"operand {k} two bytes off"
        step = lambda px, pd, po, pout, n=Tn * 4 * HW: lib.vk_dpmpp2m_step(px, pd, po, pout, f(0.5), f(0.6), f(-0.1), n, st)   # noqa: E731
        assert step(None, p(net), None, p(out)) == EINVAL and step(p(x), None, None, p(out)) == EINVAL and step(p(x), p(net), None, None) == EINVAL
        assert step(p(x), p(net), None, p(out), n=0) == EINVAL and step(p(x), p(net), None, p(out), n=-5) == EINVAL
        for k in range(4):
            args = [p(x), p(net), p(hist), p(out)]
            args[k] = p((x, net, hist, out)[k], 2)
            assert step(*args) == EINVAL, f"operand {k} two bytes off"
        # the wrappers, as tests/test_operands_gpu.py does for sampler_update: a ValueError that starts with the operand's name
        good_hist = G.scratch(x0, "hist")
        for name, call in (("net_out", lambda: ops.sampler_update_2m(x, net[:Tn], s, good_hist, 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("scale", lambda: ops.sampler_update_2m(x, net, s[:1], good_hist, 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("net_out", lambda: ops.sampler_update_2m(x, net.to(BF16), s, good_hist, 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("hist", lambda: ops.sampler_update_2m(x, net, s, good_hist[:1], 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("hist", lambda: ops.sampler_update_2m(x, net, s, good_hist.reshape(Tn, 4, Ww, Hh), 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("hist", lambda: ops.sampler_update_2m(x, net, s, x, 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("x", lambda: ops.sampler_update_2m(x[:, :3], net, s, good_hist, 1.0, 0.5, 0.5, 0.6, -0.1, False)),
                           ("den", lambda: ops.dpmpp2m_step(x, good_hist[:1], None, 0.5, 0.6, -0.1)),
                           ("den_old", lambda: ops.dpmpp2m_step(x, good_hist, good_hist.to(BF16), 0.5, 0.6, -0.1)),
                           ("out", lambda: ops.dpmpp2m_step(x, good_hist, None, 0.5, 0.6, -0.1, out=good_hist.view(-1))),
                           ("x", lambda: ops.dpmpp2m_step(x.to(BF16), good_hist, None, 0.5, 0.6, -0.1))):
            with pytest.raises(ValueError, match=f"^{name}: "):
                call()
        torch.cuda.synchronize()
        assert torch.isnan(hist).all() and torch.isnan(out).all(), "a refused call launches nothing: the outputs keep their poison"
        assert torch.equal(x, x0) and torch.equal(good_hist, x0)
        G.verify()
    with pytest.raises(_lib.VistaHipError):
        ops.dpmpp2m_step(torch.zeros(4), torch.zeros(4), None, 0.5, 0.5, 0.0)


# ---- 4. the generic path on the analytic denoiser --------------------------------------------------------------------------------------------------
def test_generic_path_on_the_analytic_denoiser_against_the_float64_recurrence():
    from vista_amd.modules.diffusionmodules.sampling import DPMPP2MSampler
    steps, s_data = 20, 1.0
    sampler = DPMPP2MSampler(EDM, num_steps=steps)   # no guider config: IdentityGuider
    noise, cond_frame = _randn(5, 4, 16, 32, seed=11), _randn(5, 4, 16, 32, seed=12, scale=0.8)
    mask = torch.tensor([1.0, 0, 0, 0, 0])
    seen = []

    def denoiser(x, sigma, cond, cond_mask):
        seen.append(float(sigma[0]))
        return x * (s_data ** 2 / (s_data ** 2 + sigma ** 2)).view(-1, 1, 1, 1)
    x_in = noise.clone().cuda()
    got = sampler(denoiser, x_in, cond={}, cond_frame=cond_frame.cuda(), cond_mask=mask.cuda()).cpu()
    sig = sampler.host_sigmas()
    assert len(seen) == steps and seen == [float(v) for v in sig[:-1]], "one denoiser evaluation per step"
    assert torch.equal(x_in.cpu(), noise * torch.sqrt(1.0 + sig[0] ** 2)), "the caller's noise is scaled in place"
    sig64 = sig.double().numpy()
    want = torch.from_numpy(R.sample_f64(R.gaussian_denoiser(s_data), noise.double().numpy() * math.sqrt(1.0 + sig64[0] ** 2), sig64, "2m",
                                         cond_frame.double().numpy(), mask.double().numpy()))
    rel = ((got.double() - want)[1:].norm() / want[1:].norm()).item()
    euler = torch.from_numpy(R.sample_f64(R.gaussian_denoiser(s_data), noise.double().numpy() * math.sqrt(1.0 + sig64[0] ** 2), sig64, "euler",
                                          cond_frame.double().numpy(), mask.double().numpy()))
    print(f"GENERIC2M analytic denoiser, {steps} steps: rel-L2 from the float64 recurrence {rel:.3e} (bound 1e-4); "
          f"the float64 Euler run lies {((euler - want)[1:].norm() / want[1:].norm()).item():.3e} away")
    assert torch.isfinite(got).all() and rel <= 1e-4
    assert torch.equal(got[0], cond_frame[0]), "the conditioning frame is cond_frame, bit for bit"


# ---- 5. the tiny UNet against the CPU oracle -------------------------------------------------------------------------------------------------------
STEPS = 4   # one first-order step, two second-order steps, the final step
# rel-L2 from the oracle run, measured on the MI355X (profiles/dpmpp2m_parity.txt); the asserted bound is measured + 25 % (README, round 6)
# (the two paths agree bit for bit at this size, so their figures are equal; Euler beside them, printed and not asserted: 1.4197e-2 / 1.1943e-2)
MEASURED_2M = {("VanillaCFG", "fused"): 2.7576e-2, ("VanillaCFG", "generic"): 2.7576e-2,                                  # bound 3.4470e-2
               ("TrianglePredictionGuider", "fused"): 2.1937e-2, ("TrianglePredictionGuider", "generic"): 2.1937e-2}      # bound 2.7421e-2
_ORACLE = {}


def _guider(name):
    if name == "VanillaCFG":
        return {"target": P + "guiders.VanillaCFG", "params": {"scale": 2.5}}
    return {"target": P + "guiders." + name, "params": {"max_scale": 2.5, "min_scale": 1.0, "num_frames": T}}


def _window():
    from vista_amd import synth
    return synth.window_inputs(T=T, H=H // 8, W=W // 8, seed=41, n_cond=1, trajectory=[0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2])


def _oracle(model, guider):
    """The CPU oracle's 4-step runs of both updates, once per guider and process."""
    from oracle import vista_oracle as O
    if guider not in _ORACLE:
        sd = {k: v.detach().float().cpu() for k, v in model.model.diffusion_model.state_dict().items()}
        w = _window()
        scale = 2.5 if guider == "VanillaCFG" else O.triangle_guider_scale(T)
        fn = lambda a, s, c, m: O.denoiser_forward(sd, a, s, c, m, T)   # noqa: E731
        with torch.no_grad():
            two = R.sample_with(fn, "2m", w["noise"], w["c"], w["uc"], w["cond_frame"], w["cond_mask"], STEPS, scale=scale)
            euler = O.euler_edm_sample(fn, w["noise"], w["c"], w["uc"], w["cond_frame"], w["cond_mask"], STEPS, scale=scale)
        _ORACLE[guider] = {"DPMPP2MSampler": two, "EulerEDMSampler": euler}
    return _ORACLE[guider]


def _sampler(name, guider, steps=STEPS):
    from vista_amd.modules.diffusionmodules import sampling
    if name == "DPMPP2MSampler":
        return sampling.DPMPP2MSampler(EDM, num_steps=steps, guider_config=_guider(guider))
    return sampling.EulerEDMSampler(num_steps=steps, discretization_config=EDM, guider_config=_guider(guider), s_churn=0.0, s_tmin=0.0, s_tmax=999.0,
                                    s_noise=1.0)


def _gpu_run(model, name, guider, path, graph=False, steps=STEPS, x_out=None):
    from vista_amd import sample_utils as SU
    w = _window()
    cu = lambda dct: {k: v.cuda() for k, v in dct.items()}   # noqa: E731
    s = _sampler(name, guider, steps)
    s.graph = s.cfg_streams = graph
    x = w["noise"].clone().cuda()
    got = s(SU.rollout_denoiser(model, fused=(path == "fused")), x, cond=cu(w["c"]), uc=cu(w["uc"]), cond_frame=w["cond_frame"].cuda(),
            cond_mask=w["cond_mask"].cuda())
    if x_out is not None:
        x_out.append(x.cpu())
    return got.cpu()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("guider", ["VanillaCFG", "TrianglePredictionGuider"])
def test_both_paths_on_the_tiny_unet_against_the_cpu_oracle(world, model, guider):
    from oracle import vista_oracle as O
    w, want = _window(), _oracle(model, guider)
    got, scaled = {}, []
    for name in ("DPMPP2MSampler", "EulerEDMSampler"):
        for path in ("fused", "generic"):
            got[name, path] = _gpu_run(model, name, guider, path, x_out=scaled)
            r = _rel(got[name, path], want[name])
            print(f"PARITY2M {guider} {name} {path} {STEPS} steps: rel-L2 from the CPU oracle {r:.4e}")
        print(f"PARITY2M {guider} {name}: fused against generic {_rel(got[name, 'fused'], got[name, 'generic']):.4e}")
    print(f"PARITY2M {guider}: the oracle's 2M run lies {_rel(want['DPMPP2MSampler'], want['EulerEDMSampler']):.4e} from its Euler run")
    s0 = torch.sqrt(1.0 + O.edm_sigmas(STEPS)[0] ** 2)
    for x in scaled:
        assert torch.equal(x, w["noise"] * s0), "the caller's noise is scaled in place, as for Euler"
    for path in ("fused", "generic"):
        out = got["DPMPP2MSampler", path]
        assert torch.isfinite(out).all() and torch.equal(out[0], w["cond_frame"][0]), "conditioning frames are cond_frame, bit for bit"
        r, bound = _rel(out, want["DPMPP2MSampler"]), 1.25 * MEASURED_2M[guider, path]
        assert r <= bound, (guider, path, r, bound)


# ---- 6. graph replay -------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_leaves_the_shared_graph_cache_to_euler(world, model):
    eager = _gpu_run(model, "DPMPP2MSampler", "VanillaCFG", "fused", graph=False)
    replay = _gpu_run(model, "DPMPP2MSampler", "VanillaCFG", "fused", graph=True)
    assert torch.equal(replay, eager)
    cache = model.model.diffusion_model.__dict__.get("_hipgraph_cache", {})
    keys = set(cache)
    assert keys, "the graph path ran"
    e_eager = _gpu_run(model, "EulerEDMSampler", "VanillaCFG", "fused", graph=False)
    e_replay = _gpu_run(model, "EulerEDMSampler", "VanillaCFG", "fused", graph=True)
    assert torch.equal(e_replay, e_eager), "an Euler run through the graphs the 2M run captured"
    assert set(cache) == keys, "the update is outside the graph: the same keys serve both samplers"
    assert not torch.equal(e_eager, eager)


# ---- 7. the front door -----------------------------------------------------------------------------------------------------------------------------
BOTH = ["EulerEDMSampler", "DPMPP2MSampler"]


def _sweep(model, world, **kw):
    from vista_amd import sample, step_sweep
    sample.seed_everything(23)
    return step_sweep.run(model, world["frames"], None, height=H, width=W, n_frames=T, cond_aug=0.02, **kw)


def test_step_sweep_run_reports_every_field(world, model):
    from vista_amd import step_sweep
    rep = _sweep(model, world, samplers=BOTH, budgets=[2, 4], ref_steps=8)
    assert isinstance(rep, step_sweep.SweepReport) and (rep.ref_sampler, rep.ref_steps, rep.cond) == ("DPMPP2MSampler", 8, [0])
    assert math.isfinite(rep.ref_gap) and rep.ref_gap > 0 and rep.ref_seconds > 0
    assert [(r["sampler"], r["steps"]) for r in rep.runs] == [(s, n) for s in BOTH for n in (2, 4)]
    for r in rep.runs:
        assert sorted(r) == sorted(step_sweep.RUN_FIELDS) and len(r["frame_err"]) == T
        assert r["frame_err"][0] == 0.0 and all(math.isfinite(v) and v > 0 for v in r["frame_err"][1:]), "the conditioning frame reports exactly 0"
        assert r["latent_err"] == step_sweep.clip_error(r["frame_err"], [0]) > 0
        assert math.isfinite(r["mean_psnr"]) and 0 < r["mean_ssim"] <= 1 and r["seconds"] > 0
        print(f"SWEEP {r['sampler']} {r['steps']} steps: latent_err {r['latent_err']:.4e} psnr {r['mean_psnr']:.2f} ssim {r['mean_ssim']:.4f}")
    print(f"SWEEP ref_gap {rep.ref_gap:.4e}")
    rec = step_sweep.make_record(0, world["frames"], rep, {"seed": 23})
    assert sorted(rec) == ["cond", "frames", "index", "ref_gap", "ref_sampler", "ref_seconds", "ref_steps", "runs", "seed", "settings"]
    json.dumps(rec, allow_nan=False)
    # the reference sampler's run at ref_steps, made again: the same bits, so no distance at all
    again = _sweep(model, world, samplers=["DPMPP2MSampler"], budgets=[8], ref_steps=8)
    (r,) = again.runs
    assert r["latent_err"] == 0.0 and r["frame_err"] == [0.0] * T and r["mean_psnr"] is None and abs(r["mean_ssim"] - 1.0) <= 1e-6
    assert again.ref_gap == rep.ref_gap


def test_step_sweep_cli_writes_both_files_and_starts_them_anew(world, model):
    save = str(world["dir"] / "sweep_out")
    base = [sys.executable, "-m", "vista_amd.step_sweep", "--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES",
            "--data_root", world["data_root"], "--anno_file", world["anno"], "--n_frames", str(T), "--height", str(H), "--width", str(W),
            "--cond_aug", "0.02", "--n_scenes", "1", "--save", save, "--ref_steps", "2"]
    for extra, steps in ((["--samplers", "EulerEDMSampler,DPMPP2MSampler", "--budgets", "2"], 2), (["--samplers", "EulerEDMSampler", "--budgets", "1", "--eager"], 1)):
        res = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        with open(os.path.join(save, "steps.jsonl")) as f:
            records = [json.loads(line) for line in f]
        with open(os.path.join(save, "steps_summary.json")) as f:
            summary = json.load(f)
        assert len(records) == 1 and summary["scenes"] == 1, "both files describe one run"
        rec = records[0]
        assert rec["index"] == 0 and rec["seed"] == 23 and rec["frames"] == [world["frames"][0]] and rec["cond"] == [0]
        assert rec["settings"]["budgets"] == [steps] and [r["steps"] for r in rec["runs"]] == [steps] * len(rec["settings"]["samplers"])
        assert [(r["sampler"], r["steps"]) for r in summary["runs"]] == [(r["sampler"], r["steps"]) for r in rec["runs"]]
        assert len(summary["equal_error"]) == len(rec["runs"])
    want = _sweep(model, world, samplers=["EulerEDMSampler"], budgets=[1], ref_steps=2, eager=True)
    assert rec["runs"][0]["frame_err"] == want.runs[0]["frame_err"] and rec["ref_gap"] == want.ref_gap, "the CLI writes what run() returns"


def test_the_environment_hook_reaches_sample_run(world, model, monkeypatch):
    from vista_amd import sample

    def run(**kw):
        torch.manual_seed(9)
        return sample.run(model, world["frames"], None, height=H, width=W, n_frames=T, n_steps=3, cond_aug=0.02, **kw)
    monkeypatch.delenv("VISTA_SAMPLER", raising=False)
    euler, named = run(), run(sampler="DPMPP2MSampler")
    monkeypatch.setenv("VISTA_SAMPLER", "DPMPP2MSampler")
    hooked = run()
    for a, b in zip(hooked, named):
        assert torch.equal(a, b)
    assert not torch.equal(named[1], euler[1]) and torch.equal(run(sampler="EulerEDMSampler")[1], euler[1])


def test_a_session_its_forks_and_a_planner_keep_the_sampler_they_were_built_with(world, model, monkeypatch):
    from vista_amd import drive, plan, sample
    from vista_amd.modules.diffusionmodules import sampling
    kw = dict(height=H, width=W, n_frames=T, n_steps=3, cond_aug=0.02)
    monkeypatch.delenv("VISTA_SAMPLER", raising=False)
    torch.manual_seed(9)
    named = drive.DriveSession(model, world["frames"], guider="VanillaCFG", sampler="DPMPP2MSampler", **kw)
    after_construction = torch.cuda.get_rng_state()   # (the sessions built below draw their own cond_aug noise from the same generator)
    assert type(named.sampler) is sampling.DPMPP2MSampler and named.sampler_name == "DPMPP2MSampler"
    assert type(drive.DriveSession(model, world["frames"], **kw).sampler) is sampling.EulerEDMSampler, "unset: the reference's sampler"
    monkeypatch.setenv("VISTA_SAMPLER", "EulerEDMSampler")   # the hook changing later does not reach a session that exists
    branch = named.fork()
    assert branch.sampler is named.sampler and branch.sampler_name == "DPMPP2MSampler"
    assert type(plan.Planner(named, ens_size=2, score_steps=2).sampler) is sampling.EulerEDMSampler, "sampler=None: the hook"
    assert type(plan.Planner(named, ens_size=2, score_steps=2, sampler="DPMPP2MSampler").sampler) is sampling.DPMPP2MSampler
    monkeypatch.setenv("VISTA_SAMPLER", "DPMPP2MSampler")
    assert type(drive.DriveSession(model, world["frames"], **kw).sampler) is sampling.DPMPP2MSampler
    assert type(plan.Planner(named, ens_size=2, score_steps=2).sampler) is sampling.DPMPP2MSampler
    # the session's first round is sample.run's single round: the same draws in the same order, the same sampler
    torch.cuda.set_rng_state(after_construction)
    latents = branch.step(None).latents
    torch.manual_seed(9)
    want = sample.run(model, world["frames"], None, sampler="DPMPP2MSampler", **kw)[1]
    assert torch.equal(latents, want)
