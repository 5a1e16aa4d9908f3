"""Host side of the DPM-Solver++(2M) sampler and of `vista_amd.step_sweep`: the yardstick's scaffolding against the oracle, the coefficients,
the order of the method on an analytic denoiser, the sampler factory and its environment hook, the sweep's parser, refusals and summary. No GPU."""
import math
import os
import re

import pytest
import torch

from tests import _dpmpp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("EulerEDMSampler", "DPMPP2MSampler")


# ---- 1. the yardstick's scaffolding ------------------------------------------------------------------------------------------------------------
def _linear_world(T=3, h=4, w=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    cond = {"concat": rnd(T, 4, h, w), "crossattn": rnd(T, 1, 8), "vector": rnd(T, 8)}
    uc = {"concat": torch.zeros(T, 4, h, w), "crossattn": rnd(T, 1, 8), "vector": rnd(T, 8)}
    mix = rnd(4, 4) * 0.3

    def denoise(x, sigma, c, cond_mask):   # linear in x, with a sigma-dependent gain and a conditioning term
        gain = (1.0 / (1.0 + sigma ** 2)).reshape(-1, 1, 1, 1)
        return torch.einsum("oc,nchw->nohw", mix, x) * gain + 0.1 * c["concat"] + c["vector"].mean(1).reshape(-1, 1, 1, 1)
    mask = torch.zeros(T)
    mask[0] = 1
    return denoise, rnd(T, 4, h, w), cond, uc, rnd(T, 4, h, w), mask


@pytest.mark.parametrize("guider", ["cfg", "identity"])
@pytest.mark.parametrize("steps", [1, 3, 7])
def test_scaffolding_with_the_euler_update_is_the_oracles_sampler_bit_for_bit(steps, guider):
    from oracle import vista_oracle as O
    denoise, x, cond, uc, cond_frame, mask = _linear_world()
    for m in (mask, torch.zeros_like(mask)):
        want = O.euler_edm_sample(denoise, x, cond, uc, cond_frame, m, steps, scale=2.5, guider=guider)
        got = R.sample_with(denoise, "euler", x, cond, uc, cond_frame, m, steps, scale=2.5, guider=guider)
        assert torch.equal(got, want)
    per_frame = O.triangle_guider_scale(3)
    assert torch.equal(R.sample_with(denoise, "euler", x, cond, uc, cond_frame, mask, steps, scale=per_frame),
                       O.euler_edm_sample(denoise, x, cond, uc, cond_frame, mask, steps, scale=per_frame))
    two = R.sample_with(denoise, "2m", x, cond, uc, cond_frame, mask, steps, guider=guider)
    assert torch.isfinite(two).all() and torch.equal(two[0], cond_frame[0])


# ---- 2. coefficients ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 10, 50])
def test_coefficients_equal_the_float64_restatement(n):
    from vista_amd import sample_utils as SU
    from vista_amd.modules.diffusionmodules import sampling
    sig = SU.init_sampling(sampler="DPMPP2MSampler", steps=n).host_sigmas()   # the shipped schedule, as the sampler holds it
    got, want = sampling.dpmpp2m_coefficients(sig), R.coefficients_f64(sig)
    assert len(got) == len(want) == n
    for (a, b, c), ref in zip(got, want):
        for v, r in zip((a, b, c), ref):
            assert isinstance(v, float) and abs(v - r) <= 1e-12 * abs(r), (n, v, r)
    assert got[-1] == (0.0, 1.0, 0.0) and got[0][2] == 0.0
    s = [float(v) for v in sig]
    h_prev = None
    for i, (a, b, c) in enumerate(got[:-1]):
        h = math.log(s[i] / s[i + 1])
        e = -math.expm1(-h)
        assert abs(e - (1.0 - a)) <= 1e-12 and abs(a - s[i + 1] / s[i]) <= 1e-12 * a
        assert abs((b + c) - e) <= 1e-12 * e, "b + c = e: a constant denoiser is integrated exactly"
        if h_prev is not None:
            r = h_prev / h
            assert abs(c + e / (2 * r)) <= 1e-12 * abs(c) and c < 0.0
        h_prev = h
    # the coefficients, applied as the kernels apply them, are the recurrence of the yardstick
    den = R.gaussian_denoiser(1.0)
    sig64 = [float(v) for v in sig]
    x = x0 = math.sqrt(1.0 + sig64[0] ** 2)
    old = 0.0
    for i, (a, b, c) in enumerate(got):
        d = den(x, sig64[i])
        x, old = a * x + b * d + c * old, d
    want_x = float(R.sample_f64(den, [x0], sig64, "2m")[0])
    assert abs(x - want_x) <= 1e-12 * abs(want_x)


# ---- 3. order ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
def test_second_order_on_the_analytic_denoiser(s):
    euler = {n: R.order_error("euler", n, s) for n in (10, 20, 30, 50, 100)}
    two = {n: R.order_error("2m", n, s) for n in (10, 20, 30, 50, 100)}
    print(f"ORDER s={s}: euler {euler}  2m {two}")
    for n in (10, 20, 30, 50):
        assert two[n] < euler[n], n
    assert two[30] < euler[50]
    assert 3.5 <= two[50] / two[100] <= 5.5
    assert 1.8 <= euler[50] / euler[100] <= 2.2


# ---- 4. the factory and the hook ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guider", ["IdentityGuider", "VanillaCFG", "LinearPredictionGuider", "TrianglePredictionGuider"])
def test_get_sampler_builds_the_class_with_the_same_dicts(guider):
    import inspect
    from vista_amd import sample_utils as SU
    from vista_amd.modules.diffusionmodules import discretizer, guiders, sampling
    s = SU.get_sampler("DPMPP2MSampler", 9, SU.get_discretization("EDMDiscretization"), SU.get_guider(guider, 3.0, 7))
    assert type(s) is sampling.DPMPP2MSampler and type(s.discretization) is discretizer.EDMDiscretization and type(s.guider) is getattr(guiders, guider)
    assert (s.discretization.sigma_min, s.discretization.sigma_max, s.discretization.rho) == (0.002, 700.0, 7.0)
    assert s.num_steps == 9 and s.verbose is False and s.graph is None and s.cfg_streams is None and not hasattr(s, "s_churn")
    assert type(SU.init_sampling(sampler="DPMPP2MSampler", guider=guider)) is sampling.DPMPP2MSampler
    euler = SU.init_sampling(guider=guider, steps=9, cfg_scale=3.0, num_frames=7)
    assert torch.equal(s.host_sigmas(), euler.host_sigmas())
    assert list(inspect.signature(sampling.DPMPP2MSampler.__init__).parameters)[1:] == ["discretization_config", "num_steps", "guider_config", "verbose",
                                                                                      "device"]
    with pytest.raises(ValueError, match="^Unknown sampler HeunEDMSampler$"):
        SU.get_sampler("HeunEDMSampler", 9, SU.get_discretization("EDMDiscretization"), SU.get_guider(guider, 3.0, 7))


def test_the_environment_hook_selects_the_sampler_and_a_bad_value_is_refused_by_name(monkeypatch):
    import inspect
    from vista_amd import drive, plan, reward, sample
    from vista_amd import sample_utils as SU
    monkeypatch.delenv("VISTA_SAMPLER", raising=False)
    assert SU.sampler_name() == "EulerEDMSampler" and SU.sampler_name("DPMPP2MSampler") == "DPMPP2MSampler"
    monkeypatch.setenv("VISTA_SAMPLER", "")
    assert SU.sampler_name() == "EulerEDMSampler"
    monkeypatch.setenv("VISTA_SAMPLER", "DPMPP2MSampler")
    assert SU.sampler_name() == "DPMPP2MSampler" and SU.sampler_name("EulerEDMSampler") == "EulerEDMSampler", "an argument wins over the hook"
    monkeypatch.setenv("VISTA_SAMPLER", "HeunEDMSampler")
    with pytest.raises(ValueError, match="Unknown sampler HeunEDMSampler.*VISTA_SAMPLER"):
        SU.sampler_name()
    with pytest.raises(ValueError, match="Unknown sampler Nope"):
        SU.sampler_name("Nope")
    # every CLI that samples refuses the bad hook before a model is built (a model needs a GPU and a checkpoint: neither is here)
    small = ["--height", "128", "--width", "256", "--n_frames", "5"]
    for module, argv in ((sample, small), (reward, small)):
        with pytest.raises(ValueError, match="Unknown sampler HeunEDMSampler"):
            module.main(argv)
    for fn in (sample.run, reward.run, drive.DriveSession.__init__, plan.Planner.__init__):
        assert inspect.signature(fn).parameters["sampler"].default is None, fn


# ---- 5. the sweep's host side ------------------------------------------------------------------------------------------------------------------
def test_sweep_parser_is_samples_plus_five():
    from vista_amd import sample, step_sweep
    base = {a.dest: a for a in sample.parse_args()._actions}
    mine = {a.dest: a for a in step_sweep.parse_args()._actions}
    for dest, a in base.items():
        b = mine.pop(dest)
        assert (b.option_strings, b.default, b.type, b.nargs, b.const) == (a.option_strings, a.default, a.type, a.nargs, a.const), dest
    assert {k: (v.default, v.type) for k, v in mine.items()} == {
        "n_scenes": (0, int), "samplers": ("EulerEDMSampler,DPMPP2MSampler", str), "budgets": ("10,15,20,30,50", str), "ref_steps": (200, int),
        "ref_sampler": ("DPMPP2MSampler", str)}
    assert step_sweep.parse_samplers("EulerEDMSampler, DPMPP2MSampler") == list(SAMPLERS)
    assert step_sweep.parse_budgets("10,15,20,30,50", 200) == [10, 15, 20, 30, 50] and step_sweep.parse_budgets("4, 2,4", 4) == [4, 2]


@pytest.mark.parametrize("argv,match", [
    (["--height", "100"], "--height 100"),                                   # what check_sizes refuses
    (["--n_frames", "40"], "--n_frames 40"),
    (["--samplers", "EulerEDMSampler,HeunEDMSampler"], "Unknown sampler HeunEDMSampler"),
    (["--ref_sampler", "HeunEDMSampler"], "--ref_sampler: Unknown sampler HeunEDMSampler"),
    (["--samplers", ","], "--samplers.*empty"),
    (["--budgets", ""], "--budgets.*empty"),
    (["--budgets", "10,0"], "--budgets.*budget of 0"),
    (["--budgets", "10,-3"], "--budgets.*budget of -3"),
    (["--budgets", "10,x"], "--budgets.*'x'"),
    (["--budgets", "10,201"], "--budgets.*201.*--ref_steps 200"),
    (["--budgets", "10,30", "--ref_steps", "20"], "--budgets.*30.*--ref_steps 20"),
    (["--n_rounds", "2"], "--n_rounds 2"),
    (["--n_scenes", "0"], "--n_scenes 0.*random walk"),
    (["--n_scenes", "-1", "--rand_gen"], "--n_scenes -1"),
])
def test_sweep_refusals_name_the_flag_before_a_model_is_built(argv, match, monkeypatch):
    from vista_amd import step_sweep
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(step_sweep.SU, "init_model", lambda *a, **k: pytest.fail("a refused run must not build a model"))
    with pytest.raises(ValueError, match=match):
        step_sweep.main(["--n_scenes", "1"] + argv)


def test_sweep_refuses_several_ranks_and_allows_the_img_dataset(monkeypatch):
    from vista_amd import step_sweep
    built = []
    monkeypatch.setattr(step_sweep.SU, "init_model", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(KeyboardInterrupt()))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE 2"):
        step_sweep.main(["--n_scenes", "1"])
    assert not built
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(KeyboardInterrupt):   # every check passed: the next thing main does is build the model
        step_sweep.main(["--n_scenes", "1", "--dataset", "IMG"])
    assert len(built) == 1


def _record(index, cond, runs):
    return {"index": index, "cond": cond, "ref_gap": 0.01 * (index + 1), "ref_sampler": "DPMPP2MSampler", "ref_steps": 8,
            "runs": [{"sampler": s, "steps": n, "frame_err": fe, "latent_err": None, "mean_psnr": p, "mean_ssim": 0.5, "seconds": 1.0}
                     for s, n, fe, p in runs]}


def test_summarise_gives_the_equal_error_table():
    from vista_amd import step_sweep
    E, D = SAMPLERS
    # frame 0 is a conditioning frame (error 0, left out of every mean: with it the means would be a third smaller)
    recs = [_record(0, [0], [(E, 2, [0.0, 0.9, 0.7], 20.0), (E, 4, [0.0, 0.5, 0.3], 24.0), (D, 2, [0.0, 0.4, 0.4], 25.0), (D, 4, [0.0, 0.1, 0.1], None)]),
            _record(1, [0], [(E, 2, [0.0, 0.7, 0.9], 22.0), (E, 4, [0.0, 0.3, 0.5], 26.0), (D, 2, [0.0, 0.4, 0.4], 27.0), (D, 4, [0.0, 0.1, 0.1], 30.0)])]
    out = step_sweep.summarise(recs)
    assert out["scenes"] == 2 and abs(out["ref_gap"] - 0.015) < 1e-15 and (out["ref_sampler"], out["ref_steps"]) == ("DPMPP2MSampler", 8)
    runs = {(r["sampler"], r["steps"]): r for r in out["runs"]}
    want = {(E, 2): 0.8, (E, 4): 0.4, (D, 2): 0.4, (D, 4): 0.1}
    for k, v in want.items():
        assert abs(runs[k]["latent_err"] - v) < 1e-15 and runs[k]["scenes"] == 2, k
    assert runs[(E, 2)]["mean_psnr"] == 21.0 and runs[(D, 4)]["mean_psnr"] is None, "a null in a mean makes the mean null"
    table = {(r["sampler"], r["steps"]): r["matched_by"] for r in out["equal_error"]}
    assert table == {(E, 2): {D: 2},      # 2M at 2 steps is already below Euler at 2
                     (E, 4): {D: 2},      # a tie (0.4 vs 0.4) counts: not larger
                     (D, 2): {E: 4},      # the tie, seen from the other side
                     (D, 4): {E: None}}   # no Euler budget swept reaches 0.1
    assert step_sweep.clip_error([0.0, 0.5, 0.3], [0]) == 0.4 and step_sweep.summarise([])["scenes"] == 0
    assert step_sweep.summarise(recs) == out, "a pure function"


# ---- 6. the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_table_and_abi_version():
    import ctypes
    from vista_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(vk_\w+)\s*\(", hdr, flags=re.M))
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert {"vk_sampler_update_2m", "vk_dpmpp2m_step"} <= declared
    assert _lib.SIGNATURES["vk_sampler_update_2m"] == [vp] * 4 + [i32] * 3 + [f32] * 5 + [i32, vp]
    assert _lib.SIGNATURES["vk_dpmpp2m_step"] == [vp] * 4 + [f32] * 3 + [i64, vp]
    assert _lib.ABI_VERSION == 9
    for name in ("libvista_hip.so", "libvista_hip_f16.so"):   # storage-type independent: both libraries link them
        path = os.path.join(ROOT, "vista_amd", "lib", name)
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            assert hasattr(lib, "vk_sampler_update_2m") and hasattr(lib, "vk_dpmpp2m_step") and lib.vk_abi_version() == 9, name
