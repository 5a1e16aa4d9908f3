"""Host side of the denoising-loss front door (vista_amd/denoise_loss.py and the loss classes under vista_amd/modules/diffusionmodules): the
classes' API against the reference's recorded signatures, the weightings and sigma samplers against the golden, the float64 restatement
tests/_loss_ref.py against the reference's own fp32 results -- with the proof that its bound bites --, and the CLI: flags, refusals, the sigma
grid, the record and summary formats. No GPU. The golden files are written by tools/make_golden_diffusion_loss.py from the real reference."""
import inspect
import json
import math
import os

import pytest
import torch

from tests import _loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLD, "diffusion_loss_tiny.pt"))


# ---- the classes --------------------------------------------------------------------------------------------------------------------------------
def test_class_names_kwargs_and_defaults_are_the_references():
    from vista_amd.util import get_obj_from_str
    with open(os.path.join(GOLD, "loss_api.json")) as f:
        api = json.load(f)
    assert sorted(api) == ["DiscreteSampling", "EDMSampling", "EDMWeighting", "EpsWeighting", "StandardDiffusionLoss", "UnitWeighting", "VWeighting"]
    for name, entry in api.items():
        cls = get_obj_from_str(entry["target"])   # the reference's target string resolves to this package's class
        assert cls.__name__ == name and cls.__module__.startswith("vista_amd.modules.diffusionmodules.")
        params = [p for p in list(inspect.signature(cls.__init__).parameters.values())[1:] if p.kind not in (p.VAR_POSITIONAL, p.VAR_KEYWORD)]
        mine = [{"name": p.name, "default": None if p.default is p.empty else repr(p.default), "required": p.default is p.empty} for p in params]
        assert mine == entry["params"], name
    from vista_amd.modules.diffusionmodules.loss import StandardDiffusionLoss
    for method in ("get_noised_input", "forward", "_forward", "get_loss"):
        assert callable(getattr(StandardDiffusionLoss, method))
    assert list(inspect.signature(StandardDiffusionLoss.forward).parameters)[1:] == ["network", "denoiser", "conditioner", "input", "batch"]
    assert list(inspect.signature(StandardDiffusionLoss._forward).parameters)[1:5] == ["network", "denoiser", "cond", "input"]
    hooks = {k: p for k, p in inspect.signature(StandardDiffusionLoss._forward).parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert {"sigmas", "cond_mask", "noise", "offset"} <= set(hooks) and all(p.default is None for k, p in hooks.items() if k != "return_sums")
    doc = inspect.getdoc(inspect.getmodule(StandardDiffusionLoss))
    assert "torch.no_grad()" in doc and "NOT built" in doc


def test_the_references_loss_fn_config_instantiates_unmodified():
    import yaml
    from vista_amd.modules.diffusionmodules import loss, loss_weighting, sigma_sampling
    from vista_amd.util import instantiate_from_config
    with open(os.path.join(GOLD, "loss_fn_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["target"] == "vwm.modules.diffusionmodules.loss.StandardDiffusionLoss"
    fn = instantiate_from_config(cfg)
    assert isinstance(fn, loss.StandardDiffusionLoss) and isinstance(fn.sigma_sampler, sigma_sampling.EDMSampling)
    assert isinstance(fn.loss_weighting, loss_weighting.VWeighting) and fn.loss_weighting.sigma_data == 1.0
    assert (fn.loss_type, fn.use_additional_loss, fn.offset_noise_level, fn.additional_loss_weight) == ("l2", True, 0.02, 0.1)
    assert (fn.num_frames, fn.replace_cond_frames, fn.cond_frames_choices) == (25, True, [[], [0], [0, 1], [0, 1, 2]])
    assert (fn.sigma_sampler.p_mean, fn.sigma_sampler.p_std, fn.sigma_sampler.num_frames) == (1.0, 1.6, 25)


def test_weightings_and_samplers_equal_the_golden(golden):
    from vista_amd.modules.diffusionmodules import loss_weighting as lw, sigma_sampling as ss
    w = golden["weightings"]
    for key, obj in (("Unit", lw.UnitWeighting()), ("EDM", lw.EDMWeighting()), ("EDM_0.7", lw.EDMWeighting(sigma_data=0.7)), ("V", lw.VWeighting()),
                     ("Eps", lw.EpsWeighting())):
        assert torch.equal(obj(w["sigma"]), w[key]), key
        name = key.split("_")[0]
        assert R.rel(R.weighting(name, w["sigma"], 0.7 if key == "EDM_0.7" else 0.5), w[key]) < 1e-6, key
    s = golden["samplers"]
    assert torch.equal(ss.EDMSampling()(6, rand=s["rand"]), s["EDM_default"])
    assert torch.equal(ss.EDMSampling(p_mean=1.0, p_std=1.6)(6, rand=s["rand"]), s["EDM_phase2"])
    torch.manual_seed(11)   # the draw comes from torch's CPU generator, one value per clip
    drawn = ss.EDMSampling(p_mean=1.0, p_std=1.6, num_frames=3)(6)
    assert torch.equal(drawn, s["EDM_seed11_frames3"]) and torch.equal(drawn[:3], drawn[:1].expand(3)) and drawn[0] != drawn[3]
    disc = s["discretization_config"]
    assert torch.equal(ss.DiscreteSampling(disc, 10)(6, rand=s["idx"]), s["Discrete"])
    assert torch.equal(ss.DiscreteSampling(disc, 10).sigmas, s["Discrete_table"])
    assert torch.equal(ss.DiscreteSampling(disc, 10, do_append_zero=True, flip=False).sigmas, s["Discrete_noflip_zero"])
    torch.manual_seed(3)
    picked = ss.DiscreteSampling(disc, 10, num_frames=2)(4)
    assert picked.shape == (4,) and picked[0] == picked[1] and picked[2] == picked[3] and all(v in s["Discrete_table"] for v in picked)


def test_cond_mask_draw_picks_what_the_reference_picked(golden):
    """The tool seeds Python's generator with 101 + i before configuration i; the reference's first use of it is the mask draw."""
    import random
    from vista_amd.modules.diffusionmodules.loss import StandardDiffusionLoss
    P = "vwm.modules.diffusionmodules."
    drawn = 0
    for i, case in enumerate(golden["cases"]):
        if not case["replace_cond_frames"]:
            continue
        fn = StandardDiffusionLoss({"target": P + "sigma_sampling.EDMSampling", "params": {"num_frames": case["num_frames"]}},
                                   {"target": P + "loss_weighting.VWeighting"}, num_frames=case["num_frames"], replace_cond_frames=True,
                                   cond_frames_choices=case["cond_frames_choices"])
        random.seed(101 + i)
        assert torch.equal(fn.draw_cond_mask(case["input"].shape[0]), case["cond_mask"]), i
        drawn += int(case["cond_mask"].sum())
    assert drawn > 0
    with pytest.raises(ValueError, match="shorter than a clip"):
        StandardDiffusionLoss({"target": P + "sigma_sampling.EDMSampling"}, {"target": P + "loss_weighting.VWeighting"}, num_frames=2,
                              replace_cond_frames=True, cond_frames_choices=[[], [0, 1]]).draw_cond_mask(2)
    with pytest.raises(ValueError, match="'l2' or 'l1'"):
        StandardDiffusionLoss({"target": P + "sigma_sampling.EDMSampling"}, {"target": P + "loss_weighting.VWeighting"}, loss_type="huber")


def test_keep_mask_is_the_references_disc_with_its_ties_and_its_asymmetry():
    from vista_amd.modules.diffusionmodules.util import fourier_keep_mask
    for Hh, Ww in ((8, 8), (8, 16), (5, 7), (1, 1), (1, 12), (72, 128)):
        keep = fourier_keep_mask(Hh, Ww)
        assert keep.dtype == torch.uint8 and keep.shape == (Hh, Ww)
        assert torch.equal(keep.bool(), ~torch.fft.ifftshift(R.disc_mask(Hh, Ww))), (Hh, Ww)
    k8 = fourier_keep_mask(8, 8)
    assert [int(k8[a, b]) for a in (2, -2) for b in (2, -2)] == [0, 0, 0, 0], "the four ties (+-2, +-2) lie inside the disc (<=)"
    assert int(k8[3, 0]) == 1 and int(k8[2, 1]) == 0
    k57 = fourier_keep_mask(5, 7).bool()
    assert not torch.equal(k57, torch.roll(k57.flip(0, 1), (1, 1), (0, 1))), "an odd plane's mask is not symmetric, and is left so"
    assert int((fourier_keep_mask(72, 128) == 0).sum()) == 3617
    assert fourier_keep_mask(8, 8) is fourier_keep_mask(8, 8), "cached per (H, W, d_s)"


# ---- the float64 restatement against the reference ------------------------------------------------------------------------------------------------
def _case_loss(case, defect=None):
    m = case["cond_mask"] if case["replace_cond_frames"] else None
    return R.loss(case["model_output"], case["input"], R.weighting("V", case["sigmas"]), case["num_frames"], m, case["loss_type"],
                  case["use_additional_loss"], case["additional_loss_weight"], defect=defect)


def test_restatement_equals_the_reference_within_rounding(golden):
    """The reference computes in fp32; the distance is its rounding. The recorded figure (R.REFERENCE_LOSS_REL, profiles/diffusion_loss_parity.txt)
    is the largest over the configurations; the bound is 8 x it."""
    assert R.REFERENCE_LOSS_REL < 1e-5, "a larger figure would be a fault of the restatement, not rounding"
    worst = 0.0
    for i, case in enumerate(golden["cases"]):
        m = case["cond_mask"] if case["replace_cond_frames"] else None
        noised = R.noised_input_f32(case["input"], case["noise"], case["sigmas"], m, case["offset"], case["offset_noise_level"])
        assert torch.equal(noised, case["noised"]), (i, "the noising is one fp32 expression: bit for bit")
        r = R.rel(_case_loss(case), case["loss"])
        worst = max(worst, r)
        print(f"LOSSREF case {i} {case['loss_type']} additional={case['use_additional_loss']} replace={case['replace_cond_frames']} "
              f"T={case['num_frames']} {tuple(case['input'].shape)}: reference vs float64 {r:.3e}")
        assert r <= R.LOSS_BOUND, (i, r)
        if case["use_additional_loss"]:
            predict = R.blend(case["model_output"], case["input"], m).float()
            for key, x in (("predict_hf", predict), ("target_hf", case["input"])):
                err = R.filter_error(case[key], R.fourier_filter(x, 0.0), x).max().item()
                assert err < 2e-6, (i, key, err)   # fp32 FFT of at most 128 points: a few ulps of the plane's scale
    print(f"LOSSREF worst {worst:.3e}, recorded {R.REFERENCE_LOSS_REL:.3e}, bound {R.LOSS_BOUND:.3e}")
    assert worst <= R.REFERENCE_LOSS_REL * 1.01, "the recorded figure is the measured one"
    for f in golden["fourier_filter"]:
        assert R.filter_error(f["y"], R.fourier_filter(f["x"], f["scale"]), f["x"]).max().item() < 2e-6


APPLIES = {   # defect -> the configurations on which it changes the result
    "pair_shift": lambda c: c["use_additional_loss"] and c["num_frames"] > 2,
    "norm_axis": lambda c: c["use_additional_loss"] and c["num_frames"] > 1,
    "no_blend": lambda c: c["replace_cond_frames"] and c["num_frames"] > 1,
    "aux_t0": lambda c: c["use_additional_loss"] and c["num_frames"] > 1 and not c["replace_cond_frames"],
    "tie_flip": lambda c: c["use_additional_loss"] and tuple(c["input"].shape[-2:]) == (8, 8),
    "mask_sym": lambda c: c["use_additional_loss"] and tuple(c["input"].shape[-2:]) == (5, 7),
    "w_frame": lambda c: c["use_additional_loss"] and c["num_frames"] > 1 and not c["replace_cond_frames"],
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_bound_bites(defect, golden):
    """Each defect, applied to the restatement, lands outside the bound on every configuration it concerns."""
    assert sorted(APPLIES) == sorted(R.DEFECTS)
    hit = [c for c in golden["cases"] if APPLIES[defect](c)]
    assert len(hit) >= 2, "both loss types"
    for case in hit:
        r = R.rel(_case_loss(case, defect), case["loss"])
        print(f"LOSSBITES {defect} {case['loss_type']} {tuple(case['input'].shape)}: {r:.3e} against the bound {R.LOSS_BOUND:.3e}")
        assert r > R.LOSS_BOUND, (defect, r)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_are_the_sampling_flags_plus_the_loss_flags():
    from vista_amd import denoise_loss, sample
    base = {a.dest: a for a in sample.parse_args()._actions if a.dest != "help"}
    mine = {a.dest: a for a in denoise_loss.parse_args()._actions if a.dest != "help"}
    assert not set(base) - set(mine)
    for name, a in base.items():
        b = mine[name]
        assert (b.option_strings, b.default, b.type, b.nargs, b.const) == (a.option_strings, a.default, a.type, a.nargs, a.const), name
    added = {k: (mine[k].default, mine[k].type) for k in set(mine) - set(base)}
    assert added == {"n_scenes": (0, int), "n_sigmas": (8, int), "p_mean": (1.0, float), "p_std": (1.6, float), "loss_type": ("l2", str),
                     "weighting": ("V", str), "no_additional_loss": (False, None), "additional_loss_weight": (0.1, float),
                     "offset_noise_level": (0.0, float), "noise_seed": (0, int)}
    assert mine["weighting"].choices == ["V", "EDM", "Eps", "Unit"] and mine["loss_type"].choices == ["l2", "l1"]


@pytest.mark.parametrize("flags,env,match", [
    (["--rand_gen"], {"WORLD_SIZE": "2"}, "WORLD_SIZE 2"),
    ([], {}, "--n_scenes 0"),
    (["--n_scenes", "-1"], {}, "--n_scenes -1"),
    (["--rand_gen", "--height", "100"], {}, "--height 100"),
    (["--rand_gen", "--n_frames", "33"], {}, "--n_frames 33"),
    (["--rand_gen", "--n_conds", "0"], {}, "--n_conds 0"),
    (["--rand_gen", "--n_sigmas", "0"], {}, "--n_sigmas 0"),
    (["--rand_gen", "--n_conds", "25"], {}, "--n_conds 25"),
    (["--rand_gen", "--n_frames", "5", "--n_conds", "5"], {}, "nothing is left to score"),
    (["--rand_gen", "--height", "640"], {}, "80 x 128 plane does not fit"),
], ids=["world_size", "random_walk_without_a_count", "negative_count", "height", "window", "n_conds_zero", "n_sigmas", "all_frames_cond",
        "all_of_five_cond", "oversize_plane"])
def test_what_cannot_run_is_refused_before_a_model_is_built(flags, env, match, monkeypatch, tmp_path):
    from vista_amd import denoise_loss
    from vista_amd import sample_utils as SU

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(SU, "init_model", no_model)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(ValueError, match=match):
        denoise_loss.main(flags + ["--save", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists(), "a refused run writes nothing"


def test_what_is_allowed_reaches_the_model(monkeypatch, tmp_path):
    """The IMG dataset, the oversize plane without the additional terms, a counted random walk: each gets as far as building the model."""
    from vista_amd import denoise_loss
    from vista_amd import sample_utils as SU

    class Built(Exception):
        pass

    def built(*a, **k):
        raise Built()
    monkeypatch.setattr(SU, "init_model", built)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for flags in (["--rand_gen", "--dataset", "IMG"], ["--rand_gen", "--height", "640", "--no_additional_loss"], ["--n_scenes", "3"],
                  ["--rand_gen", "--n_sigmas", "1"]):
        with pytest.raises(Built):
            denoise_loss.main(flags + ["--save", str(tmp_path / "out")])


def test_sigma_grid_values():
    from statistics import NormalDist
    from vista_amd import denoise_loss
    grid = denoise_loss.sigma_grid(8)
    assert grid == R.sigma_grid(8, 1.0, 1.6) and grid == sorted(grid) and len(grid) == 8
    for i, s in enumerate(grid):   # sigma_i is the (i + 0.5) / n quantile of the log-normal
        assert abs(NormalDist(1.0, 1.6).cdf(math.log(s)) - (i + 0.5) / 8) < 1e-12
    assert all(abs(math.log(a) + math.log(b) - 2.0) < 1e-12 for a, b in zip(grid, reversed(grid))), "symmetric about p_mean in log sigma"
    assert denoise_loss.sigma_grid(1) == [math.e] and denoise_loss.sigma_grid(1, p_mean=0.0, p_std=5.0) == [1.0]
    assert abs(denoise_loss.sigma_grid(2)[0] - math.exp(1.0 + 1.6 * NormalDist().inv_cdf(0.25))) < 1e-15
    with pytest.raises(ValueError, match="--n_sigmas 0"):
        denoise_loss.sigma_grid(0)


def _fake_report(denoise_loss, scale, n_sigmas=2, T=3):
    sig = denoise_loss.sigma_grid(n_sigmas)
    return denoise_loss.LossReport(sig, [scale * (i + 1) for i in range(n_sigmas)], [0.5 * scale] * n_sigmas, [0.6 * scale] * n_sigmas,
                                   [0.25 * scale] * n_sigmas, [[0.0] + [scale * t for t in range(1, T)] for _ in range(n_sigmas)], [0])


@pytest.mark.parametrize("n_sigmas", [2, 1])
def test_record_and_summary_formats(tmp_path, n_sigmas):
    from vista_amd import denoise_loss, frontdoor
    opt = denoise_loss.parse_args().parse_args(["--rand_gen", "--n_sigmas", str(n_sigmas), "--n_frames", "3"])
    save = str(tmp_path / "out")
    path = frontdoor.start_records(save, denoise_loss.RECORDS_NAME)
    records = []
    for index, scale in ((0, 1.0), (4, 3.0)):
        rec = denoise_loss.make_record(index, [f"scene{index}/a.png", "b.png", "c.png"], _fake_report(denoise_loss, scale, n_sigmas), opt,
                                       {"load": 0.12345678, "forward": 1.0})
        assert frontdoor.append_record(save, denoise_loss.RECORDS_NAME, rec) == path
        records.append(rec)
    with open(path) as f:
        lines = [json.loads(line) for line in f]
    assert lines == records and [r["index"] for r in lines] == [0, 4]
    r = lines[1]
    assert sorted(r) == sorted(["index", "frames", "seed", "noise_seed", "settings", "sigmas", "loss", "mse", "dynamics", "structure", "frame_mse",
                                "cond", "timings"])
    assert r["frames"] == ["scene4/a.png"] and r["seed"] == 23 and r["noise_seed"] == 0 and r["cond"] == [0]
    assert r["sigmas"] == denoise_loss.sigma_grid(n_sigmas) and len(r["loss"]) == n_sigmas and len(r["frame_mse"]) == n_sigmas
    assert all(len(row) == 3 for row in r["frame_mse"]) and r["timings"] == {"load": 0.1235, "forward": 1.0}
    assert r["settings"]["weighting"] == "V" and r["settings"]["additional_loss"] is True and r["settings"]["n_sigmas"] == n_sigmas
    summary_path = frontdoor.write_summary(save, denoise_loss.SUMMARY_NAME, denoise_loss.summarize(records))
    with open(summary_path) as f:
        summary = json.load(f)
    assert os.path.basename(summary_path) == "loss_summary.json" and summary["scenes"] == 2 and summary["sigmas"] == r["sigmas"]
    assert summary["loss"] == [2.0 * (i + 1) for i in range(n_sigmas)] and summary["mse"] == [1.0] * n_sigmas
    assert summary["frame_mse"] == [[0.0, 2.0, 4.0]] * n_sigmas and summary["cond"] == [0]
    frontdoor.start_records(save, denoise_loss.RECORDS_NAME)
    assert open(path).read() == "", "the file describes one run"
    bad = _fake_report(denoise_loss, float("nan"), n_sigmas)
    with pytest.raises(ValueError):
        frontdoor.append_record(save, denoise_loss.RECORDS_NAME, denoise_loss.make_record(0, ["a"], bad, opt))


def test_library_exports_the_loss_entry_points_and_the_plane_rule():
    from vista_amd import _lib, build, ops
    assert "loss.hip" in build.SOURCES
    lib = _lib.load()
    for name in ("vk_loss_noise_input", "vk_fourier_highpass", "vk_fourier_highpass_lds_bytes", "vk_loss_stats"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    assert "#define VK_LOSS_STATS_BLOCKS 16" in hdr and ops.LOSS_STATS_BLOCKS == 16 and "#define VK_LOSS_MAX_CHANNELS 64" in hdr
    for Hh, Ww in ((72, 128), (1, 1), (5, 7), (80, 128), (72, 144), (0, 4), (4, -1)):
        fits = ops.fourier_highpass_fits(Hh, Ww)
        assert (lib.vk_fourier_highpass_lds_bytes(Hh, Ww) > 0) == fits, (Hh, Ww)
    assert lib.vk_fourier_highpass_lds_bytes(72, 128) == 150656 and "takes 150656" in hdr
    with pytest.raises(_lib.VistaHipError, match="no CPU fallback"):
        ops.loss_noise_input(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2), torch.ones(1))
