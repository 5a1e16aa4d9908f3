"""Writes the goldens of the denoising-loss front door by running the REAL reference classes on the CPU (oracle/ref_shim.install()):

  tests/golden/diffusion_loss_tiny.pt   per configuration: the inputs, the draws the reference made, the stub denoiser's output, the reference's
                                        noised input, fourier_filter outputs and losses; the weightings and both sigma samplers on fixed `rand`
  tests/golden/loss_api.json            names, constructor kwargs and defaults of the reference's classes (read from their signatures)
  tests/golden/loss_fn_config.yaml      the loss_fn_config block of the reference's phase 2 training config (settings only, anchors resolved)

Needs the reference tree (VISTA_REFERENCE); nothing of its program text is copied. kornia / open_clip are empty stand-ins, as in
oracle/make_golden_cond.py: the reference's loss.py imports the conditioner module for an annotation only. fourier_filter builds its mask with
.cuda(): that call is a no-op in this process.

    python tools/make_golden_diffusion_loss.py
"""
import contextlib
import inspect
import io
import itertools
import json
import os
import random
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CHOICES = [[], [0], [0, 1], [0, 1, 2]]


def reference_modules():
    ref_shim.install()
    for name in ("kornia", "open_clip"):
        sys.modules.setdefault(name, types.ModuleType(name))
    torch.Tensor.cuda = lambda self, *a, **k: self   # this process has no GPU; the reference's mask is built with .cuda()
    with contextlib.redirect_stdout(io.StringIO()):
        from vwm.modules.diffusionmodules import loss, loss_weighting, sigma_sampling, util
    return loss, loss_weighting, sigma_sampling, util


class Recorder:
    """Wraps torch.randn / torch.randn_like for the duration and keeps what they returned, in call order."""

    def __enter__(self):
        self.calls, self.saved = [], (torch.randn, torch.randn_like)

        def randn(*a, **k):
            out = self.saved[0](*a, **k)
            self.calls.append(("randn", out.clone()))
            return out

        def randn_like(*a, **k):
            out = self.saved[1](*a, **k)
            self.calls.append(("randn_like", out.clone()))
            return out

        torch.randn, torch.randn_like = randn, randn_like
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self.saved
        return False


def stub_denoiser(seen):
    """Stands in for denoiser(network, noised, sigmas, cond, cond_mask): a smooth function of its input whose frame-to-frame changes differ
    from the target's, recorded with what it was handed."""
    def denoiser(network, noised_input, sigmas, cond, cond_mask):
        c_skip = 1.0 / (sigmas ** 2 + 1.0)
        out = noised_input * c_skip[:, None, None, None] + 0.1 * torch.tanh(torch.roll(noised_input, 1, dims=-1))
        seen.update(noised=noised_input.clone(), sigmas=sigmas.clone(), cond_mask=cond_mask.clone(), out=out.clone())
        return out
    return denoiser


def one_case(loss_mod, loss_type, additional, replace, T, H, W, seed):
    B, C = (2 if additional else 1), 4   # (without the additional terms nothing couples the frames of a clip: one clip is enough)
    n = B * T
    fn = loss_mod.StandardDiffusionLoss(
        sigma_sampler_config={"target": "vwm.modules.diffusionmodules.sigma_sampling.EDMSampling",
                              "params": {"p_mean": 1.0, "p_std": 1.6, "num_frames": T}},
        loss_weighting_config={"target": "vwm.modules.diffusionmodules.loss_weighting.VWeighting"},
        loss_type=loss_type, use_additional_loss=additional, offset_noise_level=0.02, additional_loss_weight=0.1, num_frames=T,
        replace_cond_frames=replace, cond_frames_choices=[c for c in CHOICES if len(c) < T])
    torch.manual_seed(seed)
    random.seed(seed)
    smooth = torch.randn(B, 1, C, H, W).expand(B, T, C, H, W) + 0.3 * torch.randn(B, T, C, H, W).cumsum(1)   # a clip that moves a little
    x = smooth.reshape(n, C, H, W).contiguous()
    seen, hf = {}, []
    real_filter = loss_mod.fourier_filter

    def recording_filter(t, scale, *a, **k):
        out = real_filter(t, scale, *a, **k)
        hf.append(out.clone())
        return out

    loss_mod.fourier_filter = recording_filter
    try:
        with Recorder() as rec, torch.no_grad():
            got = fn._forward(None, stub_denoiser(seen), {}, x)
    finally:
        loss_mod.fourier_filter = real_filter
    kinds = [k for k, _ in rec.calls]
    assert kinds == ["randn", "randn_like", "randn"], kinds   # sigma sampler, noise, offset
    case = {"loss_type": loss_type, "use_additional_loss": additional, "replace_cond_frames": replace, "num_frames": T, "B": B,
            "offset_noise_level": 0.02, "additional_loss_weight": 0.1, "cond_frames_choices": [c for c in CHOICES if len(c) < T],
            "input": x, "sigmas": seen["sigmas"], "cond_mask": seen["cond_mask"], "noise": rec.calls[1][1], "offset": rec.calls[2][1],
            "noised": seen["noised"], "model_output": seen["out"], "loss": got.clone()}
    if additional:
        case["predict_hf"], case["target_hf"] = hf
    return case


def api(classes):
    out = {}
    for cls in classes:
        params = []
        for p in list(inspect.signature(cls.__init__).parameters.values())[1:]:
            if p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD):
                continue
            params.append({"name": p.name, "default": None if p.default is p.empty else repr(p.default), "required": p.default is p.empty})
        out[cls.__name__] = {"target": f"{cls.__module__}.{cls.__name__}", "params": params}
    return out


def main():
    loss_mod, lw, ss, util = reference_modules()
    cases, seed = [], 100
    # every combination at 8 x 16, T = 5; the additional terms with the blend on the tie plane (8 x 8) and the odd plane (5 x 7); T = 1
    table = [(lt, ad, rp, 5, 8, 16) for lt, ad, rp in itertools.product(("l2", "l1"), (False, True), (False, True))]
    table += [(lt, True, True, 5, H, W) for lt in ("l2", "l1") for H, W in ((8, 8), (5, 7))]
    table += [(lt, True, True, 1, 8, 16) for lt in ("l2", "l1")] + [("l2", False, False, 1, 5, 7)]
    for lt, ad, rp, T, H, W in table:
        seed += 1
        cases.append(one_case(loss_mod, lt, ad, rp, T, H, W, seed))
    # fourier_filter alone, scale 0 and 0.5, on unit-normal planes of every shape the tests use (72 x 128 stays out: too large to commit)
    torch.manual_seed(7)
    filt = []
    for (H, W), scale in itertools.product(((8, 8), (8, 16), (5, 7), (1, 1), (1, 12)), (0.0, 0.5)):
        x = torch.randn(2, 3, H, W)
        filt.append({"H": H, "W": W, "scale": scale, "x": x, "y": util.fourier_filter(x, scale)})
    sig = torch.tensor([0.002, 0.05, 0.5, 1.0, 2.718, 40.0, 700.0])
    weights = {"sigma": sig, "Unit": lw.UnitWeighting()(sig), "EDM": lw.EDMWeighting()(sig), "EDM_0.7": lw.EDMWeighting(sigma_data=0.7)(sig),
               "V": lw.VWeighting()(sig), "Eps": lw.EpsWeighting()(sig)}
    rand = torch.tensor([-2.0, -0.5, 0.0, 0.25, 1.5, 3.0])
    idx = torch.tensor([0, 3, 9, 5, 1, 7])
    disc = {"target": "vwm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": {"sigma_min": 0.002, "sigma_max": 700.0, "rho": 7.0}}
    torch.manual_seed(11)
    drawn = ss.EDMSampling(p_mean=1.0, p_std=1.6, num_frames=3)(6)
    samplers = {"rand": rand, "EDM_default": ss.EDMSampling()(6, rand=rand), "EDM_phase2": ss.EDMSampling(p_mean=1.0, p_std=1.6)(6, rand=rand),
                "EDM_seed11_frames3": drawn, "idx": idx, "discretization_config": disc,
                "Discrete": ss.DiscreteSampling(disc, 10)(6, rand=idx), "Discrete_table": ss.DiscreteSampling(disc, 10).sigmas,
                "Discrete_noflip_zero": ss.DiscreteSampling(disc, 10, do_append_zero=True, flip=False).sigmas}
    os.makedirs(GOLD, exist_ok=True)
    torch.save({"cases": cases, "fourier_filter": filt, "weightings": weights, "samplers": samplers},
               os.path.join(GOLD, "diffusion_loss_tiny.pt"))
    with open(os.path.join(GOLD, "loss_api.json"), "w") as f:
        json.dump(api([lw.UnitWeighting, lw.EDMWeighting, lw.VWeighting, lw.EpsWeighting, ss.EDMSampling, ss.DiscreteSampling,
                       loss_mod.StandardDiffusionLoss]), f, indent=1, sort_keys=True)
        f.write("\n")
    import yaml
    with open(os.path.join(ref_shim.REF_ROOT, "configs", "training", "vista_phase2_stage2.yaml")) as f:
        block = yaml.safe_load(f)["model"]["params"]["loss_fn_config"]
    with open(os.path.join(GOLD, "loss_fn_config.yaml"), "w") as f:
        yaml.safe_dump(block, f, sort_keys=False)
    print(len(cases), "cases;", os.path.getsize(os.path.join(GOLD, "diffusion_loss_tiny.pt")), "bytes")


if __name__ == "__main__":
    main()
