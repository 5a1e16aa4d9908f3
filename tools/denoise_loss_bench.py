"""Full-size run of the denoising-loss front door on cuda:0 with wall time per stage: the pipeline of tools/frontdoor_bench.py (shipped config,
seeded random weights unless --ckpt names a checkpoint, 25 synthetic 1600x900 pictures), vista_amd.denoise_loss.run at 576x1024 x 25 frames.

    python tools/denoise_loss_bench.py [--n_sigmas 8] [--runs 2] [--ckpt vista.safetensors] [--no_additional_loss]
Prints one JSON line per run (the first includes weight packing, the second is warm): `forward` is the n_sigmas eager denoiser forwards, `loss`
everything else of the per-sigma loop (noise draw, noising, high-pass, statistics, the copy of the sums to the host). The last line times the
three loss kernels alone (events around 20 calls each) on latents of the same shape."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.frontdoor_bench import seed_weights  # noqa: E402


def kernel_times(T, h, w, reps=20):
    from vista_amd import ops
    from vista_amd.modules.diffusionmodules.util import fourier_keep_mask_on
    g = torch.Generator(device="cuda").manual_seed(0)
    x, y = (torch.randn(T, 4, h, w, device="cuda", generator=g) for _ in range(2))
    sigma, mask = torch.full((T,), 2.0, device="cuda"), torch.zeros(T, device="cuda")
    keep = fourier_keep_mask_on(x.device, h, w)
    hf = ops.fourier_highpass(x, keep, 0.0, b=y, cond_mask=mask)
    calls = {"noise_input": lambda: ops.loss_noise_input(x, y, sigma, mask), "fourier_highpass": lambda: ops.fourier_highpass(x, keep, 0.0, b=y, cond_mask=mask),
             "loss_stats": lambda: ops.loss_stats(x, y, T, cond_mask=mask, hf=hf)}
    out = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(1e3 * a.elapsed_time(b) / reps, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_sigmas", type=int, default=8)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--no_additional_loss", action="store_true")
    a = ap.parse_args()
    from PIL import Image
    from vista_amd import denoise_loss, sample
    from vista_amd import sample_utils as SU
    from vista_amd.modules.attention import invalidate_packed
    torch.cuda.set_device(0)
    T, H, W = 25, 576, 1024
    SU.check_sizes(H, W, T, 1)
    t0 = time.perf_counter()
    model = SU.init_model({"config": None, "ckpt": a.ckpt}, load_ckpt=a.ckpt is not None)
    if a.ckpt is None:
        for i, m in enumerate((model.model.diffusion_model, model.conditioner, model.first_stage_model)):
            seed_weights(m, i)
            invalidate_packed(m)
    torch.cuda.synchronize()
    t_model = time.perf_counter() - t0
    work = tempfile.mkdtemp(prefix="denoise_loss_")
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:900, 0:1600]
    frames = []
    for i in range(T):
        img = np.stack([127 + 110 * np.sin((xx + 8 * i) / (40.0 + 9 * c)) * np.cos(yy / (31.0 + 5 * c)) for c in range(3)], -1)
        img += rng.normal(0, 8, img.shape)
        frames.append(os.path.join(work, f"{i:02}.png"))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(frames[-1])
    for r in range(a.runs):
        sample.seed_everything(23)
        timings = {}
        t0 = time.perf_counter()
        rep = denoise_loss.run(model, frames, None, height=H, width=W, n_frames=T, n_sigmas=a.n_sigmas, additional=not a.no_additional_loss,
                               timings=timings)
        print(json.dumps({"run": r, "n_sigmas": a.n_sigmas, "size": [H, W], "frames": T, "additional": not a.no_additional_loss,
                          "init_model_s": round(t_model, 2), "scene_s": round(time.perf_counter() - t0, 3),
                          "stage_s": {k: round(v, 4) for k, v in timings.items()},
                          "forward_ms_per_sigma": round(1e3 * timings["forward"] / a.n_sigmas, 2),
                          "loss_ms_per_sigma": round(1e3 * timings["loss"] / a.n_sigmas, 2), "sigmas": [round(s, 4) for s in rep.sigmas],
                          "loss": rep.loss, "mse": rep.mse, "weights": a.ckpt or "seeded"}), flush=True)
    print(json.dumps({"kernels": kernel_times(T, H // 8, W // 8)}), flush=True)


if __name__ == "__main__":
    main()
