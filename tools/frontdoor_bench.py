"""Full-size run of the sampling front door on cuda:0 with wall time per stage: vista_amd.sample_utils.init_model from the shipped config
(1.65 B UNet, ViT-H/14 conditioner, first-stage encoder + decoder; seeded random weights unless --ckpt names a checkpoint), 25 synthetic 1600x900
pictures written as PNGs, vista_amd.sample.run at 576x1024 and the six perform_save_locally calls of the CLI.

    python tools/frontdoor_bench.py [--steps 50] [--rounds 1] [--ckpt vista.safetensors] [--eager] [--out DIR]
Prints one JSON line per run (the first includes weight packing and graph capture, the second is warm). Times on different machines are not
comparable: quote the same machine's `python bench.py` step next to them."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def seed_weights(module, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():   # as bench.build_model: every tensor re-randomised at a variance-preserving scale
        for name, p in module.named_parameters():
            if name.endswith("mix_factor"):
                p.normal_(0, 0.5, generator=g)
            elif p.dim() >= 2:
                p.normal_(0, float(p[0].numel()) ** -0.5, generator=g)
            elif name.endswith(".weight"):
                p.normal_(1.0, 0.1, generator=g)
            else:
                p.normal_(0, 0.02, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    from vista_amd.modules.attention import invalidate_packed
    torch.cuda.set_device(0)
    T, H, W = 25, 576, 1024
    SU.check_sizes(H, W, T, a.rounds)
    t0 = time.perf_counter()
    model = SU.init_model({"config": None, "ckpt": a.ckpt}, load_ckpt=a.ckpt is not None)
    if a.ckpt is None:
        for i, m in enumerate((model.model.diffusion_model, model.conditioner, model.first_stage_model)):
            seed_weights(m, i)
            invalidate_packed(m)
    torch.cuda.synchronize()
    t_model = time.perf_counter() - t0
    work = a.out or tempfile.mkdtemp(prefix="frontdoor_")
    os.makedirs(os.path.join(work, "frames"), exist_ok=True)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:900, 0:1600]
    frames = []
    for i in range(T):   # a drifting pattern with some texture: 25 different pictures of nuScenes' size
        img = np.stack([127 + 110 * np.sin((xx + 8 * i) / (40.0 + 9 * c)) * np.cos(yy / (31.0 + 5 * c)) for c in range(3)], -1)
        img += rng.normal(0, 8, img.shape)
        frames.append(os.path.join(work, "frames", f"{i:02}.png"))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(frames[-1])
    for r in range(a.runs):
        sample.seed_everything(23)
        timings = {}
        torch.cuda.reset_peak_memory_stats()
        samples, samples_z, inputs = sample.run(model, frames, None, height=H, width=W, n_frames=T, n_rounds=a.rounds, n_steps=a.steps,
                                                eager=a.eager, timings=timings)
        t1 = time.perf_counter()
        for path, x in ((os.path.join(work, f"run{r}", "virtual"), samples), (os.path.join(work, f"run{r}", "real"), inputs)):
            for mode in ("videos", "grids", "images"):
                SU.perform_save_locally(path, x, mode, "NUSCENES", 0)
        timings["save"] = time.perf_counter() - t1
        print(json.dumps({"run": r, "steps": a.steps, "rounds": a.rounds, "eager": a.eager, "frames_out": int(samples.shape[0]),
                          "size": [H, W], "init_model_s": round(t_model, 2), "stage_s": {k: round(v, 3) for k, v in timings.items()},
                          "sample_ms_per_step": round(1e3 * timings["sample"] / (a.steps * a.rounds), 2),
                          "finite": bool(torch.isfinite(samples).all()), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
                          "weights": a.ckpt or "seeded"}), flush=True)


if __name__ == "__main__":
    main()
