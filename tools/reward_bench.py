"""Full-size run of the reward front door on cuda:0 with wall time per stage: the pipeline of tools/frontdoor_bench.py (shipped config, seeded
random weights unless --ckpt names a checkpoint, 25 synthetic 1600x900 pictures), vista_amd.reward.run at 576x1024 x 25 frames with
--ens members x --steps steps per candidate.

    python tools/reward_bench.py [--ens 5] [--steps 10] [--candidates 1] [--maps] [--ckpt vista.safetensors] [--eager] [--out DIR]
Prints one JSON line per run (the first includes weight packing and graph capture, the second is warm). The expectation to hold a line against
is ens x steps UNet steps at the same machine's `python bench.py` step time plus one encode, per candidate."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ens", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=1, help="1: no action; 2: + a trajectory")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--maps", action="store_true", help="also write the heat videos")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image
    from vista_amd import reward
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
    work = a.out or tempfile.mkdtemp(prefix="reward_")
    os.makedirs(os.path.join(work, "frames"), exist_ok=True)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:900, 0:1600]
    frames = []
    for i in range(T):
        img = np.stack([127 + 110 * np.sin((xx + 8 * i) / (40.0 + 9 * c)) * np.cos(yy / (31.0 + 5 * c)) for c in range(3)], -1)
        img += rng.normal(0, 8, img.shape)
        frames.append(os.path.join(work, "frames", f"{i:02}.png"))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(frames[-1])
    actions = [{}, {"trajectory": torch.tensor([0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2])}][:max(1, min(2, a.candidates))]
    names = ["free", "traj"][:len(actions)]
    for r in range(a.runs):
        reward.seed_everything(23)
        timings, inputs = {}, []
        torch.cuda.reset_peak_memory_stats()
        reports = reward.run(model, frames, actions, height=H, width=W, n_frames=T, n_steps=a.steps, ens_size=a.ens, eager=a.eager,
                             want_map=a.maps, timings=timings, inputs_out=inputs)
        t1 = time.perf_counter()
        save = os.path.join(work, f"run{r}")
        for mode in ("videos", "grids", "images"):
            SU.perform_save_locally(os.path.join(save, "real"), inputs[0], mode, "NUSCENES", 0)
        if a.maps:
            reward.save_heat_videos(save, inputs[0], [(n, act, None) for n, act in zip(names, actions)], reports, "NUSCENES", 0)
        timings["save"] = time.perf_counter() - t1
        steps = a.ens * a.steps * len(actions)
        print(json.dumps({"run": r, "ens": a.ens, "steps": a.steps, "candidates": names, "eager": a.eager, "size": [H, W], "frames": T,
                          "init_model_s": round(t_model, 2), "stage_s": {k: round(v, 3) for k, v in timings.items()},
                          "sample_ms_per_unet_step": round(1e3 * timings["sample"] / steps, 2), "unet_steps": steps,
                          "rewards": [float(rep.reward) for rep in reports], "mean_variance": [rep.mean_variance for rep in reports],
                          "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), "weights": a.ckpt or "seeded"}), flush=True)


if __name__ == "__main__":
    main()
