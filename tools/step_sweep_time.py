"""Full-size run of the step-budget sweep on cuda:0: the pipeline of tools/frontdoor_bench.py (shipped config, seeded random weights unless --ckpt
names a checkpoint, 25 synthetic 1600x900 pictures), vista_amd.step_sweep.run at 576x1024 x 25 frames with the CLI's default lists.

    python tools/step_sweep_time.py [--budgets 10,15,20,30,50] [--ref_steps 200] [--ckpt vista.safetensors] [--out profiles/step_sweep_time.txt]
Prints, and writes to --out, the seconds of every run's denoising loop (the reference run comes first and includes the graph capture) and the
time per call of the update kernels beside vk_sampler_update's (events around 50 calls each, on a step's own shapes). On seeded weights the
errors say nothing about a trained model; they are printed for the record's shape only. Nothing asserts a time."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.frontdoor_bench import seed_weights  # noqa: E402


def kernel_times(T, h, w, ld=8, reps=50):
    """us per call of vk_sampler_update, vk_sampler_update_2m (with history) and vk_dpmpp2m_step on a step's shapes."""
    from vista_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    x, hist, den, old = (torch.randn(T, 4, h, w, device="cuda", generator=g) for _ in range(4))
    net = torch.randn(2 * T, h * w, ld, device="cuda", generator=g)
    scale = torch.full((T,), 2.5, device="cuda")
    calls = {"vk_sampler_update": lambda: ops.sampler_update(x, net, scale, -0.9, 0.2, 3.0, 2.9),
             "vk_sampler_update_2m": lambda: ops.sampler_update_2m(x, net, scale, hist, -0.9, 0.2, 0.97, 0.04, -0.01, False),
             "vk_dpmpp2m_step": lambda: ops.dpmpp2m_step(x, den, old, 0.97, 0.04, -0.01, out=x)}
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
        out[name] = 1e3 * a.elapsed_time(b) / reps
    return out


def main():
    from vista_amd import step_sweep
    ap = argparse.ArgumentParser()
    ap.add_argument("--samplers", default=step_sweep.DEFAULT_SAMPLERS)
    ap.add_argument("--budgets", default=step_sweep.DEFAULT_BUDGETS)
    ap.add_argument("--ref_steps", type=int, default=200)
    ap.add_argument("--ref_sampler", default="DPMPP2MSampler")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_sweep_time.txt"))
    a = ap.parse_args()
    from PIL import Image
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    from vista_amd.modules.attention import invalidate_packed
    samplers, budgets = step_sweep.parse_samplers(a.samplers), step_sweep.parse_budgets(a.budgets, a.ref_steps)
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
    print(f"model ready after {t_model:.1f} s; sweeping {samplers} x {budgets} against {a.ref_sampler} at {a.ref_steps} steps", flush=True)
    work = tempfile.mkdtemp(prefix="step_sweep_")
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:900, 0:1600]
    frames = []
    for i in range(T):
        img = np.stack([127 + 110 * np.sin((xx + 8 * i) / (40.0 + 9 * c)) * np.cos(yy / (31.0 + 5 * c)) for c in range(3)], -1)
        img += rng.normal(0, 8, img.shape)
        frames.append(os.path.join(work, f"{i:02}.png"))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(frames[-1])
    sample.seed_everything(23)
    t0 = time.perf_counter()
    rep = step_sweep.run(model, frames, None, height=H, width=W, n_frames=T, samplers=samplers, budgets=budgets, ref_steps=a.ref_steps,
                         ref_sampler=a.ref_sampler)
    scene = time.perf_counter() - t0
    lines = [f"step_sweep at {H} x {W} x {T} frames, weights: {a.ckpt or 'seeded random (errors below say nothing about a trained model)'}; one run each, "
             "spread not measured", f"init_model {t_model:.1f} s, the scene {scene:.1f} s",
             f"reference {rep.ref_sampler} at {rep.ref_steps} steps: {rep.ref_seconds:.2f} s ({1e3 * rep.ref_seconds / rep.ref_steps:.1f} ms/step, graph capture "
             f"included); ref_gap {rep.ref_gap:.3e}"]
    for r in rep.runs:
        lines.append(f"  {r['sampler']:16s} {r['steps']:4d} steps  {r['seconds']:7.2f} s  {1e3 * r['seconds'] / r['steps']:7.1f} ms/step   latent_err {r['latent_err']:.3e}")
    k = kernel_times(T, H // 8, W // 8)
    lines.append("update kernels on a step's shapes (us per call, events around 50 calls): " + ", ".join(f"{n} {v:.1f}" for n, v in k.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
