"""Times what the planner adds (vista_amd/plan.py); what it prints belongs in profiles/plan_round_time.txt (not yet written: see DESIGN f6).
  1. vk_candidate_frame_stats on (K, E, T, C, h, w) = (3, 5, 25, 4, 72, 128), t0 = 3 -- the ensembles of three candidates at full size -- against
     the three calls of vk_ensemble_frame_stats a caller without it makes (each on a dense copy of its 22 scored frames, the copy not timed):
     device events around each of 200 calls after 5 warm-up calls.
  2. One planned round of the full-size pipeline of tools/frontdoor_bench.py (shipped config, seeded random weights, 576 x 1024 x 25 frames):
     round 0 is stepped plainly, round 1 is planned over --candidates actions with --ens members of --score_steps steps and committed with
     --steps steps; wall time of the scoring, of the commit and of a plain round, and the decode / conditioner calls each made.
    python tools/plan_time.py [--candidates 3] [--ens 5] [--score_steps 10] [--steps 50] [--kernel_only]"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from vista_amd import ops  # noqa: E402

SHAPE, T0 = (3, 5, 25, 4, 72, 128), 3


def timed(fn, reps=200, warm=5):
    """(min, median, max) milliseconds of one call of fn."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in events:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in events)
    return t[0], t[len(t) // 2], t[-1]


def kernel():
    x = torch.randn(SHAPE, generator=torch.Generator(device="cuda").manual_seed(0), device="cuda") * 3 + 1
    tails = [x[k][:, T0:].contiguous() for k in range(SHAPE[0])]
    nbytes = 4 * sum(t.numel() for t in tails)
    for name, fn in (("vk_candidate_frame_stats, one call", lambda: ops.candidate_frame_stats(x, T0)),
                     ("vk_ensemble_frame_stats, three calls", lambda: [ops.ensemble_frame_stats(t, want_map=False) for t in tails])):
        lo, med, hi = timed(fn)
        print(f"[timing] {name}: {SHAPE} t0 {T0}, min {lo * 1e3:.1f} us, median {med * 1e3:.1f} us, max {hi * 1e3:.1f} us; {nbytes} bytes read "
              f"-> {nbytes / (med * 1e-3) / 1e9:.1f} GB/s at the median (host launches included)", flush=True)


def planned_round(a):
    from PIL import Image
    from tools.frontdoor_bench import seed_weights
    from vista_amd import drive, plan, sample
    from vista_amd import sample_utils as SU
    from vista_amd.modules.attention import invalidate_packed
    T, H, W = 25, 576, 1024
    SU.check_sizes(H, W, T, 2)
    model = SU.init_model({"config": None, "ckpt": None}, load_ckpt=False)
    for i, m in enumerate((model.model.diffusion_model, model.conditioner, model.first_stage_model)):
        seed_weights(m, i)
        invalidate_packed(m)
    work = tempfile.mkdtemp(prefix="plan_")
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:900, 0:1600]
    frames = []
    for i in range(T):
        img = np.stack([127 + 110 * np.sin((xx + 8 * i) / (40.0 + 9 * c)) * np.cos(yy / (31.0 + 5 * c)) for c in range(3)], -1)
        img += rng.normal(0, 8, img.shape)
        frames.append(os.path.join(work, f"{i:02}.png"))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(frames[-1])
    actions = [{"command": torch.tensor(k % 4)} for k in range(a.candidates)]
    calls = {"decode": 0, "condition": 0}
    decode, condition = model.decode_first_stage, model.condition_fn
    model.decode_first_stage = lambda *p, **k: (calls.__setitem__("decode", calls["decode"] + 1), decode(*p, **k))[1]
    model.condition_fn = lambda *p, **k: (calls.__setitem__("condition", calls["condition"] + 1), condition(*p, **k))[1]

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()
    sample.seed_everything(23)
    session = drive.DriveSession(model, frames, height=H, width=W, n_frames=T, n_steps=a.steps)
    planner = plan.Planner(session, ens_size=a.ens, score_steps=a.score_steps)
    t = clock()
    session.step(actions[0])             # (weight packing and graph capture fall into this round)
    print(f"[timing] round 0, plain, {a.steps} steps (first use: packing and capture included): {clock() - t:.2f} s", flush=True)
    warm = session.fork()
    t = clock()
    warm.step(actions[0])
    plain = clock() - t
    print(f"[timing] round 1, plain, {a.steps} steps: {plain:.2f} s", flush=True)
    calls.update(decode=0, condition=0)
    t = clock()
    scores = planner.score(actions)
    scoring = clock() - t
    scored = dict(calls)
    best = plan.require_best(scores, session.rounds)
    t = clock()
    session.step(actions[best])
    commit = clock() - t
    steps = a.candidates * a.ens * a.score_steps
    print(f"[timing] round 1, planned over {a.candidates} candidates x {a.ens} members x {a.score_steps} steps: scoring {scoring:.2f} s "
          f"({steps} UNet steps, {1e3 * scoring / steps:.1f} ms each with the decode, the conditioner runs and the statistics spread over them; "
          f"{scored['decode']} decode, {scored['condition']} conditioner calls), commit {commit:.2f} s; planned / plain round = "
          f"{(scoring + commit) / plain:.2f}", flush=True)
    print(f"[result] chosen {best}, reward {[round(float(v), 6) for v in scores.reward]} (seeded random weights: the numbers mean nothing)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--ens", type=int, default=5)
    ap.add_argument("--score_steps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel_only", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    kernel()
    if not a.kernel_only:
        planned_round(a)


if __name__ == "__main__":
    main()
