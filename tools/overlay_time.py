"""Times one vk_stroke_overlay_u8 launch over the 91 frames (4 rounds of T = 25) of a 576 x 1024 rollout with a typical HUD, out of place and in
place: device events around each of 200 launches after 5 warm-up launches. profiles/overlay.txt holds the figures of one run.
    python tools/overlay_time.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vista_amd import drive, ops  # noqa: E402

H, W, T, ROUNDS = 576, 1024, 25, 4
FULL = {"goal": [0.4, 0.6], "trajectory": [5.0, 0.5, 10.0, 1.0, 15.0, 2.5, 20.0, 5.0], "command": 1, "speed": [6.0, 7.0, 8.0, 9.0],
        "angle": [0.1, -0.2, 0.3, 0.05]}
ACTIONS = [FULL, {"command": 2, "trajectory": FULL["trajectory"]}, {"goal": [0.7, 0.5], "speed": FULL["speed"], "angle": FULL["angle"]}, FULL]


def timed(src, dst, plan, which, reps=200, warm=5):
    """(min, median, max) milliseconds of one launch."""
    for _ in range(warm):
        ops.stroke_overlay(src, plan, which, out=dst)
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in events:
        a.record()
        ops.stroke_overlay(src, plan, which, out=dst)
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in events)
    return t[0], t[len(t) // 2], t[-1]


def main():
    n = drive.round_range(ROUNDS - 1, T)[1]
    sets = [drive.hud_strokes(a, H, W) for a in ACTIONS]
    which = torch.tensor([drive.frame_round(i, T) for i in range(n)], dtype=torch.int32, device="cuda")
    frames = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator(device="cuda").manual_seed(0), dtype=torch.uint8, device="cuda")
    plan = ops.stroke_plan(sets)
    print("counts (sets, strokes, segments):", ops.stroke_counts(sets))
    lo, med, hi = timed(frames, torch.empty_like(frames), plan, which)
    nbytes = 2 * frames.numel()
    print(f"[timing] out of place: {n} x {H} x {W} x 3, min {lo * 1e3:.1f} us, median {med * 1e3:.1f} us, max {hi * 1e3:.1f} us; "
          f"{nbytes} bytes read + written -> {nbytes / (med * 1e-3) / 1e9:.1f} GB/s at the median")
    work = frames.clone()
    lo, med, hi = timed(work, work, plan, which)
    print(f"[timing] in place: min {lo * 1e3:.1f} us, median {med * 1e3:.1f} us, max {hi * 1e3:.1f} us (tiles outside every box return at once)")


if __name__ == "__main__":
    main()
