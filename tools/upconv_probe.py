"""Per-launch time of the UNet's upsample convolution, nine-tap (ops.conv3x3(..., ups=2)) against folded (ops.upconv2x2), at the three BASELINE
shapes for n = 50 and n = 25 images, with HIP events: the two forms alternated in one process, best of ROUNDS x REPS launches after a warm-up, the
folded form in both tile orders, TFLOP/s on the FLOPs each form actually executes, and the relative L2 distance of one output from the other.
One JSON line per (shape, n). Source of the per-launch table of profiles/upconv_fold.txt.

    python tools/upconv_probe.py [--n 50 25] [--rounds 3] [--reps 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vista_amd import ops  # noqa: E402

SHAPES = ((1280, 9, 16), (1280, 18, 32), (640, 36, 64))   # (channels, source H, source W) of the level 3->2, 2->1 and 1->0 upsamples


def best_ms(fn, rounds, reps):
    best = float("inf")
    for _ in range(rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for k in range(reps):
            fn()
            ev[k + 1].record()
        torch.cuda.synchronize()
        best = min([best] + [ev[k].elapsed_time(ev[k + 1]) for k in range(reps)])
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[50, 25])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    for C, H, W in SHAPES:
        w = torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5
        b = torch.randn(C, generator=g)
        pw9, pw4 = ops.pack_conv3x3(w, b), ops.pack_upconv2x2(w, b)
        for n in args.n:
            x = torch.randn(n, H * W, C, generator=g).to(ops.ACT).cuda()
            out9 = torch.empty((n * 4 * H * W, C), dtype=ops.ACT, device="cuda")
            out4 = torch.empty_like(out9)
            if not ops.upconv2x2_fits(x, pw4, n, H, W):
                print(json.dumps({"C": C, "H": H, "W": W, "n": n, "folded": "declined"}), flush=True)
                continue

            def nine():
                ops.conv3x3(x, pw9, n, H, W, ups=2, out=out9)

            def fold(fastest):
                def run():
                    ops.UPCONV_CLASS_FASTEST = fastest
                    ops.upconv2x2(x, pw4, n, H, W, out=out4)
                return run
            forms = {"nine_tap": nine, "folded_class_slowest": fold(False), "folded_class_fastest": fold(True)}
            for fn in forms.values():   # warm-up
                for _ in range(3):
                    fn()
            ms = {k: float("inf") for k in forms}
            for _ in range(args.rounds):   # alternated: one round of each form in turn
                for k, fn in forms.items():
                    ms[k] = min(ms[k], best_ms(fn, 1, args.reps))
            rel = ((out4.double() - out9.double()).norm() / out9.double().norm()).item()
            mac = n * 4 * H * W * C * C
            rec = {"C": C, "H": H, "W": W, "n": n, "rel_l2_folded_vs_nine_tap": rel}
            for k, t in ms.items():
                flop = 2.0 * mac * (9 if k == "nine_tap" else 4)
                rec[k] = {"ms": round(t, 4), "tflops_executed": round(flop / t * 1e-9, 1)}
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
