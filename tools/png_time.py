"""Times the PNG output path on one MI355X, for the 25 frames of one window and the 91 frames of a 4-round rollout at 576 x 1024 and for their
grids: each of the three kernels (device events, median of RUNS runs after one warm-up), and `perform_save_locally` for `images` and for `grids`
with VISTA_PNG=hip and with the hook unset (Pillow), in the same call: wall clock from float frames on the GPU to the closed files in a temporary
directory (median of WALL_RUNS), with the bytes written in both modes. Nothing is asserted. profiles/png_time.txt holds one run.
    python tools/png_time.py [--out profiles/png_time.txt] [--runs 5] [--wall-runs 3]"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vista_amd import _lib, ops  # noqa: E402
from vista_amd import sample_utils as SU  # noqa: E402
from tools.mjpeg_time import H, W, device_ms, frames_u8, stats  # noqa: E402

SEG_ROWS = 16


def kernel_lines(lib, x, runs):
    """x (n, h, w, 3) uint8 on the GPU -> the three kernels' lines"""
    p = ops._p
    n, h, w, _ = x.shape
    rb, segs = 1 + 3 * w, (h + SEG_ROWS - 1) // SEG_ROWS
    ns = n * segs
    rows = torch.empty((n, h, rb), dtype=torch.uint8, device="cuda")
    sizes = torch.empty(ns, dtype=torch.int32, device="cuda")
    adler = torch.empty((ns, 2), dtype=torch.int32, device="cuda")
    plan = torch.empty((ns, ops.PNG_PLAN_WORDS), dtype=torch.int32, device="cuda")
    t_filter = device_ms(lambda: lib.vk_png_filter_u8(p(x), p(rows), n, h, w, ops._stream()), runs)
    t_plan = device_ms(lambda: lib.vk_png_deflate_plan(p(rows), p(sizes), p(adler), p(plan), n, h, rb, SEG_ROWS, ns, ops._stream()), runs)
    offsets = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(sizes, 0, dtype=torch.int64)
    total = int(offsets[-1])
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    t_write = device_ms(lambda: lib.vk_png_deflate_write(p(rows), p(plan), p(offsets), p(out), total, n, h, rb, SEG_ROWS, ns, ops._stream()), runs)
    return [f"  {n} x {h} x {w}: {rows.numel()} bytes of rows, {ns} segments, deflate data {total} bytes",
            f"    vk_png_filter_u8       {stats(t_filter)}",
            f"    vk_png_deflate_plan    {stats(t_plan)}",
            f"    vk_png_deflate_write   {stats(t_write)}"]


def save_ms(samples, mode, hook, runs):
    """perform_save_locally(mode) under VISTA_PNG=hook (None: unset) -> (wall-clock times in ms, bytes written by one call)"""
    saved = os.environ.get("VISTA_PNG")
    os.environ.pop("VISTA_PNG", None)
    if hook:
        os.environ["VISTA_PNG"] = hook
    try:
        out, written = [], 0
        for i in range(runs + 1):                      # (the first is the warm-up)
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                SU.perform_save_locally(os.path.join(tmp, "virtual"), samples, mode, "IMG", 0)
                torch.cuda.synchronize()
                if i:
                    out.append((time.perf_counter() - t0) * 1e3)
                folder = os.path.join(tmp, "virtual", mode)
                written = sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder))
        return out, written
    finally:
        os.environ.pop("VISTA_PNG", None)
        if saved is not None:
            os.environ["VISTA_PNG"] = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "png_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--wall-runs", type=int, default=3)
    opt = ap.parse_args()
    lib = _lib.load()
    lines = [f"PNG output path, {torch.cuda.get_device_name(0)}, {H} x {W}, segments of {SEG_ROWS} rows: tools/png_time.py",
             "kernels: device events around one launch; perform_save_locally: wall clock from float frames on the GPU to the closed files (a temporary",
             "directory), VISTA_PNG=hip and the hook unset (Pillow) in the same call", ""]
    for n in (25, 91):
        x = frames_u8(n)
        samples = (x.permute(0, 3, 1, 2).float() / 255.0).contiguous()
        grid = ops.frames_to_u8(samples, real=False, grid=True)
        lines.append(f"{n} frames")
        lines += kernel_lines(lib, x, opt.runs) + kernel_lines(lib, grid[None].contiguous(), opt.runs)
        for mode in ("images", "grids"):
            t_hip, b_hip = save_ms(samples, mode, "hip", opt.wall_runs)
            t_pil, b_pil = save_ms(samples, mode, None, opt.wall_runs)
            hip, pil = sorted(t_hip)[len(t_hip) // 2], sorted(t_pil)[len(t_pil) // 2]
            lines += [f"  perform_save_locally({mode}), VISTA_PNG=hip   {stats(t_hip)}   -> {b_hip} bytes",
                      f"  perform_save_locally({mode}), hook unset      {stats(t_pil)}   -> {b_pil} bytes",
                      f"    the hook's path takes {hip / pil:.4f} of the Pillow path's time ({pil / hip:.1f} x faster) and writes {b_hip / b_pil:.4f} of its bytes"]
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
