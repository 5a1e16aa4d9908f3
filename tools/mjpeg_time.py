"""Times the Motion-JPEG output path on one MI355X, for the 25 frames of one window and the 91 frames of a 4-round rollout at 576 x 1024:
each of the three kernels (device events), the whole save_video call with VISTA_VIDEO=mjpeg (frames on the GPU -> the .avi on disk, wall clock),
and the animated-PNG path on the same frames (frames on the GPU -> .cpu().numpy() -> the .apng on disk), with both file sizes. Every figure is the
median of RUNS runs after one warm-up, with the smallest and the largest beside it. Nothing is asserted. profiles/mjpeg_time.txt holds one run.
    python tools/mjpeg_time.py [--out profiles/mjpeg_time.txt] [--quality 90] [--runs 5]"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vista_amd import _lib, ops  # noqa: E402
from vista_amd import sample_utils as SU  # noqa: E402

H, W = 576, 1024


def frames_u8(n):
    """A moving scene-like picture: smooth colour structure, an edge pattern and sensor-like noise (pure noise would flatter neither encoder)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.arange(H, device="cuda", dtype=torch.float32)[None, :, None, None]
    x = torch.arange(W, device="cuda", dtype=torch.float32)[None, None, :, None]
    t = torch.arange(n, device="cuda", dtype=torch.float32)[:, None, None, None]
    c = torch.arange(3, device="cuda", dtype=torch.float32)[None, None, None, :]
    base = 127 + 70 * torch.sin(x / (37 + 9 * c) + t / 5) * torch.cos(y / (29 + 5 * c)) + 30 * torch.sign(torch.sin((x + 3 * t) / 11) * torch.sin(y / 13))
    return (base + 4 * torch.randn(base.shape, generator=g, device="cuda")).clamp(0, 255).to(torch.uint8).contiguous()


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.3f} ms   (min {ms[0]:9.3f}, max {ms[-1]:9.3f}, {len(ms)} runs)"


def device_ms(fn, runs):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall_ms(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mjpeg_time.txt"))
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--runs", type=int, default=5)
    opt = ap.parse_args()
    lib, p = _lib.load(), ops._p
    lines = [f"Motion-JPEG output path, {torch.cuda.get_device_name(0)}, {H} x {W}, quality {opt.quality}: tools/mjpeg_time.py",
             "kernels: device events around one launch; save_video: wall clock from 8-bit frames on the GPU to the closed file (a temporary directory)", ""]
    for n in (25, 91):
        x = frames_u8(n)
        mh, mw = (H + 15) // 16, (W + 15) // 16
        blocks = n * 6 * mh * mw
        q = ops.jpeg_quant(opt.quality)
        coef = torch.empty((n, 6 * mh * mw, 64), dtype=torch.int16, device="cuda")
        sizes = torch.empty(n * mh, dtype=torch.int32, device="cuda")
        dct = lambda: lib.vk_jpeg_dct_quant_u8(p(x), p(coef), ctypes.byref(q), n, H, W, ops._stream())  # noqa: E731
        size = lambda: lib.vk_jpeg_interval_sizes(p(coef), p(sizes), n, mh, mw, blocks, ops._stream())  # noqa: E731
        t_dct, t_size = device_ms(dct, opt.runs), device_ms(size, opt.runs)
        offsets = torch.zeros(n * mh + 1, dtype=torch.int64, device="cuda")
        offsets[1:] = torch.cumsum(sizes, 0, dtype=torch.int64)
        total = int(offsets[-1])
        scan = torch.empty(total, dtype=torch.uint8, device="cuda")
        write = lambda: lib.vk_jpeg_entropy_write(p(coef), p(offsets), p(scan), total, n, mh, mw, blocks, ops._stream())  # noqa: E731
        t_write = device_ms(write, opt.runs)
        saved = {k: os.environ.get(k) for k in ("VISTA_VIDEO", "VISTA_VIDEO_QUALITY")}
        try:
            with tempfile.TemporaryDirectory() as tmp:
                stem = os.path.join(tmp, "v")
                os.environ["VISTA_VIDEO"], os.environ["VISTA_VIDEO_QUALITY"] = "mjpeg", str(opt.quality)
                t_avi = wall_ms(lambda: SU.save_video(stem, x, 10), opt.runs)
                avi_bytes = os.path.getsize(stem + ".avi")
                os.environ["VISTA_VIDEO"] = "apng"
                t_apng = wall_ms(lambda: SU.save_video(stem, x.cpu().numpy(), 10), opt.runs)
                apng = [f for f in os.listdir(tmp) if not f.endswith(".avi")][0]
                apng_bytes = os.path.getsize(os.path.join(tmp, apng))
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        lines += [f"{n} frames ({x.numel()} bytes of RGB, {blocks} blocks, {n * mh} restart intervals, scans {total} bytes)",
                  f"  vk_jpeg_dct_quant_u8     {stats(t_dct)}",
                  f"  vk_jpeg_interval_sizes   {stats(t_size)}",
                  f"  vk_jpeg_entropy_write    {stats(t_write)}",
                  f"  save_video, mjpeg        {stats(t_avi)}   -> {avi_bytes} bytes (.avi)",
                  f"  save_video, {apng.rsplit('.', 1)[1]:<12} {stats(t_apng)}   -> {apng_bytes} bytes (the path without the hook, same frames)", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
