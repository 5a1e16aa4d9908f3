"""PSNR and SSIM of predicted against real frames, on the bytes that end up in the saved pictures.

`frame_metrics(pred, real)` converts float frames to 8 bit the way `perform_save_locally` does (ops.frames_to_u8), runs vk_frame_fidelity_u8
(csrc/fidelity.hip) over the two stacks and forms PSNR and the mean SSIM on the host in float64. SSIM is Wang, Bovik, Sheikh and Simoncelli
(2004): an 11-tap Gaussian window (sigma 1.5), valid positions only, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, per channel, then averaged over
the three channels. CLIP-space scores from the checkpoint's own image tower are in perceptual.py; LPIPS and FVD are not built.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

TAPS, SIGMA = 11, 1.5


def gaussian_window(taps=TAPS, sigma=SIGMA):
    """The 1-D window in float64, normalised to sum 1."""
    x = np.arange(taps, dtype=np.float64) - (taps - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


WINDOW_F64 = gaussian_window()
WINDOW_F32 = np.ascontiguousarray(WINDOW_F64.astype(np.float32))   # rounded once: the very table the kernel is handed
WINDOW_F32.setflags(write=False)


def window_ptr():
    """WINDOW_F32 as the `const float*` (host memory) vk_frame_fidelity_u8 reads during the call."""
    return WINDOW_F32.ctypes.data_as(C.POINTER(C.c_float))


@dataclass
class FidelityReport:
    sse: np.ndarray     # (n, 3) int64: sum of squared byte differences per frame and channel
    mse: np.ndarray     # (n,) float64: over all three channels
    psnr: np.ndarray    # (n,) float64: 10 log10(255^2 / mse); inf where the frames are identical
    ssim: np.ndarray    # (n,) float64: mean SSIM index over valid window positions and channels


def _as_u8(x, real, name):
    import torch
    from . import ops
    if x.dtype == torch.uint8:
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"frame_metrics: {name} is uint8 and must be (n, H, W, 3), got {tuple(x.shape)}")
        return x.contiguous()
    if x.dtype == torch.float32:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"frame_metrics: {name} is fp32 and must be (n, 3, H, W), got {tuple(x.shape)}")
        return ops.frames_to_u8(x, real=real)
    raise TypeError(f"frame_metrics: {name} must be uint8 (n, H, W, 3) or fp32 (n, 3, H, W) frames, got {x.dtype}")


def report_from_sums(sse, ssim_sum, H, W):
    """(n, 3) int64 squared-difference sums and (n, 3) float64 SSIM map sums of (H, W) frames -> FidelityReport, in float64 on the host."""
    sse = np.asarray(sse, dtype=np.int64).reshape(-1, 3)
    ssim_sum = np.asarray(ssim_sum, dtype=np.float64).reshape(-1, 3)
    total = sse.sum(axis=1)
    mse = total.astype(np.float64) / (3.0 * H * W)
    psnr = np.full(total.shape, np.inf, dtype=np.float64)
    nz = total > 0
    psnr[nz] = 10.0 * np.log10(255.0 * 255.0 * 3.0 * H * W / total[nz].astype(np.float64))
    ssim = (ssim_sum / float((H - (TAPS - 1)) * (W - (TAPS - 1)))).mean(axis=1)
    return FidelityReport(sse=sse, mse=mse, psnr=psnr, ssim=ssim)


def frame_metrics(pred, real):
    """pred, real: uint8 (n, H, W, 3) stacks, or fp32 (n, 3, H, W) frames -- `pred` samples in [0, 1], `real` inputs in [-1, 1], converted with
    ops.frames_to_u8 as the saved pictures are -> FidelityReport. Frames pair up by index; both on the GPU, H, W >= 11."""
    from . import ops
    a, b = _as_u8(pred, False, "pred"), _as_u8(real, True, "real")
    if a.shape != b.shape:
        raise ValueError(f"frame_metrics: pred has {tuple(a.shape)} bytes, real {tuple(b.shape)}: the stacks must pair up frame by frame")
    n, H, W, _ = a.shape
    if H < TAPS or W < TAPS:
        raise ValueError(f"frame_metrics: {H} x {W} frames are smaller than the {TAPS} x {TAPS} SSIM window")
    if n == 0:
        return report_from_sums(np.zeros((0, 3), np.int64), np.zeros((0, 3)), H, W)
    sse, ssim_sum = ops.frame_fidelity_u8(a, b)
    return report_from_sums(sse.cpu().numpy(), ssim_sum.cpu().numpy(), H, W)
