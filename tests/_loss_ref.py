"""This repository's own float64 restatement of the denoising loss (torch on the CPU, torch.fft in float64): what StandardDiffusionLoss and the
kernels of csrc/loss.hip are held to. It imports nothing from the reference, so it runs wherever the tests run.

Definitions (n = B * T images of C x H x W, frame t of clip b is image b * T + t):
  predict = out * (1 - m) + target * m per image (m = cond_mask; out where there is none)
  e       = (predict - target)^2 (l2) or |predict - target| (l1)
  dd      = (target_t - target_{t-1}) - (predict_t - predict_{t-1}), a = dd^2 or |dd|, for t >= 1
  norm    = per (clip, channel): sqrt(sum a^2) (l2) or sum a (l1) over (t >= 1, h, w); aux_w = 1 at t = 0, else 1 + a / max(norm, 1e-12)
  hf      = fourier_filter(predict, 0) - fourier_filter(target, 0)
  S0, S1, S2 per image = sum e, sum e * aux_w, sum hf^2 or |hf|
  loss    = w_i S0_i / (C H W) per image, or mean_i[w_i S1_i / (C H W)] + lambda * mean_i[w_i S2_i / (C H W)] with the additional terms

`defect=` switches one deliberate mistake on (tests/test_denoise_loss_cpu.py shows that each of them exceeds the parity bound):
  "pair_shift"  frame differences paired one frame off        "norm_axis"  the norm taken over the channel axis instead of (t, h, w)
  "no_blend"    the cond-frame blend left out                 "aux_t0"     the dynamics weight applied at t = 0 too
  "tie_flip"    one tie frequency of the 8 x 8 mask flipped   "mask_sym"   the mask of an odd plane symmetrised
  "w_frame"     every frame weighted with its neighbour's w
"""
import math

import torch

F64 = torch.float64
# The reference computes in fp32: the largest relative distance (max |reference - restatement| / max |reference| per output) of its losses from
# this float64 restatement over every configuration of tests/golden/diffusion_loss_tiny.pt, as measured on the CPU (profiles/diffusion_loss_parity.txt).
# It is rounding: fp32 element arithmetic of under ten operations, sums of at most 2^13 non-negative terms; a figure above 1e-5 would be a fault.
REFERENCE_LOSS_REL = 1.46e-7
LOSS_BOUND = 8 * REFERENCE_LOSS_REL
HIGHPASS_FACTOR = 16   # the high-pass kernel may be this many times further from float64 than the reference's own fp32 torch.fft path
DEFECTS = ("pair_shift", "norm_axis", "no_blend", "aux_t0", "tie_flip", "mask_sym", "w_frame")


def disc_mask(H, W, d_s=0.25, defect=None):
    """(H, W) bool over the SHIFTED spectrum (zero frequency at (H // 2, W // 2)): True inside the low-frequency disc, i.e. where the filter
    multiplies by `scale`. Python floats are doubles: the comparison is evaluated as the reference evaluates it."""
    inside = torch.zeros((H, W), dtype=torch.bool)
    for h in range(H):
        for w in range(W):
            inside[h, w] = (2 * h / H - 1) ** 2 + (2 * w / W - 1) ** 2 <= 2 * d_s
    if defect == "tie_flip" and (H, W) == (8, 8):
        inside[6, 6] = not bool(inside[6, 6])   # frequency (2, 2): d^2 = 0.25 + 0.25 equals 2 * d_s exactly
    if defect == "mask_sym":
        u = torch.fft.ifftshift(inside)
        mirrored = torch.roll(u.flip(0, 1), shifts=(1, 1), dims=(0, 1))   # frequency (-kh, -kw)
        inside = torch.fft.fftshift(u | mirrored)
    return inside


def fourier_filter(x, scale, d_s=0.25, defect=None, dtype=F64):
    """x (..., H, W) -> `dtype` (float64: the yardstick; float32: the arithmetic of the reference's own torch.fft path, whose distance from the
    yardstick sizes the kernel's bound): 2-D DFT, the disc multiplied by `scale`, inverse DFT, real part."""
    x = x.to(dtype)
    H, W = x.shape[-2:]
    factor = torch.ones((H, W), dtype=dtype)
    factor[disc_mask(H, W, d_s, defect)] = scale
    freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1)) * factor
    return torch.fft.ifftn(torch.fft.ifftshift(freq, dim=(-2, -1)), dim=(-2, -1)).real


def filter_error(y, y64, x):
    """Per plane: max |y - y64| / rms(x), x the filter's input. -> a tensor over the leading axes."""
    rms = x.to(F64).pow(2).mean((-2, -1)).sqrt()
    err = (y.to(F64) - y64).abs().amax((-2, -1))
    return torch.where(err == 0, torch.zeros_like(err), err / rms)


def rel(got, ref):
    """max |got - ref| / max |ref| (0 where both are 0 throughout)."""
    got, ref = torch.as_tensor(got, dtype=F64), torch.as_tensor(ref, dtype=F64)
    top = ref.abs().max().item()
    d = (got - ref).abs().max().item()
    return 0.0 if d == 0 else d / top if top > 0 else float("inf")


def noised_input_f32(x, noise, sigmas, cond_mask=None, offset=None, level=0.0):
    """torch's fp32 expression on the CPU, operation by operation: what vk_loss_noise_input must equal bit for bit."""
    x, noise, sigmas = x.float(), noise.float(), sigmas.float()
    if offset is not None:
        noise = noise + level * offset.float()[:, :, None, None]
    s = sigmas if cond_mask is None else (1 - cond_mask.float()) * sigmas
    return x + noise * s[:, None, None, None]


def blend(out, target, cond_mask=None, defect=None):
    out, target = out.to(F64), target.to(F64)
    if cond_mask is None or defect == "no_blend":
        return out
    m = cond_mask.to(F64)[:, None, None, None]
    return out * (1 - m) + target * m


def frame_sums(out, target, T, cond_mask=None, l1=False, additional=True, defect=None):
    """(n, 3) float64: S0, S1, S2 per image (S1 = S0 and S2 = 0 without the additional terms)."""
    target = target.to(F64)
    predict = blend(out, target, cond_mask, defect)
    n, C, H, W = target.shape
    diff = predict - target
    e = diff.abs() if l1 else diff ** 2
    s0 = e.reshape(n, -1).sum(1)
    if not additional:
        return torch.stack([s0, s0, torch.zeros_like(s0)], 1)
    B = n // T
    p, t = predict.reshape(B, T, C, H, W), target.reshape(B, T, C, H, W)
    if defect == "pair_shift" and T > 2:
        dd = (t[:, 1:] - t[:, :-1]) - (p[:, 1:] - torch.cat([p[:, :1], p[:, :-2]], 1))
    else:
        dd = (t[:, 1:] - t[:, :-1]) - (p[:, 1:] - p[:, :-1])
    a = dd.abs() if l1 else dd ** 2
    axes = (2,) if defect == "norm_axis" else (1, 3, 4)
    norm = a.sum(axes, keepdim=True) if l1 else (a ** 2).sum(axes, keepdim=True).sqrt()
    aux = 1 + a / norm.clamp_min(1e-12)
    head = aux[:, :1] if (defect == "aux_t0" and T > 1) else torch.ones((B, 1, C, H, W), dtype=F64)
    aux_w = torch.cat([head, aux], 1).reshape(n, C, H, W)
    s1 = (e * aux_w).reshape(n, -1).sum(1)
    hf = fourier_filter(predict, 0.0, defect=defect) - fourier_filter(target, 0.0, defect=defect)
    s2 = (hf.abs() if l1 else hf ** 2).reshape(n, -1).sum(1)
    return torch.stack([s0, s1, s2], 1)


def assemble(sums, w, per_image, additional, lam, defect=None):
    w = w.reshape(-1).to(F64)
    if defect == "w_frame":
        w = torch.roll(w, 1)
    if not additional:
        return w * sums[:, 0] / per_image
    return (w * sums[:, 1] / per_image).mean() + lam * (w * sums[:, 2] / per_image).mean()


def loss(out, target, w, T, cond_mask=None, loss_type="l2", additional=True, lam=0.0, defect=None):
    """What the reference's _forward returns for a denoiser output `out`: the per-image vector, or the scalar with the additional terms."""
    sums = frame_sums(out, target, T, cond_mask, loss_type == "l1", additional, defect)
    return assemble(sums, w, target[0].numel(), additional, lam, defect)


def weighting(name, sigma, sigma_data=0.5):
    s = sigma.to(F64)
    if name == "Unit":
        return torch.ones_like(s)
    if name == "Eps":
        return s ** -2.0
    sd = 1.0 if name == "V" else sigma_data
    return (s ** 2 + sd ** 2) / (s * sd) ** 2


def sigma_grid(n, p_mean, p_std):
    """The mid-quantiles of the log-normal: exp(p_mean + p_std * Phi^-1((i + 0.5) / n))."""
    from statistics import NormalDist
    return [math.exp(p_mean + p_std * NormalDist().inv_cdf((i + 0.5) / n)) for i in range(n)]
