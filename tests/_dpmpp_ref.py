"""Yardsticks of the DPM-Solver++(2M) tests, independent of vista_amd: nothing here imports the package.

  * float64 numpy: the recurrence in the form k-diffusion's sample_dpmpp_2m states it (t = -ln sigma, h, r, denoised_d; first-order first and
    final steps), the Euler recurrence beside it, the (a, b, c) coefficients of `x' = a x + b d + c d_old` derived from that form, the EDM
    schedule, and the analytic denoiser of Gaussian data with its exact probability-flow solution.
  * torch: `sample_with(denoise_fn, update, ...)`, the scaffolding of oracle.vista_oracle.euler_edm_sample (in-place scale of a clone, replace
    before each step and after the loop, guider_prepare_inputs / guider_combine) around a swappable update: "euler" (the oracle's own two
    expressions, so the scaffolding can be pinned to the oracle bit for bit) or "2m".
"""
import math

import numpy as np
import torch

from oracle import vista_oracle as O


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------------
def edm_sigmas_f64(n, sigma_min=0.002, sigma_max=700.0, rho=7.0):
    """EDMDiscretization in float64, with the appended 0: n + 1 values, n steps."""
    ramp = np.linspace(0.0, 1.0, n)
    lo, hi = sigma_min ** (1.0 / rho), sigma_max ** (1.0 / rho)
    return np.concatenate([(hi + ramp * (lo - hi)) ** rho, [0.0]])


def coefficients_f64(sigmas):
    """[(a, b, c)] per step from sample_dpmpp_2m's expressions: x' = (s_next / s) x - expm1(-h) denoised_d,
    denoised_d = (1 + 1 / (2 r)) d - (1 / (2 r)) d_old."""
    s = [float(v) for v in sigmas]
    out, have_old = [], False
    for i in range(len(s) - 1):
        if s[i + 1] == 0.0:
            out.append((0.0, 1.0, 0.0))   # h = inf: s_next / s = 0, -expm1(-inf) = 1
            have_old = True
            continue
        t, t_next = -math.log(s[i]), -math.log(s[i + 1])
        h = t_next - t
        e = -math.expm1(-h)
        if not have_old:
            out.append((s[i + 1] / s[i], e, 0.0))
        else:
            r = (t - (-math.log(s[i - 1]))) / h
            out.append((s[i + 1] / s[i], e * (1.0 + 1.0 / (2.0 * r)), -e / (2.0 * r)))
        have_old = True
    return out


def _replace(x, cond_frame, mask):
    m = mask.reshape((-1,) + (1,) * (x.ndim - 1))
    return x * (1.0 - m) + cond_frame * m


def sample_f64(denoise, x, sigmas, update, cond_frame=None, mask=None):
    """denoise(x, sigma) -> denoised, numpy float64. `x` is the already scaled start. update: "euler" | "2m"."""
    x = np.array(x, dtype=np.float64)
    s = [float(v) for v in sigmas]
    replace = mask is not None and bool(np.any(mask))
    old = None
    for i in range(len(s) - 1):
        if replace:
            x = _replace(x, cond_frame, mask)
        den = denoise(x, s[i])
        if update == "euler":
            x = x + (x - den) / s[i] * (s[i + 1] - s[i])
        elif s[i + 1] == 0.0:
            x = den
        else:
            t, t_next = -math.log(s[i]), -math.log(s[i + 1])
            h = t_next - t
            if old is None:
                x = (s[i + 1] / s[i]) * x - math.expm1(-h) * den
            else:
                r = (t - (-math.log(s[i - 1]))) / h
                den_d = (1.0 + 1.0 / (2.0 * r)) * den - (1.0 / (2.0 * r)) * old
                x = (s[i + 1] / s[i]) * x - math.expm1(-h) * den_d
        old = den
    if replace:
        x = _replace(x, cond_frame, mask)
    return x


def gaussian_denoiser(s):
    """The exact denoiser of data ~ N(0, s^2): D(x, sigma) = x s^2 / (s^2 + sigma^2)."""
    return lambda x, sigma: x * (s * s / (s * s + sigma * sigma))


def gaussian_exact(x0, s, sigma0):
    """The probability-flow solution at sigma = 0 from x0 at sigma0: dx/dsigma = x sigma / (s^2 + sigma^2)."""
    return x0 * s / math.sqrt(s * s + sigma0 * sigma0)


def order_error(update, n, s):
    """Relative error at sigma = 0 of an n-step run on the Gaussian denoiser over the EDM schedule (linear in x: one scalar suffices)."""
    sig = edm_sigmas_f64(n)
    x0 = math.sqrt(1.0 + sig[0] ** 2)
    got = float(sample_f64(gaussian_denoiser(s), np.array([x0]), sig, update)[0])
    want = gaussian_exact(x0, s, sig[0])
    return abs(got - want) / abs(want)


# ---- torch -----------------------------------------------------------------------------------------------------------------------------------
def sample_with(denoise_fn, update, x, cond, uc, cond_frame, cond_mask, num_steps, scale=2.5, guider="cfg"):
    """euler_edm_sample's loop (oracle/vista_oracle.py) with the update swapped; every tensor keeps x's dtype."""
    x = x.clone()
    sigmas = O.edm_sigmas(num_steps)
    x *= torch.sqrt(1.0 + sigmas[0] ** 2)
    s_in = x.new_ones([x.shape[0]])
    replace = cond_mask is not None and bool(cond_mask.any())
    coef = coefficients_f64(sigmas)
    old = None
    for i in range(len(sigmas) - 1):
        if replace:
            x = x * O.append_dims(1 - cond_mask, x.ndim) + cond_frame * O.append_dims(cond_mask, cond_frame.ndim)
        sigma, next_sigma = s_in * sigmas[i], s_in * sigmas[i + 1]
        if guider == "identity":
            denoised = denoise_fn(x, sigma, cond, cond_mask)
        else:
            denoised = O.guider_combine(denoise_fn(*O.guider_prepare_inputs(x, sigma, cond, cond_mask, uc)), scale)
        if update == "euler":
            d = (x - denoised) / O.append_dims(sigma, x.ndim)
            x = x + O.append_dims(next_sigma - sigma, x.ndim) * d
        elif update == "2m":
            a, b, c = coef[i]
            x = a * x + b * denoised + (c * old if c != 0.0 else 0.0)
            old = denoised
        else:
            raise ValueError(update)
    if replace:
        x = x * O.append_dims(1 - cond_mask, x.ndim) + cond_frame * O.append_dims(cond_mask, cond_frame.ndim)
    return x
