"""What the fidelity tests share (tests/test_fidelity_cpu.py, tests/test_fidelity_gpu.py): the float64 SSIM reference in numpy, a numpy-float32
emulation of the kernel's stated arithmetic with and without the pivot, the case table and the SSIM bound.

The bound. The kernel forms every window's index in fp32 and sums the indices in fp64, so a frame's error against float64 is the mean of its
windows' fp32 errors. The bound is 4 x the largest frame error of the PIVOTED float32 emulation below against the float64 reference over
the case table (every shape x every content), measured on the CPU; the factor 4 is there because the kernel contracts the tap sums into
FMAs and may add taps in another order than numpy. Measured (tests/test_fidelity_cpu.py prints every entry; profiles/fidelity_parity.txt):
  * shapes with more than one window position: the largest pivoted error is 3.70e-6 (the 250...255 texture at 27 x 43; that content carries
    0.9e-6 ... 3.7e-6 at every such shape, every other content at most 7.4e-7)                              -> SSIM_BOUND = 1.48e-5
  * the one-window shape 11 x 11: a frame IS one window and nothing averages. On the 250...255 texture the pivoted moments are near
    125^2 = 15,600, where an fp32 ulp is 1e-3, against a denominator sxx + syy + C2 of 64: 2.13e-5 for that single index. One bound over
    both kinds of shape would be 8.5e-5 and sit above what it has to exclude (below), so the one-window shape has its own
                                                                                                            -> SSIM_BOUND_ONE_WINDOW = 8.5e-5
What the bound has to exclude: the same arithmetic WITHOUT the pivot is off by 6.67e-5 on flat 255 against flat 254 at every shape and by
3.0e-5 ... 5.1e-5 on the 250...255 texture at every shape with more than one window: 2x to 4.5x SSIM_BOUND. A kernel without the pivot fails
the table at nine shapes of ten; at 11 x 11 alone the bound cannot tell the two forms apart."""
import numpy as np

from vista_amd import fidelity, ops

TAPS = fidelity.TAPS
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
SSIM_BOUND = 4 * 3.70e-6              # frames of more than one window position
SSIM_BOUND_ONE_WINDOW = 4 * 2.13e-5   # H == W == 11
TILE_H, TILE_W = ops.FIDELITY_TILE_H, ops.FIDELITY_TILE_W

# (n, H, W): one window; a 39-byte row stride; an odd middle size; one position fewer / one more than a tile along each axis; two tiles plus
# one; a whole tile and one tile + 2 / two tiles + 2 at widths that take the 4-bytes-per-lane path; the tiny world; full row width
SHAPES = [(1, 11, 11), (2, 12, 13), (3, 21, 35),
          (3, TILE_H + TAPS - 2, TILE_W + TAPS - 2), (3, TILE_H + TAPS, TILE_W + TAPS), (2, 2 * TILE_H + TAPS, 2 * TILE_W + TAPS),
          (3, TILE_H + TAPS - 1, TILE_W + TAPS + 1), (2, 2 * TILE_H + TAPS - 1, 2 * TILE_W + TAPS + 1),
          (5, 128, 256), (1, 27, 1024)]
CONTENTS = ("noise_vs_noise", "noise_pm3", "flat255_vs_254", "flat255_vs_0", "bright_250_255", "ramp_pm8", "itself")


def ssim_bound(H, W):
    return SSIM_BOUND_ONE_WINDOW if (H, W) == (TAPS, TAPS) else SSIM_BOUND


def make_case(name, shape, seed=0):
    """-> (a, b) uint8 (n, H, W, 3)."""
    n, H, W = shape
    rng = np.random.default_rng([seed, n, H, W, CONTENTS.index(name)])
    full = (n, H, W, 3)
    if name == "noise_vs_noise":
        return rng.integers(0, 256, full, dtype=np.uint8), rng.integers(0, 256, full, dtype=np.uint8)
    if name == "noise_pm3":
        a = rng.integers(0, 256, full, dtype=np.int64)
        return a.astype(np.uint8), np.clip(a + rng.integers(-3, 4, full), 0, 255).astype(np.uint8)
    if name == "flat255_vs_254":
        return np.full(full, 255, np.uint8), np.full(full, 254, np.uint8)
    if name == "flat255_vs_0":
        return np.full(full, 255, np.uint8), np.zeros(full, np.uint8)
    if name == "bright_250_255":
        return rng.integers(250, 256, full, dtype=np.uint8), rng.integers(250, 256, full, dtype=np.uint8)
    if name == "ramp_pm8":
        yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
        a = (np.arange(n)[:, None, None, None] * 17 + (3 * xx + 2 * yy + 40 * cc)[None]) % 256
        return a.astype(np.uint8), np.clip(a + rng.integers(-8, 9, full), 0, 255).astype(np.uint8)
    if name == "itself":
        a = rng.integers(0, 256, full, dtype=np.uint8)
        return a, a.copy()
    raise KeyError(name)


def _filter(x, w, add_mul):
    """The separable valid window over axes 2 (columns: the rows pass) then 1 (rows: the columns pass) of (n, H, W, 3), taps in order."""
    Wd = x.shape[2] - (TAPS - 1)
    h = np.zeros(x.shape[:2] + (Wd, 3), dtype=x.dtype)
    for k in range(TAPS):
        h = add_mul(h, w[k], x[:, :, k:k + Wd])
    Hd = x.shape[1] - (TAPS - 1)
    v = np.zeros((x.shape[0], Hd, Wd, 3), dtype=x.dtype)
    for k in range(TAPS):
        v = add_mul(v, w[k], h[:, k:k + Hd])
    return v


def sse_ref(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).sum(axis=(1, 2))   # (n, 3) int64


def ssim_ref64(a, b, window=None):
    """Wang et al. 2004 in float64, with the very table the kernel is handed (fp32 values, held in float64) -> (n,) frame SSIM."""
    w = np.asarray(fidelity.WINDOW_F32 if window is None else window, dtype=np.float64)
    x, y = a.astype(np.float64), b.astype(np.float64)
    f = lambda t: _filter(t, w, lambda acc, wk, s: acc + wk * s)   # noqa: E731
    mx, my, xx, yy, xy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    sxx, syy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    index = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return index.mean(axis=(1, 2)).mean(axis=1)


def ssim_emulated32(a, b, pivot):
    """The kernel's stated arithmetic in numpy float32, one rounding per operation (no FMA): moments of x - pivot under the fp32 table, the
    pivot added back for the luminance term only, indices summed in float64 -> (n,) frame SSIM. pivot = 0 is the form without a pivot."""
    w = fidelity.WINDOW_F32
    p = np.float32(pivot)
    x, y = a.astype(np.float32) - p, b.astype(np.float32) - p
    f = lambda t: _filter(t, w, lambda acc, wk, s: acc + wk * s)   # noqa: E731
    mx, my, xx, yy, xy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    ux, uy = mx + p, my + p
    sxx, syy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    c1, c2, two = np.float32(C1), np.float32(C2), np.float32(2)
    index = ((two * (ux * uy) + c1) * (two * sxy + c2)) / (((ux * ux + uy * uy) + c1) * ((sxx + syy) + c2))
    assert index.dtype == np.float32
    return index.astype(np.float64).mean(axis=(1, 2)).mean(axis=1)
