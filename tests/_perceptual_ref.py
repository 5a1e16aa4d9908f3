"""References for the CLIP-space scores (vista_amd/perceptual.py, csrc/perceptual.hip): float64 numpy restatements of vk_embed_row_stats,
vk_embed_mmd_sums, perceptual.frame_scores and perceptual.mmd, a float32 emulation of the stated per-pair arithmetic of vk_embed_mmd_sums,
the case table and the bound.

The bound. vk_embed_mmd_sums forms every pair's term in fp32 (normalised rows, differences, their running sum of squares, gamma times it,
expm1) and adds the terms in fp64, so a sum's relative error against float64 is a mean of its terms' fp32 errors. The bound is 4 x the largest
relative error of the emulation below against the float64 reference over the three sums of every case of a class of CASES, measured on the
CPU (tests/test_perceptual_cpu.py re-measures both on every run):
    plain sets (rows at a cosine of about 0.9): 1.7e-8 ... 4.5e-8 where a sum has thousands of terms, 2.6e-7 at (2, 3, 3), where S_xx is a
    single pair of 3 columns                                                                              -> MMD_REL_BOUND = 4 * 2.6e-7
    "near" sets (every pair a near-duplicate, |u - v|^2 < 1e-5): the differences are of rows each rounded to fp32 after normalisation, so a
    term carries that rounding relative to a far smaller number: 6.5e-8 (64 rows, d = 1024) ... 5.5e-6 (2 rows, d = 80)
                                                                                                           -> MMD_REL_BOUND_NEAR = 4 * 5.5e-6
What the bounds exclude: 1 - expf(..) in place of -expm1f(..) is off by 1.2e-4 ... 1.9e-4 at (2, 3, 3) and loses every term of every near set
(relative error 1); on the plain sets of 63 ... 129 rows it is off by up to 4.6e-7, ten times the emulation there. |u - v|^2 as 2 - 2 u.v is
off by 3.5e-6 at (2, 3, 3) and by 6e-3 ... 1.3e-1 on the near sets."""
import numpy as np

SIGMA = 10.0
MMD_REL_BOUND = 4 * 2.6e-7
MMD_REL_BOUND_NEAR = 4 * 5.5e-6
ROW_STATS_CASES = ((1, 1), (3, 80), (5, 1024), (65, 1000))
# (m, n, d), or (m, n, d, "near"): y = x + 1e-4 noise, row for row (make_sets)
CASES = ((1, 1, 1), (2, 3, 3), (63, 65, 80), (64, 64, 1024), (129, 64, 1024), (65, 63, 1000), (64, 64, 1024, "near"), (33, 33, 80, "near"),
         (2, 2, 80, "near"))
LARGE = tuple(c for c in CASES if len(c) == 3 and c[0] >= 63)   # plain sets whose sums have thousands of terms


def case_id(case):
    return "x".join(map(str, case))


def mmd_bound(case):
    return MMD_REL_BOUND_NEAR if len(case) > 3 else MMD_REL_BOUND


def make_sets(case, seed=0):
    """Two sets of fp32 rows of different lengths. Plain cases: rows around a common direction at a cosine of about 0.9, as the frames of
    one drive are (k from 0.998 to 1). "near": every row of x is one row plus 1e-3 noise and y = x + 1e-4 noise, row for row -- consecutive
    frames of a still scene; every |u - v|^2 is then below 1e-5 of |u|^2."""
    m, n, d = case[:3]
    rng = np.random.default_rng(1000 * seed + 7 * m + 3 * n + d)
    common = rng.standard_normal(d)
    if len(case) > 3:
        assert m == n
        x = (common + 1e-3 * rng.standard_normal((m, d))) * rng.uniform(0.5, 3.0, (m, 1))
        y = x + 1e-4 * rng.standard_normal((n, d))
    else:
        x = (rng.standard_normal((m, d)) + 3.0 * common) * rng.uniform(0.5, 3.0, (m, 1))
        y = (rng.standard_normal((n, d)) + 3.2 * common + 0.1) * rng.uniform(0.5, 3.0, (n, 1))
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------------
def row_stats_ref(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], axis=1)


def _unit64(x):
    x = x.astype(np.float64)
    return x / np.sqrt((x * x).sum(1, keepdims=True))


def _terms64(u, v, sigma):
    """(len(u), len(v)) float64: 1 - k for every pair of unit rows."""
    out = np.empty((u.shape[0], v.shape[0]))
    for i in range(u.shape[0]):
        diff = v - u[i]
        out[i] = -np.expm1(-(diff * diff).sum(1) / (2.0 * sigma * sigma))
    return out


def mmd_sums_ref(x, y, sigma=SIGMA):
    u, v = _unit64(x), _unit64(y)
    return np.array([np.triu(_terms64(u, u, sigma), 1).sum(), np.triu(_terms64(v, v, sigma), 1).sum(), _terms64(u, v, sigma).sum()])


def mmd_ref(x, y, sigma=SIGMA, scale=1000.0):
    """The definition: means of k over ALL pairs, the diagonal included (V-statistic), and over the pairs i != j (U-statistic)."""
    u, v = _unit64(x), _unit64(y)
    kxx, kyy, kxy = 1.0 - _terms64(u, u, sigma), 1.0 - _terms64(v, v, sigma), 1.0 - _terms64(u, v, sigma)
    m, n = len(u), len(v)
    biased = scale * (kxx.mean() + kyy.mean() - 2.0 * kxy.mean())
    unbiased = None
    if m > 1 and n > 1:
        unbiased = scale * ((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (n * (n - 1)) - 2.0 * kxy.mean())
    return {"biased": biased, "unbiased": unbiased, "m": m, "n": n}


def cosines_ref(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1))


def frame_scores_ref(e_pred, e_real):
    nan = np.array([np.nan])
    return {"sim": cosines_ref(e_pred, e_real), "step": np.concatenate([nan, cosines_ref(e_pred[1:], e_pred[:-1])]),
            "step_real": np.concatenate([nan, cosines_ref(e_real[1:], e_real[:-1])])}


# ---- the float32 emulation ---------------------------------------------------------------------------------------------------------------------
def _unit32(x):
    inv = (1.0 / np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)   # fp64 sum of squares, fp32 inverse norm
    return x * inv                                                                                  # one fp32 product per element


def _terms32(u, v, sigma, form):
    f32 = np.float32
    gamma = f32(1.0 / (2.0 * sigma * sigma))
    if form == "dot":   # |u - v|^2 as 2 - 2 u.v: the form the kernel must not take
        dot = np.zeros((u.shape[0], v.shape[0]), f32)
        for k in range(u.shape[1]):
            dot = (dot.astype(np.float64) + np.outer(u[:, k], v[:, k]).astype(np.float64)).astype(f32)
        d2 = np.maximum(f32(2.0) - f32(2.0) * dot, f32(0.0))
    else:               # fp32 differences; the running sum takes each square by FMA: one rounding per column, in column order
        d2 = np.zeros((u.shape[0], v.shape[0]), f32)
        for k in range(u.shape[1]):
            diff = (u[:, k][:, None] - v[:, k][None, :]).astype(np.float64)   # (the fp32 difference, widened: its square is exact in fp64)
            d2 = (d2.astype(np.float64) + diff * diff).astype(f32)
    arg = -(gamma * d2)
    assert arg.dtype == f32
    # expm1f / expf as correctly rounded fp32 functions (numpy's own float32 expm1 is up to 3 ulp off, and low on average by one)
    if form == "one_minus_exp":
        terms = f32(1.0) - np.exp(arg.astype(np.float64)).astype(f32)
    else:
        terms = -np.expm1(arg.astype(np.float64)).astype(f32)
    assert terms.dtype == f32
    return terms.astype(np.float64)


def mmd_sums_emulated(x, y, sigma=SIGMA, form="expm1"):
    """vk_embed_mmd_sums' arithmetic in numpy float32 (form "expm1"), or one of the two forms it must not take ("one_minus_exp", "dot");
    the terms are added in float64 (numpy's order, not the kernel's: in fp64 the order moves a sum by 1e-16 of itself)."""
    u, v = _unit32(x), _unit32(y)
    return np.array([np.triu(_terms32(u, u, sigma, form), 1).sum(), np.triu(_terms32(v, v, sigma, form), 1).sum(),
                     _terms32(u, v, sigma, form).sum()])


def rel_errors(got, want):
    """Per sum |got - want| / |want|; 0 where both are equal (a sum that is exactly 0 must come out exactly 0), inf where only want is 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))
