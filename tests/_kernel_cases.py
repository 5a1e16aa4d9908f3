"""Case table and bounds of the kernel parity suites, one table per 16-bit storage type: make_cases(torch.float16) is the fp16-storage build's
(tests/_f16_cases.py, run by tests/test_f16_kernels_gpu.py under ops.storage(torch.float16)), make_cases(torch.bfloat16) the default build's
(tests/_bf16_cases.py, run by tests/test_bf16_kernels_gpu.py under ops.storage(torch.bfloat16)). tests/test_f16_bounds_cpu.py and
tests/test_bf16_bounds_cpu.py prove on the CPU that every bound passes the reference and fails a broken output.

A case is (build, ref64, run):
  build()            CPU tensors from a seeded generator; every 16-bit operand is already a value of the storage type (V operands of attention:
                     bf16 values in both builds);
  ref64(inputs)      plain torch in float64 from those same values -> list of outputs;
  run(ops, inputs)   the ops.* call on the GPU copies of the inputs (weight packs are built here, inside the storage context) -> list of outputs,
                     each in its true dtype (the storage type, bf16 for an alt_cols_from V block, fp32).
`specs` names the bound of every output. Nothing here touches a GPU at import time.

The GPU modules run every case on poisoned outputs inside guard bands (tests/_guard.py; tests/_parity_bodies.py: case_under_tile): `inputs` are
arena copies, the ops.* calls allocate arenas, and run() re-homes what a pack builds outside the allocation factories (rehome_pack: the colsum
of a LayerNorm fold, pack_ff_out) and takes a scratch copy of the one operand an entry point is declared to write (scratch).

Operand layouts (the `operand_*` cases; include/vista_hip.h: the operand contract): the supported NARROW side of every alignment switch of the GEMM
family -- out / res1 / res2 at 8 bytes past a 16-byte boundary or in rows of N + 4 elements, an fp32 out in rows of N + 4, activations off the
128-byte line -- at M = 260 (one full 256-row tile + a ragged one, a ragged third 128-row tile), N = 320, K = 192 (three K-steps). One operand
varies at a time, everything else keeps the allocator's alignment; the varied input sits in a skewed / strided arena (Case.layout), the varied output
in one of its own (_guard.empty), so a store rounded down to 16 bytes or a row stored ld wide damages poison. Bounds A / F32 as everywhere, nothing
adopted. Each run also makes the aligned call and prints whether the two are bitwise equal (asserted where the sources state it: the same tile
variant, or variants 4 and 7), and asserts with vk_gemm_tile_choice on the launch's own descriptor which side of the switch ran.

Bounds (derived, never taken from the code under test):
  A   single-rounding kernels. With u = 2^-11 (fp16; 2^-8 for a bf16 output) BOTH
        1. |out - ref| <= 1.25 u |ref| + (u / 4) rms(ref) for EVERY element (round-to-nearest is within u relative of the fp32 value; fp32
           accumulation over K <= 5120 moves that value by ~sqrt(K) 2^-24 rms < 5e-6 rms, two orders below the absolute term), and
        2. rel_l2(out, ref) <= 1.5 rel_l2(ref.to(dtype), ref): the floor is computed from the reference itself.
  F32 fp32 outputs: |out - ref| <= 2e-5 |ref| + 2e-5 rms(ref).
  B   kernels with a known internal 16-bit rounding (ff_fused: the hidden activation; attention: P and V are bf16 in both builds): the float64
      reference emulates that rounding, the bound is the rel-L2 measured against it on the MI355X + 25 % (B_BOUNDS_* below; the measured values
      are in profiles/f16_kernel_parity.txt and profiles/bf16_kernel_parity.txt). bf16 table: no adopted bound exceeds 1.5 x the rel-L2 of the
      emulating reference rounded once to bf16 -- the output-rounding floor, computed on the CPU (the reference itself sits at 1.0 x).
  X   bitwise: torch.equal with the reference cast to the output type.
  LN  LayerNorm fold at |mean| >> std. fp16: the bf16 suite's close() tolerance scaled by the ulp ratio 2^-3. bf16: the worst element in units of
      bound A's tolerance, measured on the MI355X + 25 % (LN_BOUNDS_BF16), and every element inside close() (1.6e-2 |ref| + 2e-2 rms) besides.
A LayerNorm folded into a weight pack multiplies gamma into the weight BEFORE the pack rounds it to the storage type, so the reference of a folded
case uses that rounded product (recomputed here with the pack's own fp32 arithmetic): "the same values" are the values the kernel is handed.
"""
import ctypes
import math
import types

import torch
import torch.nn.functional as F

from tests import _guard
from tests._guard import rehome_pack, scratch

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
TILE_CFGS = (0, 1, 2, 3, 4, 5, 7)
LOG2E = 1.4426950408889634

# ---- B bounds: rel-L2 against the emulating float64 reference, measured on the MI355X (profiles/f16_kernel_parity.txt) + 25 % ----
# name -> (measured, bound). Filled from ONE run; never from a second run of the kernel on its own output.
B_BOUNDS_F16 = {
    "ff_128_noln_plain/fused": (2.160e-04, 2.700e-04),
    "ff_128_noln_plain/two_kernel": (2.160e-04, 2.700e-04),
    "ff_128_noln_res/fused": (2.139e-04, 2.674e-04),
    "ff_128_noln_res/two_kernel": (2.139e-04, 2.674e-04),
    "ff_128_noln_blend/fused": (2.100e-04, 2.625e-04),
    "ff_128_noln_blend/two_kernel": (2.100e-04, 2.625e-04),
    "ff_128_ln_plain/fused": (2.168e-04, 2.710e-04),
    "ff_128_ln_plain/two_kernel": (2.168e-04, 2.710e-04),
    "ff_128_ln_res/fused": (2.124e-04, 2.655e-04),
    "ff_128_ln_res/two_kernel": (2.123e-04, 2.654e-04),
    "ff_128_ln_blend/fused": (2.112e-04, 2.640e-04),
    "ff_128_ln_blend/two_kernel": (2.112e-04, 2.640e-04),
    "ff_1000_noln_plain/fused": (2.166e-04, 2.707e-04),
    "ff_1000_noln_plain/two_kernel": (2.166e-04, 2.707e-04),
    "ff_1000_noln_res/fused": (2.123e-04, 2.654e-04),
    "ff_1000_noln_res/two_kernel": (2.123e-04, 2.654e-04),
    "ff_1000_noln_blend/fused": (2.100e-04, 2.625e-04),
    "ff_1000_noln_blend/two_kernel": (2.100e-04, 2.625e-04),
    "ff_1000_ln_plain/fused": (2.173e-04, 2.716e-04),
    "ff_1000_ln_plain/two_kernel": (2.173e-04, 2.716e-04),
    "ff_1000_ln_res/fused": (2.128e-04, 2.660e-04),
    "ff_1000_ln_res/two_kernel": (2.128e-04, 2.660e-04),
    "ff_1000_ln_blend/fused": (2.094e-04, 2.617e-04),
    "ff_1000_ln_blend/two_kernel": (2.094e-04, 2.617e-04),
    "ff_4173_noln_plain/fused": (2.164e-04, 2.705e-04),
    "ff_4173_noln_plain/two_kernel": (2.164e-04, 2.705e-04),
    "ff_4173_noln_res/fused": (2.128e-04, 2.660e-04),
    "ff_4173_noln_res/two_kernel": (2.128e-04, 2.660e-04),
    "ff_4173_noln_blend/fused": (2.104e-04, 2.630e-04),
    "ff_4173_noln_blend/two_kernel": (2.104e-04, 2.630e-04),
    "ff_4173_ln_plain/fused": (2.171e-04, 2.714e-04),
    "ff_4173_ln_plain/two_kernel": (2.171e-04, 2.714e-04),
    "ff_4173_ln_res/fused": (2.125e-04, 2.656e-04),
    "ff_4173_ln_res/two_kernel": (2.125e-04, 2.656e-04),
    "ff_4173_ln_blend/fused": (2.101e-04, 2.626e-04),
    "ff_4173_ln_blend/two_kernel": (2.101e-04, 2.626e-04),
    "attn_spatial_2x5x144": (2.082e-04, 2.603e-04),
    "attn_spatial_2x5x144_log2": (2.111e-04, 2.639e-04),
    "attn_spatial_2x3x200": (2.074e-04, 2.592e-04),
    "attn_spatial_2x3x200_log2": (2.081e-04, 2.602e-04),
    "attn_spatial_1x2x576": (2.096e-04, 2.620e-04),
    "attn_spatial_1x2x576_log2": (2.084e-04, 2.605e-04),
    "attn_spatial_1x1x2120": (2.084e-04, 2.605e-04),
    "attn_spatial_1x1x2120_log2": (2.073e-04, 2.592e-04),
    "attn_spatial_1x3x4104": (2.088e-04, 2.610e-04),
    "attn_spatial_1x3x4104_log2": (2.084e-04, 2.605e-04),
    "attn_spatial_1x1x2304_log2": (2.165e-04, 2.707e-04),
    "attn_zero_base_gain12": (3.836e-04, 4.795e-04),
    "attn_zero_base_gain400": (4.645e-05, 5.806e-05),
    "attn_max_free_fallback_gain60": (1.030e-04, 1.287e-04),
    "attn_spike_forces_rescale": (5.345e-04, 6.681e-04),
    "attn_temporal_2x25x40x5": (4.041e-04, 5.051e-04),
    "attn_temporal_2x7x9x1": (5.575e-04, 6.969e-04),
    "attn_temporal_1x32x16x3": (3.877e-04, 4.846e-04),
    "attn_temporal_1x3x4099x5": (5.269e-04, 6.586e-04),
    "attn_temporal_2x31x5x1": (3.920e-04, 4.900e-04),
}


# bf16 table: name -> (measured, bound), from ONE run of tests/test_bf16_kernels_gpu.py on the MI355X (profiles/bf16_kernel_parity.txt)
B_BOUNDS_BF16 = {
    "ff_128_noln_plain/fused": (1.668e-03, 2.085e-03),
    "ff_128_noln_plain/two_kernel": (1.668e-03, 2.085e-03),
    "ff_128_noln_res/fused": (1.663e-03, 2.079e-03),
    "ff_128_noln_res/two_kernel": (1.663e-03, 2.079e-03),
    "ff_128_noln_blend/fused": (1.673e-03, 2.091e-03),
    "ff_128_noln_blend/two_kernel": (1.673e-03, 2.091e-03),
    "ff_128_ln_plain/fused": (1.660e-03, 2.075e-03),
    "ff_128_ln_plain/two_kernel": (1.660e-03, 2.075e-03),
    "ff_128_ln_res/fused": (1.664e-03, 2.080e-03),
    "ff_128_ln_res/two_kernel": (1.664e-03, 2.080e-03),
    "ff_128_ln_blend/fused": (1.661e-03, 2.076e-03),
    "ff_128_ln_blend/two_kernel": (1.661e-03, 2.076e-03),
    "ff_1000_noln_plain/fused": (1.669e-03, 2.086e-03),
    "ff_1000_noln_plain/two_kernel": (1.669e-03, 2.086e-03),
    "ff_1000_noln_res/fused": (1.664e-03, 2.080e-03),
    "ff_1000_noln_res/two_kernel": (1.664e-03, 2.080e-03),
    "ff_1000_noln_blend/fused": (1.664e-03, 2.080e-03),
    "ff_1000_noln_blend/two_kernel": (1.664e-03, 2.080e-03),
    "ff_1000_ln_plain/fused": (1.671e-03, 2.089e-03),
    "ff_1000_ln_plain/two_kernel": (1.671e-03, 2.089e-03),
    "ff_1000_ln_res/fused": (1.657e-03, 2.071e-03),
    "ff_1000_ln_res/two_kernel": (1.657e-03, 2.071e-03),
    "ff_1000_ln_blend/fused": (1.668e-03, 2.085e-03),
    "ff_1000_ln_blend/two_kernel": (1.668e-03, 2.085e-03),
    "ff_4173_noln_plain/fused": (1.668e-03, 2.085e-03),
    "ff_4173_noln_plain/two_kernel": (1.668e-03, 2.085e-03),
    "ff_4173_noln_res/fused": (1.664e-03, 2.080e-03),
    "ff_4173_noln_res/two_kernel": (1.664e-03, 2.080e-03),
    "ff_4173_noln_blend/fused": (1.666e-03, 2.083e-03),
    "ff_4173_noln_blend/two_kernel": (1.666e-03, 2.083e-03),
    "ff_4173_ln_plain/fused": (1.671e-03, 2.089e-03),
    "ff_4173_ln_plain/two_kernel": (1.671e-03, 2.089e-03),
    "ff_4173_ln_res/fused": (1.662e-03, 2.077e-03),
    "ff_4173_ln_res/two_kernel": (1.662e-03, 2.077e-03),
    "ff_4173_ln_blend/fused": (1.665e-03, 2.081e-03),
    "ff_4173_ln_blend/two_kernel": (1.665e-03, 2.081e-03),
    "attn_zero_base_gain12": (1.369e-03, 1.711e-03),
    "attn_zero_base_gain400": (2.980e-04, 3.725e-04),
    "attn_max_free_fallback_gain60": (5.565e-04, 6.956e-04),
    "attn_spike_forces_rescale": (1.747e-03, 2.184e-03),
    "attn_spatial_2x5x144": (1.663e-03, 2.079e-03),
    "attn_spatial_2x5x144_log2": (1.654e-03, 2.067e-03),
    "attn_spatial_2x3x200": (1.663e-03, 2.079e-03),
    "attn_spatial_2x3x200_log2": (1.657e-03, 2.071e-03),
    "attn_spatial_1x2x576": (1.663e-03, 2.079e-03),
    "attn_spatial_1x2x576_log2": (1.673e-03, 2.091e-03),
    "attn_spatial_1x1x2120": (1.659e-03, 2.074e-03),
    "attn_spatial_1x1x2120_log2": (1.658e-03, 2.073e-03),
    "attn_spatial_1x3x4104": (1.659e-03, 2.074e-03),
    "attn_spatial_1x3x4104_log2": (1.656e-03, 2.070e-03),
    "attn_spatial_1x1x2304_log2": (1.654e-03, 2.067e-03),
    "attn_temporal_2x25x40x5": (1.697e-03, 2.121e-03),
    "attn_temporal_2x7x9x1": (1.740e-03, 2.175e-03),
    "attn_temporal_1x32x16x3": (1.693e-03, 2.116e-03),
    "attn_temporal_1x3x4099x5": (1.726e-03, 2.158e-03),
    "attn_temporal_2x31x5x1": (1.690e-03, 2.113e-03),
    "vt_attn_spatial_2x5x144": (1.661e-03, 2.076e-03),
    "vt_attn_spatial_2x3x200": (1.659e-03, 2.074e-03),
    "vt_attn_spatial_1x1x2120": (1.665e-03, 2.081e-03),
    "attn_small_2x4x257x80": (1.661e-03, 2.076e-03),
    "attn_small_3x2x50x64": (1.682e-03, 2.102e-03),
    "attn_small_1x2x300x128": (1.655e-03, 2.069e-03),
    "attn_small_2x1x5x80": (1.563e-03, 1.954e-03),
}

# bf16 table, LayerNorm fold at |mean| / std = 8 and 60: "<case>[<output>]" -> (worst element in units of bound A's tolerance as measured on the
# MI355X, that + 25 %), same run
LN_BOUNDS_BF16 = {
    "lnfold_mean_over_std_8_C320[0]": (0.7421, 0.9276),
    "lnfold_mean_over_std_8_C320[1]": (0.7421, 0.9276),
    "lnfold_mean_over_std_8_C1280[0]": (0.7415, 0.9269),
    "lnfold_mean_over_std_8_C1280[1]": (0.7415, 0.9269),
    "lnfold_mean_over_std_60_C320[0]": (0.7497, 0.9371),
    "lnfold_mean_over_std_60_C320[1]": (0.7497, 0.9371),
    "lnfold_mean_over_std_60_C1280[0]": (0.7532, 0.9415),
    "lnfold_mean_over_std_60_C1280[1]": (0.7627, 0.9534),
}


# ------------------------------------------------------------------------------------------------ bounds
def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).sum().sqrt() / b.pow(2).sum().sqrt().clamp_min(1e-300)).item()


def _unit(dtype):
    return 2.0 ** -11 if dtype is F16 else 2.0 ** -8


# ------------------------------------------------------------------------------------------------ helpers
class I(dict):
    __getattr__ = dict.__getitem__


def G(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def r32(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def to_device(i, device):
    return I({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in i.items()})


def d(t):
    return t.double()


class Norm:   # stands in for a LayerNorm parameter container
    def __init__(self, weight, bias, eps=1e-5):
        self.weight, self.bias, self.eps = weight, bias, eps


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def tok2nchw(x, n, H, W):
    return x.view(n, H, W, -1).permute(0, 3, 1, 2).contiguous()


def nchw2tok(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c)


def conv3x3_ref(x, w, b, n, H, W, stride=1, ups=1, asym=False):
    xi = tok2nchw(d(x), n, H, W)
    if ups == 2:
        xi = F.interpolate(xi, scale_factor=2, mode="nearest")
    if asym:
        return nchw2tok(F.conv2d(F.pad(xi, (0, 1, 0, 1)), d(w), d(b), stride=stride))
    return nchw2tok(F.conv2d(xi, d(w), d(b), stride=stride, padding=1))


def conv_t3_ref(x, w, b, B, T, S):
    C = x.shape[-1]
    x5 = d(x).view(B, T, S, 1, C).permute(0, 4, 1, 2, 3)
    return F.conv3d(x5, d(w), d(b), padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(B * T, S, -1)


class Case:
    """kbreak(inputs) -> inputs with the last 32 of K dropped from the weight (E.3; GEMM / conv cases). rows: the output rows of output 0 are
    its first dims flattened, except trans=True (linear_vt: (n, N, S), rows = (n, S)). cfgs: the forced tile variants of a tiles=True case
    (default: all of TILE_CFGS; conv3d: 0-3, as tests/test_vae_gpu.py). layout: input name -> (skew bytes, ld elements or None), honoured by
    tests/_guard.py: embed() -- that operand sits `skew` bytes past the allocator's alignment in rows `ld` elements apart, poison in between."""

    def __init__(self, name, build, ref, run, specs, tiles=False, kbreak=None, trans=False, group="gemm", cfgs=None, dround=None, layout=None):
        self.name, self.build, self.ref, self.run, self.specs = name, build, ref, run, specs
        self.tiles, self.kbreak, self.trans, self.group, self.dround, self.layout = tiles, kbreak, trans, group, dround, dict(layout or {})
        self.cfgs = (cfgs or TILE_CFGS) if tiles else (0,)   # the forced block tiles the GPU module runs the case under

    def __repr__(self):
        return self.name


def drop_k(key="w", n=32):
    def f(i):
        j = I(i)
        w = i[key].clone()
        if w.dim() == 2:
            w[:, -n:] = 0
        elif w.dim() == 4:     # conv3x3 [Cout][Cin][3][3]: the packed K order ends with tap (2, 2) of the last 64-channel slab
            w[:, -n:, 2, 2] = 0
        elif w.shape[-1] == 3:   # conv3d [Cout][Cin][3][3][3]: the centre tap's 32-wide K run of the last slab (the last tap, (2, 2, 2), reads
            w[:, -n:, 1, 1, 1] = 0   # only zero padding from the clip's last frame, which is where the last row tile lies)
        else:                  # conv_t3 [Cout][Cin][3][1][1]
            w[:, -n:, 2] = 0
        j[key] = w
        return j
    return f


def planned(ops, fn):
    """fn() with vk_gemm_tile_choice of every vk_gemm_bf16 launch it makes, asked about the launch's own descriptor -> (result, [variant * 16 + K slices])."""
    asked, gemm = [], ops._gemm

    def recording(desc, emit_stats=False, device=None):
        ops._prepare(desc)
        if emit_stats:   # planned as the launch will be: with a row-sum buffer (ops._gemm sets the real one; any 8-byte aligned address answers alike)
            desc.rowstat_out = desc.Wt
        asked.append(ops._lib.load().vk_gemm_tile_choice(ctypes.byref(desc)))
        if emit_stats:
            desc.rowstat_out = None
        return gemm(desc, emit_stats, device)
    ops._gemm = recording
    try:
        return fn(), asked
    finally:
        ops._gemm = gemm


def same_bits_stated(a, b):
    """Do the sources state that launches planned as a and b (variant * 16 + K slices) store the same bits? The same variant and K slices (the general
    epilogue is bitwise the LDS-staged one: csrc/gemm_common.h), or the pipelined kernel against the sixteen-wave one (include/vista_hip.h: 7 == 4)."""
    return a % 16 == b % 16 and (a // 16 == b // 16 or {a // 16, b // 16} == {4, 7})


def stats_follow_the_output(st, out):
    """RowStats slabs summed over parts against float64 (sum, sum of squares) of the kernel's own 16-bit output rows: the rule of
    tests/_parity_bodies.py: check_stats. -> worst error in units of the tolerance."""
    o = out.double()
    got = st.t.sum(0).double()
    ref = torch.stack([o.sum(1), o.pow(2).sum(1)], 1)
    tol = 2e-5 * torch.stack([o.abs().sum(1), o.pow(2).sum(1)], 1) + 1e-6
    return ((got - ref).abs() / tol).max().item()


def last_tile_rows(M, tile=128):
    return ((M - 1) // tile) * tile


def splice_last_tile(case, ref, ref_broken):
    """E.3: the reference with the rows of the last (ragged) 128-row tile taken from the K-dropped reference."""
    out = ref.contiguous().clone()
    if case.trans:
        n, N, S = ref.shape
        a, b = out.transpose(1, 2).reshape(n * S, N).clone(), ref_broken.transpose(1, 2).reshape(n * S, N)
        r0 = last_tile_rows(n * S)
        a[r0:] = b[r0:]
        return a.view(n, S, N).transpose(1, 2).contiguous()
    a, b = out.view(-1, ref.shape[-1]), ref_broken.reshape(-1, ref.shape[-1])
    r0 = last_tile_rows(a.shape[0])
    a[r0:] = b[r0:]
    return out


# ------------------------------------------------------------------------------------------------ GroupNorm at a large mean, bf16, two more routes
GN_ROUTE_MEAN = (10.0, 30.0)   # |group mean| of the conv output in units of its std (~1)


def gn_route_inputs():
    """A conv3x3 on (2, 48 x 48, 320) whose bias puts every group's mean at +-(10 .. 30) std of the conv's output: the input of the GroupNorm
    routes that keep raw fp32 (sum, sum of squares) across the ABI -- statistics from the conv's epilogue (gn= partials) and groupnorm_sharded."""
    n, H, W, C = 2, 48, 48, 320
    g = G(29)
    lo, hi = GN_ROUTE_MEAN
    mean = (torch.rand(32, generator=g) - 0.5).sign() * (lo + (hi - lo) * torch.rand(32, generator=g))
    return I(n=n, H=H, W=W, C=C, x=(torch.randn(n, H * W, C, generator=g)).to(BF16), w=(torch.randn(C, C, 3, 3, generator=g) * (9 * C) ** -0.5).to(BF16),
             b=mean.repeat_interleave(C // 32) + 0.1 * torch.randn(C, generator=g), gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.2))


def gn_route_ref(y, gamma, beta):
    """float64 GroupNorm(32) of the conv's STORED output y (n, S, C)."""
    return F.group_norm(d(y).transpose(1, 2), 32, d(gamma), d(beta), 1e-5).transpose(1, 2)


def gn_raw_sum_emulation(y, gamma, beta, chunk=64):
    """Plain-torch GroupNorm of bf16 y (n, S, C) from RAW fp32 (sum, sum of squares): per-chunk fp32 sums over `chunk` rows (the epilogue's
    partials cover 64 rows), added in fp32, var = E[x^2] - mean^2 in fp32. Returns the bf16 output."""
    n, S, C = y.shape
    yf = y.float().view(n, S, 32, C // 32)
    s, q = torch.zeros(n, 32), torch.zeros(n, 32)
    for r0 in range(0, S, chunk):
        blk = yf[:, r0:r0 + chunk]
        s, q = s + blk.sum((1, 3), dtype=F32), q + (blk * blk).sum((1, 3), dtype=F32)
    cnt = float(S * (C // 32))
    m = s / cnt
    rstd = torch.rsqrt(q / cnt - m * m + 1e-5)
    return (((yf - m[:, None, :, None]) * rstd[:, None, :, None]).reshape(n, S, C) * gamma.float() + beta.float()).to(BF16)


def make_cases(st):
    """The case table, its bounds and the st-dependent helpers for storage type st (torch.float16 / torch.bfloat16) -> namespace."""
    ST = st
    B_BOUNDS = B_BOUNDS_F16 if st is F16 else B_BOUNDS_BF16
    LN_BOUNDS = {} if st is F16 else LN_BOUNDS_BF16
    CASES = []


    def add(*a, **k):
        CASES.append(Case(*a, **k))


    # ---- bounds ----
    def check(spec, out, ref, name=""):
        """One output against its float64 reference. Returns (ok, figures) where figures is a dict for the profile file / failure message."""
        kind = spec[0]
        out_c = out.detach().cpu()
        ref = ref.detach().cpu().double()
        if tuple(out_c.shape) != tuple(ref.shape):
            return False, {"shape": f"{tuple(out_c.shape)} vs {tuple(ref.shape)}"}
        if kind == "X":
            want = ref.to(F32).to(spec[1]) if spec[1] is not F32 else ref.to(F32)
            ok = out_c.dtype == want.dtype and torch.equal(out_c, want)
            return ok, {"bitwise": ok, "differing": int((out_c != want).sum()) if out_c.dtype == want.dtype else -1}
        o = out_c.double()
        if kind == "AINF":   # outputs above the fp16 range: inf exactly where the rounded reference is inf, bound A on the rest, no NaN
            want_inf = torch.isinf(ref.to(F32).to(F16))
            if torch.isnan(o).any() or not torch.equal(torch.isinf(o), want_inf):
                return False, {"nan": int(torch.isnan(o).sum()), "inf_mismatch": int((torch.isinf(o) != want_inf).sum())}
            keep = ~want_inf
            ok, fig = check(("A", F16), out_c[keep], ref[keep], name)
            fig["inf"] = int(want_inf.sum())
            return ok, fig
        if not torch.isfinite(o).all():
            return False, {"nonfinite": int((~torch.isfinite(o)).sum())}
        err = (o - ref).abs()
        rms = ref.pow(2).mean().sqrt().item()
        if kind == "A":
            dtype = spec[1]
            if out_c.dtype != dtype:
                return False, {"dtype": str(out_c.dtype)}
            u = _unit(dtype)
            tol = 1.25 * u * ref.abs() + 0.25 * u * rms
            worst = (err / tol).max().item()
            floor = rel_l2(ref.to(F32).to(dtype), ref)
            r = rel_l2(o, ref)
            return (worst <= 1.0 and r <= 1.5 * floor), {"elem": worst, "elem_bound": 1.0, "rel_l2": r, "rel_l2_bound": 1.5 * floor, "bad": int((err > tol).sum())}
        if kind == "F32":
            if out_c.dtype != F32:
                return False, {"dtype": str(out_c.dtype)}
            tol = 2e-5 * ref.abs() + 2e-5 * rms
            worst = (err / tol).max().item()
            return worst <= 1.0, {"elem": worst, "elem_bound": 1.0, "rel_l2": rel_l2(o, ref), "bad": int((err > tol).sum())}
        if kind == "B":
            if out_c.dtype != ST:
                return False, {"dtype": str(out_c.dtype)}
            r = rel_l2(o, ref)
            measured, bound = B_BOUNDS.get(spec[1], (None, None))
            return (bound is not None and r <= bound), {"rel_l2": r, "rel_l2_bound": bound, "measured": measured}
        raise ValueError(spec)


    def out_dtype(spec):
        if spec[0] in ("A", "X"):
            return spec[1]
        return F32 if spec[0] in ("F32", "TE32") else ST   # AINF, B, LN: the storage type


    def storage_cast(spec, ref):
        """What a perfect kernel would store: the reference rounded once to the output's type (E.1)."""
        t = ref.to(F32)
        return t if out_dtype(spec) is F32 else t.to(out_dtype(spec))


    def wrong_type_cast(spec, ref):
        """A broken output of the fp16 table (E.2): the reference rounded to bf16 where fp16 (or fp32) is due, returned in the output's dtype so that
        only the values differ (the LayerNorm-fold bound, 2e-3 |ref| + 2.5e-3 rms, rejects it too: a bf16 rounding is up to 2^-8 = 3.9e-3 relative).
        Where bf16 IS due (the alt_cols_from V block) the broken output is bf16 with the last mantissa bit cut: one bit short of what is due."""
        b = ref.to(F32).to(BF16)
        if out_dtype(spec) is BF16:
            b = (b.view(torch.int16) & ~1).view(BF16)
        return b if out_dtype(spec) is BF16 else b.to(F32).to(out_dtype(spec))


    def truncate_cast(spec, ref):
        """A broken bf16 output: the reference rounded TOWARD ZERO to bf16 (a store that drops the low 16 bits of the fp32 value)."""
        assert out_dtype(spec) is BF16
        return (ref.to(F32).contiguous().view(torch.int32) & ~0xFFFF).view(F32).to(BF16)


    def bitcut_cast(spec, ref):
        """A broken bf16 output: the correctly rounded value with its last mantissa bit cut (a store one bit short)."""
        assert out_dtype(spec) is BF16
        return (ref.to(F32).to(BF16).contiguous().view(torch.int16) & ~1).view(BF16)


    def close_tol(ref):
        """tests/test_kernels_gpu.py: close(), the bf16 suite's general tolerance: 1.6e-2 |ref| + 2e-2 rms."""
        return 1.6e-2 * ref.abs() + 2e-2 * ref.pow(2).mean().sqrt().item()


    def check_ln_fold(out, ref, key=None):
        """LayerNorm fold at |mean| >> std. fp16: the bf16 suite holds these rows to |err| <= 1.6e-2 |ref| + 2e-2 rms (tests/test_kernels_gpu.py:
        close()); scaled by the ulp ratio 2^-3 of the two storage types: 2e-3 |ref| + 2.5e-3 rms, every element. bf16: the worst element in units
        of bound A's tolerance against LN_BOUNDS[key] = (measured on the MI355X, measured + 25 %), and every element inside close() itself."""
        o, ref = out.detach().cpu().double(), ref.detach().cpu().double()
        if out.dtype != ST or not torch.isfinite(o).all():
            return False, {"dtype": str(out.dtype)}
        rms = ref.pow(2).mean().sqrt().item()
        err = (o - ref).abs()
        if ST is F16:
            tol = 2e-3 * ref.abs() + 2.5e-3 * rms
            worst = (err / tol).max().item()
            return worst <= 1.0, {"elem": worst, "elem_bound": 1.0, "rel_l2": rel_l2(o, ref)}
        u = _unit(ST)
        worst = (err / (1.25 * u * ref.abs() + 0.25 * u * rms)).max().item()
        cap = (err / close_tol(ref)).max().item()
        measured, bound = LN_BOUNDS.get(key, (None, None))
        return (bound is not None and worst <= bound and cap <= 1.0), {"elem": worst, "elem_bound": bound, "measured": measured, "close": cap, "rel_l2": rel_l2(o, ref)}


    def check_te32(out, ref):
        o, ref = out.detach().cpu().double(), ref.detach().cpu().double()
        worst = (o - ref).abs().max().item()
        return out.dtype == F32 and worst <= 1e-5, {"abs": worst, "abs_bound": 1e-5}


    def check_any(spec, out, ref, name=""):
        """name: "<case>[<output index>]", the key of a measured LN bound."""
        if spec[0] == "LN":
            return check_ln_fold(out, ref, name)
        if spec[0] == "TE32":
            return check_te32(out, ref)
        return check(spec, out, ref, name)


    # ---- helpers that depend on the storage type ----
    def r16(g, *shape, scale=1.0, shift=0.0, dtype=ST):
        return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


    def v_bits(v_bf16):
        """bf16 V values as the bits the library is handed (a tensor of the storage type)."""
        return v_bf16.view(ST)


    def folded(w, gamma):
        """The weight values of a pack with a folded LayerNorm: w * gamma rounded to the storage type with the pack's own fp32 arithmetic
        (ops._finish_pack)."""
        return (w.float() * gamma.float()[None, :]).to(ST)


    def ln_fold_ref(x, w, b, gamma, beta, eps=1e-5):
        """LayerNorm(x) @ W^T + b as the folded GEMM is handed it: normalised rows (float64) times the ROUNDED gamma-scaled weight, plus W beta + b."""
        x = d(x)
        xn = (x - x.mean(1, keepdim=True)) / (x.var(1, unbiased=False, keepdim=True) + eps).sqrt()
        return xn @ d(folded(w, gamma)).t() + (d(w) @ d(beta) + d(b))


    # ------------------------------------------------------------------------------------------------ GEMM family
    def _linear(M, N, K, f32, kpad=0):
        """kpad: the activation buffer is K + kpad wide (the ABI wants K % 64 == 0; the weight's K is zero-padded by the pack, the buffer's pad columns
        hold finite garbage that those zeros must cancel)."""
        def build():
            g = G(M + N + K)
            return I(x=r16(g, M, K + kpad), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N))

        def ref(i):
            return [d(i.x[:, :K]) @ d(i.w).t() + d(i.b)]

        def run(ops, i):
            return [ops.linear(i.x, ops.pack_linear(i.w, i.b), out_f32=f32)]

        def dround(i):   # a double-rounding epilogue: the product rounded to 16 bits BEFORE the bias is added
            return [d((d(i.x[:, :K]) @ d(i.w).t()).to(F32).to(ST)) + d(i.b)]
        add(f"linear_{M}x{N}x{K}" + ("_f32" if f32 else ""), build, ref, run, [("F32",) if f32 else ("A", ST)], tiles=True, kbreak=drop_k(),
            dround=None if f32 else dround)


    for _f32 in (False, True):
        _linear(300, 320, 320, _f32)       # ragged M
        _linear(1000, 4, 576, _f32)        # N = 4
        _linear(128, 128, 64, _f32)        # minimum K
        _linear(257, 960, 2432, _f32)      # N not a multiple of the 320 tile, long K
        _linear(200, 192, 352, _f32, kpad=32)   # K % 64 == 32


    def _identity():
        K = 128

        def build():
            if ST is F16:
                return I(x=torch.eye(K, dtype=ST), w=(torch.arange(256 * K, dtype=F32).reshape(256, K) % 2039 - 1019).div(1024).to(ST))   # 11 significant bits: exact in fp16, not in bf16
            return I(x=torch.eye(K, dtype=ST), w=(torch.arange(256 * K, dtype=F32).reshape(256, K) % 251 - 125).div(128).to(ST))   # 7 significant bits: exact in bf16
        add("linear_identity_asymmetric_w", build, lambda i: [d(i.w).t().contiguous()], lambda ops, i: [ops.linear(i.x, ops.pack_linear(i.w, None), out_f32=True)],
            [("X", F32)], tiles=True)


    _identity()


    def _full_epilogue():
        M, N, K, rpv = 600, 320, 640, 100

        def build():
            g = G(11)
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N), rv=r32(g, M // rpv, N), r1=r16(g, M, N), r2=r16(g, M, N), rv2=r32(g, M // rpv, N))

        def ref(i):
            return [0.3 * (d(i.x) @ d(i.w).t() + d(i.b) + d(i.rv).repeat_interleave(rpv, 0) + d(i.r1)) + 0.7 * (d(i.r2) + d(i.rv2).repeat_interleave(rpv, 0))]

        def run(ops, i):
            return [ops.linear(i.x, ops.pack_linear(i.w, i.b), rowvec=i.rv, rows_per_vec=rpv, res1=i.r1, res2=i.r2, alpha=0.3, beta=0.7, rowvec2=i.rv2)]

        def dround(i):   # the product rounded to 16 bits before bias, row vector and residuals are added
            mm = d((d(i.x) @ d(i.w).t()).to(F32).to(ST))
            return [0.3 * (mm + d(i.b) + d(i.rv).repeat_interleave(rpv, 0) + d(i.r1)) + 0.7 * (d(i.r2) + d(i.rv2).repeat_interleave(rpv, 0))]
        add("linear_full_epilogue", build, ref, run, [("A", ST)], tiles=True, kbreak=drop_k(), dround=dround)


    _full_epilogue()


    def _strided():
        M, N, K = 260, 320, 320

        def build():
            g = G(12)
            return I(big=r16(g, M, 3 * K), w=r16(g, N, K, scale=K ** -0.5))

        def ref(i):
            return [torch.cat([torch.zeros(M, N, dtype=F64), d(i.big[:, K:2 * K]) @ d(i.w).t()], 1)]

        def run(ops, i):
            buf = ops.torch.zeros(M, 2 * N, dtype=ST, device=i.big.device)   # (inside guarded(ops): an arena)
            ops.linear(i.big[:, K:2 * K], ops.pack_linear(i.w, None), out=buf[:, N:])
            assert not buf[:, :N].any(), "the columns outside the output block must stay 0, bit for bit"
            return [buf]
        add("linear_strided_a_and_out", build, ref, run, [("A", ST)], tiles=True, kbreak=drop_k())


    _strided()


    def _gelu():
        M, N, K = 300, 320, 320

        def build():
            g = G(13)
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N))
        add("linear_act_gelu", build, lambda i: [gelu64(d(i.x) @ d(i.w).t() + d(i.b))],
            lambda ops, i: [ops.linear(i.x, ops.pack_linear(i.w, i.b), act="gelu")], [("A", ST)], tiles=True, kbreak=drop_k())


    _gelu()


    def _two_source():
        M, C1, C2, N = 300, 640, 320, 320

        def build():
            g = G(14)
            return I(a=r16(g, M, C1), b2=r16(g, M, C2), w=r16(g, N, C1 + C2, scale=(C1 + C2) ** -0.5), b=r32(g, N))
        add("linear_two_source_concat", build, lambda i: [torch.cat([d(i.a), d(i.b2)], 1) @ d(i.w).t() + d(i.b)],
            lambda ops, i: [ops.linear(i.a, ops.pack_linear(i.w, i.b), x2=i.b2)], [("A", ST)], tiles=True, kbreak=drop_k())


    _two_source()


    def _alt_qkv(C, M):
        """The workload's q|k|v projection (modules/attention.py, video_attention.py): folded LayerNorm, V block (columns >= 2C) written as bf16."""
        def build():
            g = G(C + M)
            return I(x=r16(g, M, C, shift=0.3), w=r16(g, 3 * C, C, scale=C ** -0.5), b=r32(g, 3 * C), gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.3))

        def ref(i):
            y = ln_fold_ref(i.x, i.w, i.b, i.gamma, i.beta)
            return [y[:, :2 * C].contiguous(), y[:, 2 * C:].contiguous()]

        def run(ops, i):
            y = ops.linear(i.x, rehome_pack(ops.pack_linear(i.w, i.b, ln=Norm(i.gamma, i.beta))), ln=ops.rowstats(i.x), alt_cols_from=2 * C)
            return [y[:, :2 * C].contiguous(), y[:, 2 * C:].contiguous().view(BF16)]
        add(f"alt_qkv_lnfold_C{C}_M{M}", build, ref, run, [("A", ST), ("A", BF16)], tiles=True, kbreak=drop_k())


    def _qkv_lnfold(C, M):
        """The same projection without alt_cols_from (bf16 build: V is a bf16 column block like q and k)."""
        def build():
            g = G(C + M)
            return I(x=r16(g, M, C, shift=0.3), w=r16(g, 3 * C, C, scale=C ** -0.5), b=r32(g, 3 * C), gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.3))
        add(f"qkv_lnfold_C{C}_M{M}", build, lambda i: [ln_fold_ref(i.x, i.w, i.b, i.gamma, i.beta)],
            lambda ops, i: [ops.linear(i.x, rehome_pack(ops.pack_linear(i.w, i.b, ln=Norm(i.gamma, i.beta))), ln=ops.rowstats(i.x))], [("A", ST)], tiles=True, kbreak=drop_k())


    for _C in (320, 640):
        for _M in (300, 4173):
            if ST is F16:     # alt_cols_from exists in the fp16 build only
                _alt_qkv(_C, _M)
            else:
                _qkv_lnfold(_C, _M)


    def _alt_boundary(at_end):
        M, N, K = 300, 320, 320
        a = N - 32 if at_end else 32

        def build():
            g = G(15 + a)
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N))

        def ref(i):
            y = d(i.x) @ d(i.w).t() + d(i.b)
            return [y[:, :a].contiguous(), y[:, a:].contiguous()]

        def run(ops, i):
            y = ops.linear(i.x, ops.pack_linear(i.w, i.b), alt_cols_from=a)
            return [y[:, :a].contiguous(), y[:, a:].contiguous().view(BF16)]
        add(f"alt_boundary_{a}_of_{N}", build, ref, run, [("A", ST), ("A", BF16)], tiles=True, kbreak=drop_k())


    if ST is F16:
        _alt_boundary(False)
        _alt_boundary(True)


    def _geglu(M, C, fold):
        def build():
            g = G(M + C)
            i = I(x=r16(g, M, C, shift=0.3 if fold else 0.0), w=r16(g, 8 * C, C, scale=C ** -0.5), b=r32(g, 8 * C))
            if fold:
                i.update(gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.3))
            return i

        def ref(i):
            h = ln_fold_ref(i.x, i.w, i.b, i.gamma, i.beta) if fold else d(i.x) @ d(i.w).t() + d(i.b)
            a, gt = h.chunk(2, dim=-1)
            return [a * gelu64(gt)]

        def run(ops, i):
            if fold:
                return [ops.linear(i.x, rehome_pack(ops.pack_geglu(i.w, i.b, ln=Norm(i.gamma, i.beta))), ln=ops.rowstats(i.x))]
            return [ops.linear(i.x, ops.pack_geglu(i.w, i.b))]
        add(("geglu_lnfold" if fold else "geglu") + f"_{M}x{C}", build, ref, run, [("A", ST)], tiles=True, kbreak=drop_k())


    _geglu(200, 64, False)
    _geglu(460, 320, False)
    _geglu(600, 320, True)


    def _linear_vt(n, S, C):
        def build():
            g = G(n + S + C)
            return I(x=r16(g, n * S, C), w=r16(g, C, C, scale=C ** -0.5))
        add(f"linear_vt_{n}x{S}x{C}", build, lambda i: [(d(i.x) @ d(i.w).t()).view(n, S, C).transpose(1, 2).contiguous()],
            lambda ops, i: [ops.linear_vt(i.x, ops.pack_linear(i.w, None), S)], [("A", ST)], tiles=True, kbreak=drop_k(), trans=True)


    _linear_vt(3, 144, 320)
    _linear_vt(5, 16, 64)


    def _conv3x3(name, n, H, W, Cin, Cout, stride=1, ups=1, asym=False, epi=False):
        def build():
            g = G(n + H + W + Cin + Cout + stride + ups)
            i = I(x=r16(g, n, H * W, Cin), w=r16(g, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5), b=r32(g, Cout))
            if epi:
                i.update(rv=r32(g, n, Cout), r1=r16(g, n, H * W, Cout))
            return i

        def ref(i):
            y = conv3x3_ref(i.x, i.w, i.b, n, H, W, stride, ups, asym)
            return [y + d(i.rv)[:, None, :] + d(i.r1) if epi else y]

        def run(ops, i):
            kw = dict(rowvec=i.rv, res1=i.r1) if epi else {}
            return [ops.conv3x3(i.x, ops.pack_conv3x3(i.w, i.b), n, H, W, stride=stride, ups=ups, asym_pad=asym, **kw)[0]]
        add(name, build, ref, run, [("A", ST)], tiles=True, kbreak=drop_k())


    _conv3x3("conv3x3_2x9x16_64to320", 2, 9, 16, 64, 320)
    _conv3x3("conv3x3_stride2", 2, 18, 32, 128, 64, stride=2)
    _conv3x3("conv3x3_asym_pad", 2, 18, 32, 128, 64, stride=2, asym=True)
    _conv3x3("conv3x3_ups2", 2, 9, 16, 192, 128, ups=2)
    _conv3x3("conv3x3_rowvec_res1", 4, 9, 16, 128, 192, epi=True)


    def _conv_in_pad8():
        n, H, W = 2, 9, 16

        def build():
            g = G(16)
            return I(x8=r16(g, n, 8, H, W).float(), w=r16(g, 320, 8, 3, 3, scale=72 ** -0.5), b=r32(g, 320))

        def kbreak(i):   # the 8 real channels sit at the START of the one 64-channel slab: drop the last 4 of them at tap (2, 2)
            j = I(i)
            j["w"] = i.w.clone()
            j["w"][:, -4:, 2, 2] = 0
            return j
        add("conv3x3_in_pad8", build, lambda i: [nchw2tok(F.conv2d(d(i.x8), d(i.w), d(i.b), padding=1))],
            lambda ops, i: [ops.conv3x3(ops.nchw_to_tokens(i.x8, 64), ops.pack_conv3x3(i.w, i.b, cin_pad=64), n, H, W)[0]], [("A", ST)], tiles=True, kbreak=kbreak)


    _conv_in_pad8()


    def _conv_t3(B, T, S, C, blend):
        def build():
            g = G(B + T + S + C + blend)
            return I(x=r16(g, B * T, S, C), w=r16(g, C, C, 3, 1, 1, scale=(3 * C) ** -0.5), b=r32(g, C), rv=r32(g, B * T, C))

        def ref(i):
            y = conv_t3_ref(i.x, i.w, i.b, B, T, S)
            return [0.3 * y + d(i.x) if blend else y + d(i.rv)[:, None, :]]

        def run(ops, i):
            pw = ops.pack_conv_t3(i.w, i.b)
            return [ops.conv_t3(i.x, pw, T, S, res2=i.x, alpha=0.3, beta=1.0) if blend else ops.conv_t3(i.x, pw, T, S, rowvec=i.rv)]
        add(f"conv_t3_{B}x{T}x{S}x{C}" + ("_blend" if blend else ""), build, ref, run, [("A", ST)], tiles=True, kbreak=drop_k())


    _conv_t3(2, 25, 24, 64, False)
    _conv_t3(2, 5, 16, 128, False)
    _conv_t3(2, 5, 16, 128, True)


    # ---- split-K (no tile forcing: the rule only runs on the launcher's own choice) ----
    def _splitk_dense():
        M, N, K = 4032, 1280, 5120

        def build():
            g = G(17)
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N), r1=r16(g, M, N), r2=r16(g, M, N))

        def ref(i):
            y = d(i.x) @ d(i.w).t() + d(i.b)
            return [0.6 * (y + d(i.r1)) + 0.4 * d(i.r2), y]

        def run(ops, i):
            pw = ops.pack_linear(i.w, i.b)
            return [ops.linear(i.x, pw, res1=i.r1, res2=i.r2, alpha=0.6, beta=0.4), ops.linear(i.x, pw, out_f32=True)]
        add("splitk_dense_4032x1280x5120", build, ref, run, [("A", ST), ("F32",)], kbreak=drop_k(), group="splitk")


    def _splitk_conv():
        n, H, W, C = 50, 9, 16, 1280

        def build():
            g = G(18)
            return I(x=r16(g, n, H * W, C), w=r16(g, C, C, 3, 3, scale=(9 * C) ** -0.5), b=r32(g, C), rv=r32(g, n, C))

        def ref(i):
            y = conv3x3_ref(i.x, i.w, i.b, n, H, W)
            return [y + d(i.rv)[:, None, :], y]

        def run(ops, i):
            pw = ops.pack_conv3x3(i.w, i.b)
            return [ops.conv3x3(i.x, pw, n, H, W, rowvec=i.rv)[0], ops.conv3x3(i.x, pw, n, H, W, out_f32=True)[0]]
        add("splitk_conv3x3_50x9x16x1280", build, ref, run, [("A", ST), ("F32",)], kbreak=drop_k(), group="splitk")


    _splitk_dense()
    _splitk_conv()


    # ---- fused FeedForward (bound B: the hidden activation is rounded to fp16 inside the kernel, and in the two-kernel form) ----
    def _ff(M, ln, mode):
        C, H, S = 320, 1280, 100

        def build():
            g = G(M + ln + len(mode))
            i = I(x=r16(g, M, C), w1=r16(g, 2 * H, C, scale=C ** -0.5), b1=r32(g, 2 * H, scale=0.5), w2=r16(g, C, H, scale=H ** -0.5), b2=r32(g, C),
                  xm=r16(g, M, C), rv2=r32(g, (M + S - 1) // S, C))
            if ln:
                i.update(gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.1))
            return i

        def ref(i):
            h = ln_fold_ref(i.x, i.w1, i.b1, i.gamma, i.beta) if ln else d(i.x) @ d(i.w1).t() + d(i.b1)
            a, gt = h.chunk(2, dim=1)
            y = d((a * gelu64(gt)).to(F32).to(ST)) @ d(i.w2).t() + d(i.b2)   # the hidden activation as both kernel forms store it
            if mode == "res":
                y = y + d(i.x)
            elif mode == "blend":
                y = 0.4 * (y + d(i.x)) + 0.6 * (d(i.xm) + d(i.rv2).repeat_interleave(S, 0)[:M])
            return [y, y]

        def run(ops, i):
            pin = rehome_pack(ops.pack_geglu(i.w1, i.b1, ln=Norm(i.gamma, i.beta) if ln else None))
            st = ops.rowstats(i.x) if ln else None
            kw = {} if mode == "plain" else (dict(res1=i.x) if mode == "res" else dict(res1=i.x, alpha=0.4, res2=i.xm, rowvec2=i.rv2, beta=0.6, rows_per_vec=S))
            return [ops.ff_fused(i.x, pin, rehome_pack(ops.pack_ff_out(i.w2, i.b2)), ln=st, **kw), ops.linear(ops.linear(i.x, pin, ln=st), ops.pack_linear(i.w2, i.b2), **kw)]
        key = f"ff_{M}_{'ln' if ln else 'noln'}_{mode}"
        add(key, build, ref, run, [("B", key + "/fused"), ("B", key + "/two_kernel")], group="ff")


    for _M in (128, 1000, 4173):
        for _ln in (False, True):
            for _mode in ("plain", "res", "blend"):
                _ff(_M, _ln, _mode)


    # ---- LayerNorm fold at a large |mean| / std (bf16 suite: test_linear_layernorm_fold_large_mean_over_std) ----
    def _lnfold_ratio(ratio, C):
        M, N = 700, 640

        def build():
            g = G(5 + int(ratio) + C)
            sign = (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1).float()
            return I(x=(torch.randn(M, C, generator=g) + ratio * sign).to(ST), w=r16(g, N, C, scale=C ** -0.5), b=r32(g, N),
                     gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.3))

        def run(ops, i):   # the row sums from both producers of the product path: the read-only pass and a GEMM epilogue (identity weight)
            pw = rehome_pack(ops.pack_linear(i.w, i.b, ln=Norm(i.gamma, i.beta)))
            x2, st = ops.linear(i.x, ops.pack_linear(torch.eye(C), None), emit_stats=True)
            assert torch.equal(x2, i.x)
            return [ops.linear(i.x, pw, ln=ops.rowstats(i.x)), ops.linear(x2, pw, ln=st)]

        def ref(i):
            y = ln_fold_ref(i.x, i.w, i.b, i.gamma, i.beta)
            return [y, y]
        add(f"lnfold_mean_over_std_{int(ratio)}_C{C}", build, ref, run, [("LN",), ("LN",)], kbreak=drop_k(), group="lnfold")


    for _r in (8.0, 60.0):
        for _C in (320, 1280):
            _lnfold_ratio(_r, _C)


    # ------------------------------------------------------------------------------------------------ normalisation
    def _groupnorm(n, S, C, fpg, silu, eps=1e-5):
        def build():
            g = G(n + S + C + fpg)
            return I(x=r16(g, n, S, C, scale=1.5, shift=0.7), gamma=r32(g, C, shift=1.0), beta=r32(g, C))

        def ref(i):
            xg = d(i.x).view(n // fpg, fpg * S, C).permute(0, 2, 1)
            y = F.group_norm(xg, 32, d(i.gamma), d(i.beta), eps)
            return [(F.silu(y) if silu else y).permute(0, 2, 1).reshape(n, S, C)]
        add(f"groupnorm_{n}x{S}x{C}_fpg{fpg}" + ("_silu" if silu else ""), build, ref,
            lambda ops, i: [ops.groupnorm(i.x, i.gamma, i.beta, eps, silu, frames_per_group=fpg)], [("A", ST)], group="norm")


    _groupnorm(4, 144, 320, 1, True)
    _groupnorm(6, 100, 64, 1, False, 1e-6)
    _groupnorm(6, 64, 192, 3, True)


    def _groupnorm_cat(n, S, C1, C2, silu):
        def build():
            g = G(n + S + C1 + C2)
            return I(a=r16(g, n, S, C1, shift=0.5), b=r16(g, n, S, C2, scale=2.0), gamma=r32(g, C1 + C2, shift=1.0), beta=r32(g, C1 + C2))

        def ref(i):
            y = F.group_norm(torch.cat([d(i.a), d(i.b)], 2).transpose(1, 2), 32, d(i.gamma), d(i.beta), 1e-5).transpose(1, 2)
            return [F.silu(y) if silu else y]
        add(f"groupnorm_cat_{n}x{S}x{C1}+{C2}", build, ref, lambda ops, i: [ops.groupnorm_cat(i.a, i.b, i.gamma, i.beta, 1e-5, silu)], [("A", ST)], group="norm")


    _groupnorm_cat(3, 144, 640, 320, True)
    _groupnorm_cat(2, 100, 64, 128, False)


    def _groupnorm_large_mean():
        n, S, C = 2, 2304, 320

        def build():
            g = G(5)
            mean = 30.0 * (torch.rand(n, 1, 32, 1, generator=g) - 0.5).sign() * (0.5 + torch.rand(n, 1, 32, 1, generator=g))
            return I(x=(torch.randn(n, S, 32, C // 32, generator=g) + mean).reshape(n, S, C).to(ST), gamma=r32(g, C, shift=1.0), beta=r32(g, C))
        # |mean| = 15..45 std: raw fp32 (sum, sum of squares) lose 8-11 bits in E[x^2] - mean^2 and leave rstd off by ~1.4e-3, which an fp16 output
        # shows (measured with raw sums: worst element 3.08 x the A.1 tolerance, 2385 of 1 474 560 elements out). The fp16 build's one-call norms
        # therefore take their sums about the group's first element (norm.hip: PIVOT); this case holds them to bound A. The bf16 build keeps raw
        # sums: 1.4e-3 is a third of its unit roundoff, and the case holds it to bound A all the same (measured: 0.750 x, profiles/bf16_kernel_parity.txt).
        add("groupnorm_large_mean", build, lambda i: [F.group_norm(d(i.x).transpose(1, 2), 32, d(i.gamma), d(i.beta), 1e-5).transpose(1, 2)],
            lambda ops, i: [ops.groupnorm(i.x, i.gamma, i.beta, 1e-5, False)], [("A", ST)], group="norm")


    _groupnorm_large_mean()


    def _layernorm(rows, C):
        rpv = 50

        def build():
            g = G(rows + C)
            return I(x=r16(g, rows, C, scale=2.0, shift=0.3), gamma=r32(g, C, shift=1.0), beta=r32(g, C), av=r32(g, (rows + rpv - 1) // rpv, C))

        def ref(i):
            # sum_out: the fp32 sum x + addvec (one fp32 rounding, as the kernel forms it) rounded to fp16; the norm reads that sum
            u = (i.x.float() + i.av.float().repeat_interleave(rpv, 0)[:rows]).to(ST)
            return [F.layer_norm(d(i.x), (C,), d(i.gamma), d(i.beta), 1e-5), d(u), F.layer_norm(d(u), (C,), d(i.gamma), d(i.beta), 1e-5)]

        def run(ops, i):
            y2, s2 = ops.layernorm(i.x, i.gamma, i.beta, addvec=i.av, rows_per_vec=rpv, want_sum=True)
            return [ops.layernorm(i.x, i.gamma, i.beta), s2, y2]
        add(f"layernorm_{rows}x{C}", build, ref, run, [("A", ST), ("X", ST), ("A", ST)], group="norm")


    _layernorm(257, 640)
    _layernorm(129, 1280)


    # ------------------------------------------------------------------------------------------------ layout / embedding kernels
    def _layout():
        def build():
            g = G(19)
            t = torch.tensor([0.25 * math.log(700.0), 0.0, -1.553652, 3.0, 24.0])
            return I(a=r16(g, 7, 33, 64), b=r16(g, 7, 33, 128), x=r32(g, 3, 8, 9, 16), y=r32(g, 3, 144, 4), t=t,
                     ea=r32(g, 5, 64), eb=r32(g, 5, 64), ec=r32(g, 5, 64), m=torch.tensor([1.0, 0, 0, 1, 0]), z=r32(g, 1000, scale=3.0),
                     big=torch.cat([r32(g, 500, scale=3.0), torch.tensor([65504.0, 65519.9, 65520.0, -70000.0, 1e-7, 6e-8, 2.98e-8, 0.0])]))

        def ref(i):
            tok = torch.cat([d(i.x).permute(0, 2, 3, 1).reshape(3, 144, 8), torch.zeros(3, 144, 56, dtype=F64)], -1)
            half = 160
            freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / half)
            args = d(i.t)[:, None] * freqs[None]
            emb = torch.cat([torch.cos(args), torch.sin(args)], -1)
            e = d(i.ea) * d(i.m)[:, None] + d(i.eb) * (1 - d(i.m)[:, None]) + d(i.ec)
            return [torch.cat([d(i.a), d(i.b)], -1), tok, d(i.y).view(3, 9, 16, 4).permute(0, 3, 1, 2).contiguous(), emb, emb, F.silu(e), F.silu(d(i.z)), d(i.big)]

        def run(ops, i):
            return [ops.concat_channels(i.a, i.b), ops.nchw_to_tokens(i.x, 64), ops.tokens_to_nchw(i.y, 3, 4, 9, 16), ops.timestep_embedding(i.t, 320),
                    ops.timestep_embedding(i.t, 320, out_f32=True), ops.emb_combine(i.ea, i.eb, i.ec, i.m)[1], ops.silu_to_bf16(i.z), ops.cast_to_bf16(i.big)]
        # timestep embedding: fp32 sin / cos of arguments up to 24 with a fp32 frequency table: |error| ~ 24 * 2^-24 * a few ulp of the table -> the fp32
        # form is held to 1e-5 absolute (TE32), the 16-bit form to bound A's absolute term on rms ~0.7 (8.6e-5) plus its rounding
        add("layout_and_embedding", build, ref, run, [("X", ST), ("X", ST), ("X", F32), ("A", ST), ("TE32",), ("A", ST), ("A", ST), ("X", ST)], group="layout")


    _layout()


    # ------------------------------------------------------------------------------------------------ attention (bound B)
    def _qkv(g, rows, C, qk_scale):
        q, k = r16(g, rows, C, scale=qk_scale), r16(g, rows, C, scale=qk_scale)
        v = r16(g, rows, C, dtype=BF16)
        return q, k, v


    def attn_ref(q, k, v, zero_base=False, first_tile_base=False):
        """softmax(q k^T) v per head in float64 with the kernel's internal roundings emulated: the probabilities are rounded to bf16 against the
        kernel's base, the row sum is that of the rounded probabilities, V is the bf16 input. q, k, v: (..., S, 64) float64, q scaled so that a score
        is the base-2 exponent. The base:
          default          the row maximum (the temporal kernel; spatial rows that one key dominates or that fit one key tile);
          zero_base        the pre-scaled query form: base 0, i.e. bf16(2^score), where the row maximum lies within +-60 octaves;
          first_tile_base  the general spatial kernel (csrc/attention.hip, attn_spatial_body): the maximum of the row's FIRST 64-key tile; a later
                           tile re-bases only when 32 of its probabilities sum to more than 2^11. The reference asserts that none exceeds 2^6, so
                           the kernel keeps that base for the whole row (diffuse rows: later maxima exceed the first tile's by a few octaves)."""
        s = q @ k.transpose(-1, -2)
        m = s[..., :64].amax(-1, keepdim=True) if first_tile_base else s.amax(-1, keepdim=True)
        if zero_base:
            m = torch.where(m.abs() <= 60.0, torch.zeros_like(m), m)
        e = s - m
        if first_tile_base:
            assert e.max().item() < 6.0, "a later key tile would re-base the online softmax: not a diffuse-row case"
        p = torch.exp2(e).to(F32).to(BF16).double()
        return (p @ v) / p.sum(-1, keepdim=True)


    def _spiky(g, S, gain):
        q, k, v = _qkv(g, S, 64, 1.0)
        for j, row in enumerate(range(70, S, 197)):
            k[row] = q[(37 * j + 5) % S] * gain
        k[:64] = -q[300] * gain
        k[S - 1] = q[300] * gain
        q[11] = 0
        return q, k, v


    def _attn_edge(key, S, log2, maker):
        c = 64 ** -0.5 * LOG2E

        def build():
            q, k, v = maker(G(S + log2))
            q = q.float().clamp(-60000, 60000).to(ST)
            k = k.float().clamp(-60000, 60000).to(ST)
            if log2:
                q = (q.float() * c).to(ST)
            return I(qkv=torch.cat([q, k, v_bits(v)], 1).contiguous())

        def ref(i):
            t = i.qkv.cpu()
            q, k, v = d(t[:, :64]), d(t[:, 64:128]), d(t[:, 128:].contiguous().view(BF16))
            return [attn_ref(q if log2 else q * c, k, v, zero_base=log2)]

        def run(ops, i):
            return [ops.attn_spatial(i.qkv[:, :64], i.qkv[:, 64:128], i.qkv[:, 128:], 1, 1, S, v_rows=True, q_log2=log2)]
        add(key, build, ref, run, [("B", key)], group="attn")


    _attn_edge("attn_zero_base_gain12", 512, True, lambda g: _spiky(g, 512, 12.0))
    _attn_edge("attn_zero_base_gain400", 512, True, lambda g: _spiky(g, 512, 400.0))
    _attn_edge("attn_max_free_fallback_gain60", 512, False, lambda g: _spiky(g, 512, 60.0))


    def _spike_rescale(g):
        q, k, v = _qkv(g, 512, 64, 1.0)
        k[300] = q[7] * 4
        k[450] = q[100] * 6
        return q, k, v


    _attn_edge("attn_spike_forces_rescale", 512, False, _spike_rescale)


    def _attn_spatial(n, heads, S, log2, zero_base=False):
        """attn_spatial(v_rows=True) on random (diffuse) rows, several images and heads; q_log2: the query carries scale x log2 e. The launcher runs
        the general kernel at every shape of the table but (1, 1, 2304) pre-scaled, which is S >= 2048 in whole 256-row workgroups: the pipelined
        zero-base kernel (zero_base)."""
        C = heads * 64
        c = 64 ** -0.5 * LOG2E

        def build():
            q, k, v = _qkv(G(n + heads + S + log2), n * S, C, 1.0)
            if log2:
                q = (q.float() * c).to(ST)
            return I(qkv=torch.cat([q, k, v_bits(v)], 1).contiguous())

        def ref(i):
            t = i.qkv.cpu()
            q, k, v = (x.view(n, S, heads, 64).transpose(1, 2) for x in (d(t[:, :C]), d(t[:, C:2 * C]), d(t[:, 2 * C:].contiguous().view(BF16))))
            return [attn_ref(q if log2 else q * c, k, v, zero_base=zero_base, first_tile_base=not zero_base).transpose(1, 2).reshape(n * S, C)]
        key = f"attn_spatial_{n}x{heads}x{S}" + ("_log2" if log2 else "")
        add(key, build, ref, lambda ops, i: [ops.attn_spatial(i.qkv[:, :C], i.qkv[:, C:2 * C], i.qkv[:, 2 * C:], n, heads, S, v_rows=True, q_log2=log2)],
            [("B", key)], group="attn")


    for _shape in ((2, 5, 144), (2, 3, 200), (1, 2, 576), (1, 1, 2120), (1, 3, 4104)):
        for _log2 in (False, True):
            _attn_spatial(*_shape, _log2)
    _attn_spatial(1, 1, 2304, True, zero_base=True)


    def _attn_temporal(B, T, S, heads):
        C = heads * 64
        c = 64 ** -0.5 * LOG2E

        def build():
            g = G(B + T + S + heads)
            q, k, v = _qkv(g, B * T * S, C, 1.0)
            return I(qkv=torch.cat([q, k, v_bits(v)], 1).contiguous())

        def ref(i):
            t = i.qkv.cpu()
            q, k, v = (x.view(B, T, S, heads, 64).permute(0, 2, 3, 1, 4) for x in (d(t[:, :C]), d(t[:, C:2 * C]), d(t[:, 2 * C:].contiguous().view(BF16))))
            return [attn_ref(q * c, k, v).permute(0, 3, 1, 2, 4).reshape(B * T * S, C)]
        key = f"attn_temporal_{B}x{T}x{S}x{heads}"
        add(key, build, ref, lambda ops, i: [ops.attn_temporal(i.qkv, B, T, S, heads)], [("B", key)], group="attn")


    _attn_temporal(2, 25, 40, 5)
    _attn_temporal(2, 7, 9, 1)
    _attn_temporal(1, 32, 16, 3)


    # ------------------------------------------------------------------------------------------------ fp16 range
    def _subnormal_weights():
        """Weights at scale 2e-4: about a quarter are fp16 subnormals (|w| < 2^-14 = 6.1e-5). fp32 output, so the only error of a correct kernel is fp32
        accumulation; an MFMA that flushed subnormal inputs would lose those products (error ~1e-1)."""
        M, N, K = 300, 320, 320

        def build():
            g = G(20)
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=2e-4))
        add("subnormal_weights_f32", build, lambda i: [d(i.x) @ d(i.w).t()], lambda ops, i: [ops.linear(i.x, ops.pack_linear(i.w, None), out_f32=True)],
            [("F32",)], kbreak=drop_k(), group="range")


    def _overflow():
        """A bias of 7e4 on columns 64..127 puts that block above 65504 (+-8 around 7e4: far from the rounding threshold 65520, so the ulp below
        the threshold is empty and inf / finite is unambiguous); the other columns are ordinary."""
        M, N, K = 300, 320, 320

        def build():
            g = G(21)
            b = r32(g, N)
            b[64:128] += 7e4
            b[128:130] -= 7e4
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=b)
        add("overflow_above_fp16_range", build, lambda i: [d(i.x) @ d(i.w).t() + d(i.b)], lambda ops, i: [ops.linear(i.x, ops.pack_linear(i.w, i.b))],
            [("AINF",)], tiles=True, kbreak=drop_k(), group="range")


    if ST is F16:     # fp16's subnormal range and its 65504 ceiling: nothing of the kind in bf16 at these magnitudes
        _subnormal_weights()
        _overflow()



    # ------------------------------------------------------------------------------------------------ launch-geometry edges (both builds)
    # Temporal attention walks nprob = B * S * heads problems, four per workgroup, on a grid capped at 4096 workgroups: (1, 3, 4099, 5) has
    # nprob = 20495 -> 5124 workgroups wanted -> 2 iterations, whole workgroups idle in the second one and nprob % 4 = 3 leaves one idle wave in an
    # active workgroup. (2, 31, 5, 1): T one below the 32-frame tile.
    _attn_temporal(1, 3, 4099, 5)
    _attn_temporal(2, 31, 5, 1)

    # The elementwise / sampler kernels of elementwise.hip run a grid-stride loop on at most 4096 x 256 threads: each op at a small odd shape and at
    # the smallest listed shape whose element count exceeds 1 048 576, where the loop wraps. float64 references; fp32 outputs: bound F32; 16-bit
    # outputs: X where the kernel's fp32 arithmetic is exact before the one rounding, A otherwise.
    WRAP = 256 * 16 * 256


    def _tok(z):   # (T, c, H, W) -> (T, H*W, c)
        return z.permute(0, 2, 3, 1).reshape(z.shape[0], -1, z.shape[1])


    def _sampler_prepare(T, H, W, cpad, uc, replace):
        c_in = torch.tensor(0.37, dtype=F32).item()   # the fp32 value the ABI's float argument carries: x * c_in is then exact in float64
        def build():
            g = G(T + H * W + cpad + uc + 2 * replace)
            m = torch.tensor([1.0, 0.0, 0.25, 1.0, 0.0][:T])
            return I(x=r32(g, T, 4, H, W, scale=3.0), cf=r32(g, T, 4, H, W), m=m, uc=r32(g, T, 4, H, W), cc=r32(g, T, 4, H, W))

        def ref(i):
            m = d(i.m).view(-1, 1, 1, 1)
            xr = d(i.x) * (1 - m) + d(i.cf) * m if replace else d(i.x)
            z = torch.zeros(T, H * W, cpad - 8, dtype=F64)
            top = torch.cat([_tok(xr * c_in), _tok(d(i.uc)) if uc else torch.zeros(T, H * W, 4, dtype=F64), z], -1)
            bot = torch.cat([_tok(xr * c_in), _tok(d(i.cc)), z], -1)
            return [torch.cat([top, bot], 0), xr]

        def run(ops, i):
            x = scratch(i.x, "x") if replace else i.x   # vk_sampler_prepare writes x with `replace` only: without, the embedded input is held unchanged
            net_in = ops.sampler_prepare(x, i.cf if replace else None, i.m if replace else None, i.uc if uc else None, i.cc, cpad, c_in, replace)
            return [net_in, x]
        # replace off: x * c_in is one exact product rounded once to fp32 and once more to 16 bits, as the reference's cast chain does: bitwise
        add(f"sampler_prepare_{T}x{H * W}x{cpad}" + ("_uc" if uc else "") + ("_replace" if replace else ""), build, ref, run,
            [("A", ST) if replace else ("X", ST), ("F32",) if replace else ("X", F32)], group="layout")


    _sampler_prepare(2, 7, 1873, 320, True, True)
    _sampler_prepare(2, 7, 1873, 320, False, False)
    for _uc in (False, True):
        for _rep in (False, True):
            _sampler_prepare(5, 11, 13, 64, _uc, _rep)
    assert 2 * 13111 * (320 // 8) > WRAP


    def _sampler_update(T, H, W, ld):
        c_out, c_skip, sig, sign = -0.9, 0.2, 3.0, 2.0

        def build():
            g = G(T + H * W + ld)
            return I(x=r32(g, T, 4, H, W, scale=3.0), net=r32(g, 2 * T, H * W, ld), s=torch.linspace(1.0, 2.5, T))

        def ref(i):
            x = d(i.x)
            untok = lambda z: z[..., :4].reshape(T, H, W, 4).permute(0, 3, 1, 2)
            du, dc = untok(d(i.net)[:T]) * c_out + x * c_skip, untok(d(i.net)[T:]) * c_out + x * c_skip
            gd = du + d(i.s).view(-1, 1, 1, 1) * (dc - du)
            return [x + (x - gd) / sig * (sign - sig)]

        def run(ops, i):
            x = scratch(i.x, "x")   # the entry point's in / out operand
            ops.sampler_update(x, i.net, i.s, c_out, c_skip, sig, sign)
            return [x]
        add(f"sampler_update_{T}x{H * W}x{ld}", build, ref, run, [("F32",)], group="layout")


    _sampler_update(29, 1, 9041, 4)
    _sampler_update(5, 11, 13, 8)
    assert 29 * 4 * 9041 > WRAP


    def _rowwise(n, chw):
        """cfg_combine, euler_step, mask_replace, denoiser_combine, scale_rows on (n, chw) rows with one scalar per row."""
        def build():
            g = G(n + chw)
            return I(x2=r32(g, 2 * n, chw), x=r32(g, n, chw, scale=3.0), y=r32(g, n, chw), s=torch.linspace(1.0, 2.5, n), sg=torch.linspace(3.0, 0.7, n),
                     sn=torch.linspace(2.0, 0.3, n), m=torch.tensor([1.0, 0.0, 0.25, 1.0, 0.0][:n]), co=r32(g, n), cs=r32(g, n))

        def ref(i):
            col = lambda v: d(v).view(-1, 1)
            x, y, x2 = d(i.x), d(i.y), d(i.x2)
            return [x2[:n] + col(i.s) * (x2[n:] - x2[:n]), x + (x - y) / col(i.sg) * (col(i.sn) - col(i.sg)), x * (1 - col(i.m)) + y * col(i.m),
                    y * col(i.co) + x * col(i.cs), x * col(i.co)]

        def run(ops, i):
            return [ops.cfg_combine(i.x2, i.s), ops.euler_step(i.x, i.y, i.sg, i.sn), ops.mask_replace(i.x, i.y, i.m), ops.denoiser_combine(i.y, i.x, i.co, i.cs),
                    ops.scale_rows(i.x, i.co)]
        add(f"rowwise_elementwise_{n}x{chw}", build, ref, run, [("F32",)] * 5, group="layout")


    _rowwise(3, 349531)
    _rowwise(5, 577)
    assert 3 * 349531 > WRAP


    def _layout_wrap():
        n_cast, HW1, HW2, rows = WRAP + 7, 11 * 3973, 230 * 380, 43691
        assert 3 * HW1 * 8 > WRAP and 3 * 4 * HW2 > WRAP and rows * (64 + 128) // 8 > WRAP

        def build():
            g = G(23)
            return I(z=r32(g, n_cast, scale=3.0), x=r32(g, 3, 8, 11, 3973), y=r32(g, 3, HW2, 8), a=r16(g, rows, 64), b=r16(g, rows, 128))

        def ref(i):
            tok = torch.cat([_tok(d(i.x)), torch.zeros(3, HW1, 56, dtype=F64)], -1)
            return [F.silu(d(i.z)), d(i.z), tok, d(i.y)[..., :4].reshape(3, 230, 380, 4).permute(0, 3, 1, 2).contiguous(), torch.cat([d(i.a), d(i.b)], -1)]

        def run(ops, i):
            return [ops.silu_to_bf16(i.z), ops.cast_to_bf16(i.z), ops.nchw_to_tokens(i.x, 64), ops.tokens_to_nchw(i.y, 3, 4, 230, 380), ops.concat_channels(i.a, i.b)]
        add("layout_past_the_grid_stride_wrap", build, ref, run, [("A", ST), ("X", ST), ("X", ST), ("X", F32), ("X", ST)], group="layout")


    _layout_wrap()

    if ST is BF16:
        # -------------------------------------------------------------------------------------------- bf16 build only: the V^T attention route
        def _vt_attn(n, heads, S):
            """linear_vt -> attn_spatial(vt): V^T (n, heads*64, S) from its own GEMM, then the spatial kernel that reads V^T tiles. Output 0 is the V^T
            tensor (single rounding), output 1 the attention of q, k and the ROUNDED V^T (bound B; P against the first key tile's maximum, as the
            q|k|v-rows route, whose result the bf16 suite holds bitwise equal to this one's)."""
            C = heads * 64
            c = 64 ** -0.5 * LOG2E

            def build():
                g = G(n + heads + S + 3)
                q, k, _ = _qkv(g, n * S, C, 1.0)
                return I(q=q, k=k, x=r16(g, n * S, C), wv=r16(g, C, C, scale=C ** -0.5))

            def ref(i):
                vt = (d(i.x) @ d(i.wv).t()).view(n, S, C).transpose(1, 2).contiguous()
                v = vt.to(F32).to(BF16).double().view(n, heads, 64, S).transpose(-1, -2)
                q, k = (t.view(n, S, heads, 64).transpose(1, 2) for t in (d(i.q), d(i.k)))
                return [vt, attn_ref(q * c, k, v, first_tile_base=True).transpose(1, 2).reshape(n * S, C)]

            def run(ops, i):
                vt = ops.linear_vt(i.x, ops.pack_linear(i.wv, None), S)
                return [vt, ops.attn_spatial(i.q, i.k, vt, n, heads, S)]
            key = f"vt_attn_spatial_{n}x{heads}x{S}"
            add(key, build, ref, run, [("A", BF16), ("B", key)], group="vt")

        for _shape in ((2, 5, 144), (2, 3, 200), (1, 1, 2120)):
            _vt_attn(*_shape)

        # -------------------------------------------------------------------------------------------- bf16 build only: first-stage / conditioner kernels
        def _conv3d(B, T, H, W, Cin, Cout):
            def build():
                g = G(B + T + H + W + Cin + Cout)
                return I(x=r16(g, B * T, H * W, Cin), w=r16(g, Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5), b=r32(g, Cout), r2=r16(g, B * T, H * W, Cout))

            def ref(i):
                x5 = d(i.x).view(B, T, H, W, Cin).permute(0, 4, 1, 2, 3)
                y = F.conv3d(x5, d(i.w), d(i.b), padding=1).permute(0, 2, 3, 4, 1).reshape(B * T, H * W, Cout)
                return [0.7 * y + d(i.r2), y]

            def run(ops, i):
                pw = ops.pack_conv3d(i.w, i.b)
                return [ops.conv3d(i.x, pw, T, H, W, res2=i.r2, alpha=0.7, beta=1.0), ops.conv3d(i.x, pw, T, H, W, out_f32=True)]
            add(f"conv3d_{B}x{T}x{H}x{W}_{Cin}to{Cout}", build, ref, run, [("A", ST), ("F32",)], tiles=True, cfgs=(0, 1, 2, 3), kbreak=drop_k(), group="firststage")

        for _shape in ((1, 5, 8, 16, 64, 64), (2, 3, 6, 10, 128, 192), (1, 4, 16, 24, 64, 4), (1, 1, 8, 8, 64, 128)):
            _conv3d(*_shape)

        def _softmax_rows(rows, cols):
            def build():
                g = G(rows + cols)
                big = r32(g, rows, cols + 64, scale=4.0)
                big[0, : min(cols, 5)] = 60.0   # a dominant cluster: the maximum must be subtracted
                return I(big=big)
            add(f"softmax_rows_{rows}x{cols}", build, lambda i: [torch.softmax(d(i.big[:, :cols]), -1)], lambda ops, i: [ops.softmax_rows(i.big[:, :cols])],
                [("A", ST)], group="firststage")

        for _shape in ((300, 9216), (7, 16384), (64, 36), (5, 1028)):
            _softmax_rows(*_shape)

        def _attn_small(n, heads, S, D):
            """fp32 VALU attention, one rounding at the output: the float64 reference needs no emulation; bound B as the issue groups it (the 1.5 x
            floor cap makes it a single-rounding bound in rel-L2)."""
            C = heads * D

            def build():
                return I(qkv=r16(G(n + heads + S + D), n * S, 3 * C))

            def ref(i):
                q, k, v = (d(i.qkv[:, j * C:(j + 1) * C]).view(n, S, heads, D).transpose(1, 2) for j in range(3))
                return [(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), -1) @ v).transpose(1, 2).reshape(n * S, C)]
            key = f"attn_small_{n}x{heads}x{S}x{D}"
            add(key, build, ref, lambda ops, i: [ops.attn_small(i.qkv, n, heads, S, D)], [("B", key)], group="firststage")

        for _shape in ((2, 4, 257, 80), (3, 2, 50, 64), (1, 2, 300, 128), (2, 1, 5, 80)):
            _attn_small(*_shape)

        def _gelu_mlp(M, N, K):
            def build():
                g = G(M + N + K + 1)
                return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N))
            add(f"linear_act_gelu_{M}x{N}x{K}", build, lambda i: [gelu64(d(i.x) @ d(i.w).t() + d(i.b))],
                lambda ops, i: [ops.linear(i.x, ops.pack_linear(i.w, i.b), act="gelu")], [("A", ST)], tiles=True, kbreak=drop_k(), group="firststage")

        _gelu_mlp(257, 5120, 1280)
        _gelu_mlp(100, 64, 128)

    # ------------------------------------------------------------------------------------------------ operand layouts: the narrow side of every switch
    def _operand_case(name, build, ref, call, layout=None, out_lay=None, out_shape=None, f32=False, narrow=True, cfgs=None, bitwise="stated", want=None,
                      kbreak=None):
        """call(ops, i, out) -> the ops.* result (out=None: the wrapper allocates, aligned). layout: input name -> (skew, ld) (Case.layout);
        out_lay: (skew, ld) of an output arena of out_shape. narrow: the layout knocks the launch off the pipelined kernel (forced 7 must not answer 7).
        bitwise: "stated" = asserted where same_bits_stated, "always" = asserted (the source promises it), None = printed only.
        want: forced variant -> (plan of the laid-out launch, plan of the aligned one), asserted."""
        layout = dict(layout or {})

        def run(ops, i):
            dev = i.x.device
            line = 256 if dev.type == "cuda" else 16   # (the GPU allocator hands out 256-byte aligned blocks; the CPU dry runs of the harness see 64)
            for k, (skew, ld) in layout.items():   # which side of a switch runs is a pure function of these
                assert i[k].data_ptr() % line == skew % line and (ld is None or i[k].stride(-2) == ld) and i[k].stride(-1) == 1, (k, i[k].data_ptr() % 256, i[k].stride())
            out = None
            if out_lay is not None:
                out = _guard.empty(out_shape, F32 if f32 else ST, dev, skew=out_lay[0], ld=out_lay[1], label=f"out of {name}")
                assert out.data_ptr() % line == out_lay[0] % line and out.stride() == (out_lay[1] or out_shape[1], 1), (out.data_ptr() % 256, out.stride())
            got, asked = planned(ops, lambda: call(ops, i, out))
            twin = I({k: (_guard.put(v.contiguous(), dev, label=f"aligned {k}") if k in layout else v) for k, v in i.items()})
            assert all(v.data_ptr() % line == 0 for v in twin.values() if torch.is_tensor(v))
            base, asked0 = planned(ops, lambda: call(ops, twin, None))
            stats = None
            if isinstance(got, tuple):
                (got, stats), (base, stats0) = got, base
            equal = got.shape == base.shape and torch.equal(got, base)
            differing = int((got != base).sum()) if got.shape == base.shape else -1
            apart = ((got.double() - base.double()).abs() / base.double().abs().clamp_min(1e-30)).max().item() if differing > 0 else 0.0
            print(f"OPERANDS {name} {'fp16' if ST is F16 else 'bf16'} cfg{ops.TILE_CFG} plan={asked} aligned_plan={asked0} bitwise_the_aligned_call={equal}"
                  f" differing={differing}/{got.numel()} worst_relative_gap={apart:.3g}")
            assert all(c > 0 for c in asked + asked0), (asked, asked0)
            if narrow and ops.TILE_CFG == 7:
                assert all(c // 16 not in (6, 7) for c in asked), f"{name}: planned {asked} on a kernel that carries only the 16-byte epilogue"
            if want is not None and ops.TILE_CFG in want:
                assert (asked[-1], asked0[-1]) == want[ops.TILE_CFG], (asked, asked0, want[ops.TILE_CFG])
            if bitwise == "always" or (bitwise == "stated" and len(asked) == len(asked0) and all(same_bits_stated(a, b) for a, b in zip(asked, asked0))):
                assert equal, f"{name}: {int((got != base).sum())} elements differ from the aligned call (plans {asked} / {asked0})"
            if stats is not None:
                worst = stats_follow_the_output(stats, got)
                print(f"OPERANDS {name} rowstats worst/tol={worst:.3g} slabs_bitwise_the_aligned_call={stats.t.shape == stats0.t.shape and torch.equal(stats.t, stats0.t)}")
                assert worst <= 1.0 and stats.M == got.shape[0], worst
            return [got]
        add(name, build, ref, run, [("F32",) if f32 else ("A", ST)], tiles=True, kbreak=kbreak or drop_k(), cfgs=cfgs, layout=layout)


    def _operand_cases():
        M, N, K, rpv = 260, 320, 192, 130       # (rows_per_vec >= 128: a 256-row tile spans at most 3 images, so the ALIGNED call stays on the staged epilogue)
        SK, LD = 8, N + 4                      # 8 bytes past a 16-byte boundary; rows of N + 4 elements: every second row 8 bytes off

        def build():
            g = G(61)
            return I(x=r16(g, M, K), w=r16(g, N, K, scale=K ** -0.5), b=r32(g, N), r1=r16(g, M, N), r2=r16(g, M, N), rv=r32(g, M // rpv, N), rv2=r32(g, M // rpv, N))

        def y(i):
            return d(i.x) @ d(i.w).t() + d(i.b)

        def plain(ops, i, out):
            return ops.linear(i.x, ops.pack_linear(i.w, i.b), out=out)

        def with_res1(ops, i, out):
            return ops.linear(i.x, ops.pack_linear(i.w, i.b), res1=i.r1, out=out)

        def with_res2(ops, i, out):
            return ops.linear(i.x, ops.pack_linear(i.w, i.b), res2=i.r2, alpha=0.3, beta=0.7, out=out)

        def full(ops, i, out):
            return ops.linear(i.x, ops.pack_linear(i.w, i.b), rowvec=i.rv, rows_per_vec=rpv, res1=i.r1, res2=i.r2, alpha=0.3, beta=0.7, rowvec2=i.rv2, out=out)

        def full_ref(i):
            return [0.3 * (y(i) + d(i.rv).repeat_interleave(rpv, 0) + d(i.r1)) + 0.7 * (d(i.r2) + d(i.rv2).repeat_interleave(rpv, 0))]
        seven = {7: (4 * 16 + 1, 7 * 16 + 1)}   # the pipelined kernel declines the narrow operand: the sixteen-wave kernel, general epilogue
        _operand_case("operand_out_skew8", build, lambda i: [y(i)], plain, out_lay=(SK, None), out_shape=(M, N), want=seven)
        _operand_case("operand_out_ldc_plus4", build, lambda i: [y(i)], plain, out_lay=(0, LD), out_shape=(M, N), want=seven)
        _operand_case("operand_res1_skew8", build, lambda i: [y(i) + d(i.r1)], with_res1, layout={"r1": (SK, None)}, want=seven)
        _operand_case("operand_res1_ld_plus4", build, lambda i: [y(i) + d(i.r1)], with_res1, layout={"r1": (0, LD)}, want=seven)
        _operand_case("operand_res2_skew8", build, lambda i: [0.3 * y(i) + 0.7 * d(i.r2)], with_res2, layout={"r2": (SK, None)}, want=seven)
        _operand_case("operand_res2_ld_plus4", build, lambda i: [0.3 * y(i) + 0.7 * d(i.r2)], with_res2, layout={"r2": (0, LD)}, want=seven)
        # (this case found the two epilogue bodies one fp32 bit apart in the fp16 build -- the compiler's contraction of alpha * u + beta * t, per
        #  instantiation: 13 / 14 of the 83200 outputs one fp16 ulp apart; the blend is now written with an explicit fmaf in every body, csrc/gemm_common.h)
        _operand_case("operand_full_epilogue_out_skew8", build, full_ref, full, out_lay=(SK, None), out_shape=(M, N), want=seven)
        _operand_case("operand_emit_stats_out_skew8", build, lambda i: [y(i)], lambda ops, i, out: ops.linear(i.x, ops.pack_linear(i.w, i.b), emit_stats=True, out=out),
                      out_lay=(SK, None), out_shape=(M, N))
        _operand_case("operand_f32_out_ldc_plus4", build, lambda i: [y(i)], lambda ops, i, out: ops.linear(i.x, ops.pack_linear(i.w, i.b), out_f32=True, out=out),
                      out_lay=(0, LD), out_shape=(M, N), f32=True, narrow=False)
        _operand_case("operand_act_gelu_out_skew8", build, lambda i: [gelu64(y(i))], lambda ops, i, out: ops.linear(i.x, ops.pack_linear(i.w, i.b), act="gelu", out=out),
                      out_lay=(SK, None), out_shape=(M, N), want=seven)
        # the L2-prefetch switch of the pipelined kernel (csrc/gemm_pipe.hip: A 128-byte aligned with lda % 64 == 0, K >= 3 K-steps, one round of tiles):
        # the activations 16 bytes off the line in rows of K + 8 elements against the aligned call -- "bitwise the same results either way"
        _operand_case("operand_a_off_the_128_byte_line", build, lambda i: [y(i)], plain, layout={"x": (16, K + 8)}, narrow=False, bitwise="always",
                      want={7: (7 * 16 + 1, 7 * 16 + 1)})

        # LayerNorm-folded q|k|v and GEGLU at width 320 (N = 960 / 2560: whole 320-column tiles, so that the pipelined kernel is what the operand loses)
        C = 320

        def build_c(geglu):
            def build():
                g = G(62 + geglu)
                return I(x=r16(g, M, C, shift=0.3), w=r16(g, (8 if geglu else 3) * C, C, scale=C ** -0.5), b=r32(g, (8 if geglu else 3) * C),
                         gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.3))
            return build

        def qkv(ops, i, out):
            return ops.linear(i.x, rehome_pack(ops.pack_linear(i.w, i.b, ln=Norm(i.gamma, i.beta))), ln=ops.rowstats(i.x), out=out)

        def geglu_ref(i):
            a, gt = (d(i.x) @ d(i.w).t() + d(i.b)).chunk(2, dim=-1)
            return [a * gelu64(gt)]
        _operand_case("operand_qkv_lnfold_out_skew8", build_c(0), lambda i: [ln_fold_ref(i.x, i.w, i.b, i.gamma, i.beta)], qkv, out_lay=(SK, None), out_shape=(M, 3 * C))
        _operand_case("operand_geglu_out_skew8", build_c(1), geglu_ref, lambda ops, i, out: ops.linear(i.x, ops.pack_geglu(i.w, i.b), out=out),
                      out_lay=(SK, None), out_shape=(M, 4 * C))

        # the implicit-GEMM convolutions: out and res1 both 8 bytes off
        n, H, W, Cin = 2, 9, 16, 64

        def build_conv():
            g = G(64)
            return I(x=r16(g, n, H * W, Cin), w=r16(g, N, Cin, 3, 3, scale=(9 * Cin) ** -0.5), b=r32(g, N), r1=r16(g, n * H * W, N))

        def conv(ops, i, out):
            return ops.conv3x3(i.x, ops.pack_conv3x3(i.w, i.b), n, H, W, res1=i.r1, out=out)[0].view(n * H * W, N)
        _operand_case("operand_conv3x3_out_res1_skew8", build_conv, lambda i: [conv3x3_ref(i.x, i.w, i.b, n, H, W).reshape(n * H * W, N) + d(i.r1)], conv,
                      layout={"r1": (SK, None)}, out_lay=(SK, None), out_shape=(n * H * W, N))
        B, T, S = 1, 3, 144

        def build_t3():
            g = G(65)
            return I(x=r16(g, B * T, S, Cin), w=r16(g, N, Cin, 3, 1, 1, scale=(3 * Cin) ** -0.5), b=r32(g, N), r1=r16(g, B * T * S, N))

        def conv_t(ops, i, out):
            return ops.conv_t3(i.x, ops.pack_conv_t3(i.w, i.b), T, S, res1=i.r1, out=out).view(B * T * S, N)
        def drop_centre_tap(i):   # (one clip: the last tile's rows are the last frame, whose tap 2 reads zero padding -- drop 32 of K from the centre tap)
            j = I(i)
            j["w"] = i.w.clone()
            j["w"][:, -32:, 1] = 0
            return j
        _operand_case("operand_conv_t3_out_res1_skew8", build_t3, lambda i: [conv_t3_ref(i.x, i.w, i.b, B, T, S).reshape(B * T * S, N) + d(i.r1)], conv_t,
                      layout={"r1": (SK, None)}, out_lay=(SK, None), out_shape=(B * T * S, N), kbreak=drop_centre_tap)

        # the streaming kernel's decline at its smallest forced shape (K = 320, N = 320): A 16-byte aligned but off the 128-byte line, out 8 bytes off --
        # forced variant 6 must fall back to a tiled kernel
        def build_s():
            g = G(66)
            return I(x=r16(g, M, C), w=r16(g, N, C, scale=C ** -0.5), b=r32(g, N))
        _operand_case("operand_stream_declines_out_skew8", build_s, lambda i: [d(i.x) @ d(i.w).t() + d(i.b)], plain, layout={"x": (16, None)}, out_lay=(SK, None),
                      out_shape=(M, N), cfgs=(6,), narrow=False, bitwise=None, want={6: (1 * 16 + 1, 6 * 16 + 1)})


    _operand_cases()

    BY_NAME = {c.name: c for c in CASES}
    assert len(BY_NAME) == len(CASES)
    return types.SimpleNamespace(ST=ST, CASES=CASES, BY_NAME=BY_NAME, B_BOUNDS=B_BOUNDS, LN_BOUNDS=LN_BOUNDS, check=check, check_any=check_any,
                                 check_ln_fold=check_ln_fold, check_te32=check_te32, out_dtype=out_dtype, storage_cast=storage_cast,
                                 wrong_type_cast=wrong_type_cast, truncate_cast=truncate_cast, bitcut_cast=bitcut_cast, close_tol=close_tol, r16=r16,
                                 v_bits=v_bits, folded=folded, ln_fold_ref=ln_fold_ref, attn_ref=attn_ref)
