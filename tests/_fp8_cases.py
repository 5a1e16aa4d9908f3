"""Case table and bounds of the fp8 (OCP e4m3, BASELINE config 5) kernel parity suite: what tests/test_fp8_kernels_gpu.py runs under
ops.storage(torch.bfloat16) and tests/test_fp8_bounds_cpu.py proves to bite. Same shape as tests/_kernel_cases.py, whose helpers and bounds A, F32
are imported through tests/_bf16_cases.py, not copied.

A case is (build, ref64, run):
  build()            CPU tensors from a seeded generator. Every fp8 operand is built here as e4m3 BYTES plus its scales (fp32 per row / per image
                     group / per output channel, or E8M0 bytes per 32-element block);
  ref64(inputs)      plain torch in float64 on the DEQUANTISED values -> list of outputs;
  run(ops, inputs)   the ops.* call on the GPU copies of the inputs -> list of outputs (a quantised output is a tuple, see Q / MX below).
Weights: build() keeps the fp32 weight `w` AND quantises it with the pack's own arithmetic (ops._finish_pack_fp8: scale = amax / 448 per output
channel in fp32, codes = e4m3(w / scale)) into `w8` / `w_scale`, which the reference dequantises; run() hands `w` to ops.pack_*_fp8 and asserts
that the pack's own wt and scale ARE those codes and scales, bit for bit (_verify_pack): the reference reads the very values the kernel is handed.

Scales are spread so that a wrong index cannot hide: activation rows x logspace(-2, 2, M) before quantisation, weight rows x logspace(-1, 1, N),
MX block scales drawn from 119..133, convolution image-group scales logspace(-2, 0, groups).

Bounds (derived from the number formats, never taken from the code under test):
  A, F32  tests/_kernel_cases.py (u = 2^-8): bf16 / fp32 outputs of the GEMMs, the convolutions and the V block of the mx8 projection. The fp32
          outputs of linear_fp8: F32 plus the summation error of the fp8 MFMA as a probe of the instruction alone measures it (MFMA_EPS below).
  Q       quantised output with a float scale, out = (codes uint8, scale fp32): quantize_rows (scale within 1e-6 relative of float64 amax / 448,
          an all-zero row gives exactly 1), layernorm_quant (2e-5), groupnorm_fp8 (the scale bounds the data and is at most 8 x -- 16 x with a
          concat -- the true maximum: a bound by design). Codes under the kernel's OWN scale s: t = ref64 / s clamped to +-448, every code c finite
          and |c - t| <= ulp8(t) / 2 + slack, ulp8(t) = 2^(max(floor(log2 |t|), -6) - 3); slack = 2^-21 |t| (two fp32 roundings in x * (1 / s), 4 x
          margin), for the two norms plus the F32 bound of the pre-quantisation value in code units, (2e-5 |y| + 2e-5 rms(y)) / s.
  MX      MX output, out = (codes uint8 (M, C), E8M0 bytes (M, >= C / 32)[, value]): per 32-column block the scale byte must be the tightest,
          e_ref = ceil(log2(amax64 / 448)), raised by one if amax64 / 2^e_ref >= 448; e_ref +- 1 is accepted only where amax64 / 448 lies within
          1e-4 relative of a power of two (such blocks are counted: "near"). Codes under the kernel's own e: the half-ulp rule with the F32 bound
          in code units as slack (GEGLU on the fp8 GEMM: plus the MFMA term of MFMA_EPS carried through a * gelu(g), the reference's `slack`).
          With a third element `value` (attention mx_out: the bf16 output of the same kernel on the same operands) the codes and scales are
          judged against THAT value with slack 2^-21 |t|; pad scale bytes must be 127. The kernel quantises its fp32 o / l, not the bf16 value
          (attention.hip: mx_quant_block_attn on oacc * inv). The check cannot tell the two apart and holds for both: rounding to bf16 is
          monotone and every e4m3 midpoint is a bf16 number, so the code of the fp32 value lies within half an e4m3 step of the bf16 value
          too; only a block whose maximum the bf16 rounding lifts onto a power of two x 448 may differ in exponent, and those are `near`.
  B       attn_spatial_fp8qk, bf16 output: rel-L2 against the emulating float64 reference, measured on the MI355X in one run + 25 %
          (B_BOUNDS_FP8, profiles/fp8_kernel_parity.txt), never above 1.5 x the rel-L2 of that reference rounded once to bf16.

Attention reference (csrc/attention.hip, attn_spatial_fp8qk_kernel): P is rounded to bf16 against a base, the row sum is that of the rounded P, V
is the bf16 input. <false> instantiations (a `scale`, or scale = 0 below S = 4096): the base is the maximum of the row's FIRST 64-key tile
(rebase() at t == 0); a later tile re-bases every row of its wave (32 QW consecutive query rows) on max(base, tile maximum) when the 32
probabilities of one lane (the keys of the tile whose bit 3 equals the lane half) sum to more than 2^11. tests/_kernel_cases.py: attn_ref
(first_tile_base) asserts that no such re-base happens, which logits of standard deviation 3 do not grant, so attn_rebased below emulates the
re-base as the kernel's code shows it. <true> (scale = 0, S >= 4096): base 0 where the first tile's maximum lies within +-60 -- attn_ref(zero_base).
"""
import math
import os
import types

import torch
import torch.nn.functional as F

from tests import _bf16_cases as bc
from tests import _parity_bodies as pb
from tests._guard import rehome_pack
from tests._bf16_cases import (BF16, F32, F64, LOG2E, Case, G, I, Norm, attn_ref, bitcut_cast, check, conv3x3_ref, conv_t3_ref, d,  # noqa: F401
                               drop_k, gelu64, last_tile_rows, ln_fold_ref, r16, r32, rel_l2, splice_last_tile, storage_cast, to_device, truncate_cast)

TAG = "FP8PARITY"
_TAGGED = types.SimpleNamespace(TAG=TAG)   # what pb.check_stats needs of a case module: its print tag
T = bc.T                      # the storage type of every non-fp8 operand: bf16 (tests/_parity_bodies.py keys its reference cache by T.ST)
E4M3, U8 = torch.float8_e4m3fn, torch.uint8
DENSE_CFGS, GEGLU_CFGS = (0, 1, 3, 4), (0, 1, 3)   # csrc/gemm_fp8.hip: fp8_cfg() maps every other value to these; GEGLU maps 4 to 3
GROUPS = {"dense": 12, "geglu": 4, "amx": 6, "conv": 8, "quant": 17, "mx8": 2, "attn": 15}

# attn_spatial_fp8qk, bf16 output: name -> (rel-L2 measured on the MI355X against the emulating float64 reference, that + 25 %), from ONE run of
# tests/test_fp8_kernels_gpu.py (profiles/fp8_kernel_parity.txt); never filled from a second run of the kernel on its own output
B_BOUNDS_FP8 = {
    "fp8_attn_2x5x144_scale": (1.519e-03, 1.899e-03),
    "fp8_attn_2x5x144_pre": (1.470e-03, 1.837e-03),
    "fp8_attn_2x3x200_scale": (1.555e-03, 1.944e-03),
    "fp8_attn_2x3x200_pre": (1.497e-03, 1.871e-03),
    "fp8_attn_1x1x2120_scale": (1.589e-03, 1.986e-03),
    "fp8_attn_1x1x2120_pre": (1.557e-03, 1.946e-03),
    "fp8_attn_1x2x4104_scale": (1.608e-03, 2.010e-03),
    "fp8_attn_1x2x4104_pre": (1.581e-03, 1.976e-03),
    "fp8_attn_1x1x4096_scale": (1.612e-03, 2.015e-03),
    "fp8_attn_1x1x4096_pre": (1.591e-03, 1.989e-03),
}

# The fp32 outputs of linear_fp8 miss F32 (2e-5 |ref| + 2e-5 rms) at every shape, worst element 5 .. 16 x the tolerance, alike under every tile.
# The miss does NOT grow with K (6.8 x at K = 16, 15.6 x at K = 144, 12.3 x at K = 2432), so it is not adopted from the kernel's own figures:
# tools/probes/fp8_mfma_sum_probe.py measures v_mfma_scale_f32_32x32x64_f8f6f4 ALONE (one wave, the accumulator chained through K / 64
# instructions, nothing else) against float64 on operands drawn as this table draws them (profiles/fp8_mfma_sum_probe.txt). The instruction's
# error is a fraction of the magnitude of the products it sums, so the bound of an fp32 output of the fp8 GEMM is
#     |out - ref| <= 2e-5 |ref| + 2e-5 rms + MFMA_EPS[1] * sum_k |a_k w_k|      (the sum in float64, scales applied: `sumabs` of the reference),
# ONE constant for every case and K: MFMA_EPS = (the probe's worst |D - ref| / sum_k |a_k b_k| over all its K, that + 25 %). The worst is that
# of K = 16, where sum |a w| is smallest; at long K an element sits well inside it (K = 2432: 1 / 14 of it), so the output as a whole is held
# to the probe as well: rel-L2 <= MFMA_REL[1] = the probe's worst rel-L2 (9.4e-6 at K = 16 rising to 1.49e-5 at K = 2432) + 25 %. The probe's
# rel-L2 per K and the kernel's lie within 13 % of each other on different random draws (K = 16: 9.38e-6 / 9.26e-6, K = 144: 1.35e-5 / 1.52e-5,
# K = 2432: 1.493e-5 / 1.487e-5; profiles/fp8_kernel_parity.txt): the miss is the instruction's, not the kernel's.
MFMA_EPS = (4.003e-05, 5.004e-05)
MFMA_REL = (1.493e-05, 1.866e-05)


# ------------------------------------------------------------------------------------------------ e4m3 / E8M0 helpers
def q8(t):
    """float -> e4m3 bytes, round to nearest even, saturating at +-448 (the cast itself yields NaN above 448)."""
    return t.to(F32).clamp(-448.0, 448.0).to(E4M3).view(U8)


def deq8(u):
    return u.view(E4M3).double()


def mx_deq(u, s):
    """e4m3 bytes (M, C) x 2^(s - 127) per 32 consecutive columns, s (M, C / 32) E8M0 bytes -> float64."""
    return deq8(u) * torch.exp2(s.double() - 127.0).repeat_interleave(32, -1)


def quant_channels(w):
    """The pack's arithmetic (ops._finish_pack_fp8) on a weight of any rank: one fp32 scale amax / 448 per output channel (dim 0)."""
    w2 = w.float().reshape(w.shape[0], -1)
    sc = (w2.abs().amax(1).clamp_min(1e-12) / 448.0).float()
    return q8(w2 / sc[:, None]).view(w.shape), sc


def ulp8(t):
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -30))).clamp_min(-6.0) - 3.0)


def toward_zero8(t):
    """A broken quantiser: t (already in code units) rounded TOWARD ZERO to the e4m3 grid."""
    t = t.double().clamp(-448.0, 448.0)
    u = ulp8(t)
    return q8(torch.sign(t) * torch.floor(t.abs() / u) * u)


def mx_e_ref(r):
    """r (M, C) float64 -> (e_ref (M, C / 32), near (M, C / 32) bool): the tightest power-of-two block exponent and the blocks where
    amax / 448 lies within 1e-4 relative of a power of two."""
    amax = r.reshape(r.shape[0], -1, 32).abs().amax(2)
    frac = (amax / 448.0).clamp_min(2.0 ** -200)
    e = torch.ceil(torch.log2(frac))
    e = torch.where(amax / torch.exp2(e) >= 448.0, e + 1, e)
    e = torch.where(amax == 0, torch.full_like(e, -127.0), e).clamp(-127.0, 127.0)
    near = ((frac / torch.exp2(torch.round(torch.log2(frac))) - 1.0).abs() <= 1e-4) & (amax > 0)
    return e, near


def mx_quant(r, shift=0):
    """The reference quantised to MX with round-to-nearest at e_ref + shift -> (codes, E8M0 bytes)."""
    e = mx_e_ref(r)[0] + shift
    return q8(r / torch.exp2(e).repeat_interleave(32, 1)), (e + 127.0).to(U8)


def _codes_fig(c, t, slack):
    t = t.clamp(-448.0, 448.0)
    ratio = (c - t).abs() / (ulp8(t) / 2 + slack)
    return ratio.max().item(), int((ratio > 1.0).sum())


def _f32_slack(r):
    return 2e-5 * r.abs() + 2e-5 * r.pow(2).mean().sqrt().item()


def check_q(spec, out, ref):
    codes, s = out
    s = s.detach().cpu().double().reshape(-1)
    if codes.dtype != U8 or out[1].dtype != F32:
        return False, {"dtype": f"{codes.dtype}/{out[1].dtype}"}
    r = ref.detach().cpu().double().reshape(s.numel(), -1)
    c = deq8(codes.detach().cpu().contiguous()).reshape(s.numel(), -1)
    if c.shape != r.shape or not torch.isfinite(c).all() or not torch.isfinite(s).all() or not (s > 0).all():
        return False, {"shape": f"{tuple(c.shape)} vs {tuple(r.shape)}", "nonfinite": int((~torch.isfinite(c)).sum())}
    amax = r.abs().amax(1)
    mode = spec[1]
    if mode in ("rows", "ln"):
        want = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
        serr = torch.where(amax == 0, (s != 1.0).double(), (s - want).abs() / want).max().item()   # an all-zero row: exactly 1
        sbound = 1e-6 if mode == "rows" else 2e-5
    else:           # groupnorm_fp8: the scale bounds the data and is at most spec[2] x the true maximum (+ 0.3 absolute), by design
        lo = (amax * 0.999 / (s * 448.0)).max().item()
        hi = (s * 448.0 / (amax * spec[2] + 0.3)).max().item()
        serr, sbound = max(lo, hi), 1.0
    t = r / s[:, None]
    slack = 2.0 ** -21 * t.clamp(-448.0, 448.0).abs()
    if mode != "rows":
        slack = slack + _f32_slack(r) / s[:, None]
    worst, bad = _codes_fig(c, t, slack)
    return (serr <= sbound and worst <= 1.0), {"scale": serr, "scale_bound": sbound, "code": worst, "code_bound": 1.0, "bad": bad}


def check_mx(spec, out, ref):
    codes, sc = out[0], out[1].detach().cpu()
    if codes.dtype != U8 or sc.dtype != U8:
        return False, {"dtype": f"{codes.dtype}/{sc.dtype}"}
    own = len(out) > 2      # judged against the kernel's own bf16 output of the same operands
    r = (out[2] if own else ref).detach().cpu().double().reshape(codes.shape[0], -1)
    c = deq8(codes.detach().cpu().contiguous())
    nb = r.shape[1] // 32
    if c.shape != r.shape or sc.shape[0] != r.shape[0] or sc.shape[1] < nb or not torch.isfinite(c).all():
        return False, {"shape": f"{tuple(c.shape)} vs {tuple(r.shape)}", "nonfinite": int((~torch.isfinite(c)).sum())}
    pad_ok = bool((sc[:, nb:] == 127).all())
    e = sc[:, :nb].double() - 127.0
    e_ref, near = mx_e_ref(r)
    scale_bad = int((~((e == e_ref) | (near & ((e - e_ref).abs() <= 1)))).sum())
    two_e = torch.exp2(e).repeat_interleave(32, 1)
    t = r / two_e
    extra = getattr(ref, "slack", None)     # GEGLU on the fp8 GEMM: the MFMA's summation error carried through a * gelu(g) (_geglu)
    slack = 2.0 ** -21 * t.clamp(-448.0, 448.0).abs() if own else (_f32_slack(r) + (0.0 if extra is None else extra)) / two_e
    worst, bad = _codes_fig(c, t, slack)
    return (scale_bad == 0 and pad_ok and worst <= 1.0), {"scale_bad": scale_bad, "near": int(near.sum()), "blocks": near.numel(), "pad_ok": pad_ok,
                                                           "code": worst, "code_bound": 1.0, "bad": bad}


def check_any(spec, out, ref, name=""):
    """name: "<case>[<output index>]", the key of a measured F32 replacement."""
    kind = spec[0]
    if kind == "Q":
        return check_q(spec, out, ref)
    if kind == "MX":
        return check_mx(spec, out, ref)
    if kind == "B":
        if out.dtype != BF16 or not torch.isfinite(out.float()).all():
            return False, {"dtype": str(out.dtype)}
        r = rel_l2(out.detach().cpu(), ref)
        measured, bound = B_BOUNDS_FP8.get(spec[1], (None, None))
        return (bound is not None and r <= bound), {"rel_l2": r, "rel_l2_bound": bound, "measured": measured}
    ok, fig = check(spec, out, ref, name)
    sumabs = getattr(ref, "sumabs", None)
    if kind == "F32" and sumabs is not None and "elem" in fig:   # an fp32 output of the fp8 GEMM: F32 plus the measured summation error of the MFMA
        r = ref.detach().cpu().double()
        err = (out.detach().cpu().double() - r).abs()
        fig["elem_f32"] = fig.pop("elem")                        # in units of the plain F32 tolerance, for the record
        fig["mfma"] = (err / sumabs).max().item()                # the kernel's error as a fraction of sum |a w|: the probe's unit
        fig["mfma_eps"], fig["rel_l2_bound"] = MFMA_EPS[1], MFMA_REL[1]
        tol = _f32_slack(r) + MFMA_EPS[1] * sumabs
        fig["elem"], fig["bad"] = (err / tol).max().item(), int((err > tol).sum())
        ok = fig["elem"] <= 1.0 and fig["rel_l2"] <= MFMA_REL[1]
    return ok, fig


def out_dtype(spec):
    return BF16 if spec[0] == "B" else (U8 if spec[0] in ("Q", "MX") else bc.out_dtype(spec))


def q_good(spec, ref, codes_of=q8):
    """The reference quantised with the reference scale: amax64 / 448 per row / image group in fp32 (1 for an all-zero row)."""
    n = spec[3] if spec[1] == "gn" else ref.shape[0]
    r = ref.double().reshape(n, -1)
    amax = r.abs().amax(1)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0).float()
    return codes_of(r / s.double()[:, None]).view(ref.shape), s


def perfect(spec, ref):
    """What a perfect kernel would store (E.1): the reference cast once to the output's form."""
    if spec[0] == "Q":
        return q_good(spec, ref)
    if spec[0] == "MX":
        if len(spec) > 1 and spec[1] == "own":
            v = ref.to(F32).to(BF16)
            return mx_quant(v.double()) + (v,)
        return mx_quant(ref.double())
    if spec[0] == "B":
        return ref.to(F32).to(BF16)
    return storage_cast(spec, ref)


# ------------------------------------------------------------------------------------------------ the table
CASES = []


def add(*a, **k):
    CASES.append(Case(*a, **k))


def _verify_pack(pw, codes2d, scale):
    """The pack's own wt and scale are, bit for bit, the codes and scales build() made and the float64 reference dequantises."""
    N, K = codes2d.shape
    assert torch.equal(pw.wt[:N, :K], codes2d) and not pw.wt[:N, K:].any() and torch.equal(pw.scale[:N], scale), "pack_*_fp8 != the reference's (w8, w_scale)"


def _weight(g, N, *rest, fan):
    w = torch.randn(N, *rest, generator=g) * fan ** -0.5 * torch.logspace(-1, 1, N).view(N, *([1] * len(rest)))
    w8, ws = quant_channels(w)
    return dict(w=w, w8=w8, w_scale=ws)


def deq_w(i):
    return deq8(i.w8) * d(i.w_scale).view(-1, *([1] * (i.w8.dim() - 1)))


def _rows(g, M, K):
    """Per-row quantised activations whose row scales span 4 decades -> (codes (M, K), fp32 scale (M,))."""
    x = torch.randn(M, K, generator=g) * torch.logspace(-2, 2, M)[:, None]
    sc = (x.abs().amax(1).clamp_min(1e-12) / 448.0).float()
    return q8(x / sc[:, None]), sc


def _codes(g, *shape, amp=100.0):
    return q8(torch.randn(*shape, generator=g) * amp)


def _rep(v, rpv, M):
    return d(v).repeat_interleave(rpv, 0)[:M]


# ---- group dense: linear_fp8 with per-row activation scales ----
def _A(i):
    return i.a8[:, i.c0:i.c0 + i.K]


def _dense_y(i):
    return (deq8(_A(i)) * d(i.a_scale)[:, None]) @ deq_w(i).t() + d(i.b)


def _dense_sumabs(i):
    return (deq8(_A(i)).abs() * d(i.a_scale)[:, None]) @ deq_w(i).abs().t()


def _dense_refs(i):
    """[reference of the bf16 output, reference of the fp32 output carrying `sumabs` = sum_k |a_k w_k| for the MFMA term of its bound]."""
    y = _dense_y(i)
    y32 = y.clone()
    y32.sumabs = _dense_sumabs(i)
    return [y, y32]


def _dense_y_dround(i):   # a double-rounding epilogue: the scaled product rounded to bf16 BEFORE bias and residuals are added
    return d(((deq8(_A(i)) * d(i.a_scale)[:, None]) @ deq_w(i).t()).to(F32).to(BF16)) + d(i.b)


def _pack_linear(ops, i):
    pw = ops.pack_linear_fp8(i.w, i.b)
    _verify_pack(pw, i.w8, i.w_scale)
    return pw


def _dense_inputs(seed, M, N, K, layout="plain"):
    g = G(seed)
    a8, sc = _rows(g, M, K)
    c0 = 0
    if layout == "tail":      # a view of a buffer 32 columns wider whose pad holds +-448: the K-tail mask must never read it into the product
        pad = torch.where(torch.rand(M, 32, generator=g) < 0.5, 0x7E, 0xFE).to(U8)
        a8 = torch.cat([a8, pad], 1)
    elif layout == "strided":  # the middle block of a (M, 3K) buffer of other codes
        a8, c0 = torch.cat([_codes(g, M, K), a8, _codes(g, M, K)], 1), K
    return I(a8=a8.contiguous(), a_scale=sc, c0=c0, K=K, b=r32(g, N), **_weight(g, N, K, fan=K))


def _dense(M, N, K, layout="plain"):
    def run(ops, i):
        pw = _pack_linear(ops, i)
        return [ops.linear_fp8(_A(i), i.a_scale, pw), ops.linear_fp8(_A(i), i.a_scale, pw, out_f32=True)]
    add(f"fp8_linear_{M}x{N}x{K}" + ("_ktail" if layout == "tail" else ""), lambda: _dense_inputs(M + N + K, M, N, K, layout),
        _dense_refs, run, [("A", BF16), ("F32",)], tiles=True, cfgs=DENSE_CFGS, kbreak=drop_k("w8"),
        dround=lambda i: [_dense_y_dround(i)] * 2, group="dense")


_dense(300, 320, 320)        # ragged M, K tail 64
_dense(260, 4, 320)          # N = 4
_dense(128, 128, 128)        # minimum whole tile
_dense(257, 960, 2432)       # long K
for _K in (16, 80, 112, 144, 336):
    _dense(200, 192, _K, layout="tail")   # K % 128 = 16, 80, 112, 16, 80; K < 128 and K = 16: a single, mostly masked K-step


def _dense_strided():
    M, N, K = 260, 320, 320

    def run(ops, i):
        buf = ops.torch.zeros(M, 2 * N, dtype=BF16, device=i.a8.device)   # (inside guarded(ops): an arena)
        ops.linear_fp8(_A(i), i.a_scale, _pack_linear(ops, i), out=buf[:, N:])
        assert not buf[:, :N].any(), "the columns outside the output block must stay 0, bit for bit"
        return [buf]
    add("fp8_linear_strided_a_and_out", lambda: _dense_inputs(12, M, N, K, "strided"), lambda i: [torch.cat([torch.zeros(M, N, dtype=F64), _dense_y(i)], 1)],
        run, [("A", BF16)], tiles=True, cfgs=DENSE_CFGS, kbreak=drop_k("w8"), group="dense")


_dense_strided()


def _dense_full_epilogue():
    M, N, K, rpv = 600, 320, 640, 100

    def build():
        i = _dense_inputs(11, M, N, K)
        g = G(111)
        i.update(rv=r32(g, M // rpv, N), r1=r16(g, M, N), r2=r16(g, M, N), rv2=r32(g, M // rpv, N))
        return i

    def epi(i, y):
        return 0.3 * (y + _rep(i.rv, rpv, M) + d(i.r1)) + 0.7 * (d(i.r2) + _rep(i.rv2, rpv, M))

    def run(ops, i):
        return [ops.linear_fp8(_A(i), i.a_scale, _pack_linear(ops, i), rowvec=i.rv, rows_per_vec=rpv, res1=i.r1, res2=i.r2, alpha=0.3, beta=0.7, rowvec2=i.rv2)]
    add("fp8_linear_full_epilogue", build, lambda i: [epi(i, _dense_y(i))], run, [("A", BF16)], tiles=True, cfgs=DENSE_CFGS, kbreak=drop_k("w8"),
        dround=lambda i: [epi(i, _dense_y_dround(i))], group="dense")


_dense_full_epilogue()


def _dense_stats():
    M, N, K = 300, 320, 320

    def build():
        i = _dense_inputs(13, M, N, K)
        i.update(r1=r16(G(113), M, N))
        return i

    def run(ops, i):
        out, st = ops.linear_fp8(_A(i), i.a_scale, _pack_linear(ops, i), res1=i.r1, emit_stats=True)
        assert st.M == M and st.t.shape == (st.parts, M, 2)
        pb.check_stats(_TAGGED, st, out)
        return [out]
    add("fp8_linear_emit_stats", build, lambda i: [_dense_y(i) + d(i.r1)], run, [("A", BF16)], tiles=True, cfgs=DENSE_CFGS, kbreak=drop_k("w8"), group="dense")


_dense_stats()


# ---- group geglu ----
def _geglu(M, K, nout, mx):
    def build():
        g = G(M + K + nout)
        a8, sc = _rows(g, M, K)
        return I(a8=a8, a_scale=sc, c0=0, K=K, b=r32(g, 2 * nout), **_weight(g, 2 * nout, K, fan=K))

    def ref(i):
        y = _dense_y(i)
        a, gt = y.chunk(2, dim=1)
        v = a * gelu64(gt)
        if mx:   # the quantised fp32 value a * gelu(g) inherits the error of a and g, which are fp32 outputs of the fp8 GEMM: each within
            # E = F32 + MFMA_EPS * sumabs of its float64 value (MFMA_EPS above); |gelu'| <= 1.13, so |dv| <= |gelu(g)| Ea + 1.13 |a| Eg
            ea, eg = (_f32_slack(y) + MFMA_EPS[1] * _dense_sumabs(i)).chunk(2, dim=1)
            v.slack = gelu64(gt).abs() * ea + 1.13 * a.abs() * eg
        return [v]

    def run(ops, i):
        pw = ops.pack_geglu_fp8(i.w, i.b)
        perm = ops.geglu_perm(nout).to(i.w8.device)
        _verify_pack(pw, i.w8[perm], i.w_scale[perm])
        out = ops.linear_fp8(i.a8, i.a_scale, pw, mx_out=mx)
        return [tuple(out)] if mx else [out]
    add(f"fp8_geglu_{M}x{K}x{nout}" + ("_mx_out" if mx else ""), build, ref, run, [("MX",) if mx else ("A", BF16)], tiles=True, cfgs=GEGLU_CFGS,
        kbreak=drop_k("w8"), group="geglu")


for _mx in (False, True):
    _geglu(200, 64, 256, _mx)
    _geglu(460, 320, 1280, _mx)


# ---- group amx: MX block-scaled activations, the two epilogues the network calls ----
def _amx(M, N, K, epi):
    S = 50
    ld = -(-K // 128) * 4     # the kernel reads one dword of scales per 128-byte K-step: (M, 8) for K = 160, pad bytes 127

    def build():
        g = G(M + N + K + len(epi))
        a_mx = torch.full((M, ld), 127, dtype=U8)
        a_mx[:, :K // 32] = torch.randint(119, 134, (M, K // 32), generator=g, dtype=U8)
        nv = (M + S - 1) // S
        return I(a8=_codes(g, M, K), a_mx=a_mx, K=K, b=r32(g, N), r1=r16(g, M, N, scale=1000.0), r2=r16(g, M, N, scale=1000.0), rv=r32(g, nv, N, scale=300.0),
                 **_weight(g, N, K, fan=K))

    def ref(i):
        y = mx_deq(i.a8, i.a_mx[:, :K // 32]) @ deq_w(i).t() + d(i.b)
        if epi == "blend":
            return [0.4 * (y + d(i.r1)) + 0.6 * (d(i.r2) + _rep(i.rv, S, M))]
        return [y + d(i.r1) + _rep(i.rv, S, M)]

    def run(ops, i):
        pw = _pack_linear(ops, i)
        if epi == "blend":   # FeedForward's out-projection
            return [ops.linear_fp8(i.a8, None, pw, a_mx=i.a_mx, res1=i.r1, alpha=0.4, res2=i.r2, rowvec2=i.rv, beta=0.6, rows_per_vec=S)]
        out, st = ops.linear_fp8(i.a8, None, pw, a_mx=i.a_mx, res1=i.r1, rowvec=i.rv, rows_per_vec=S, emit_stats=True)   # the attention out-projection
        pb.check_stats(_TAGGED, st, out)
        return [out]
    add(f"fp8_amx_{M}x{N}x{K}_{epi}", build, ref, run, [("A", BF16)], tiles=True, cfgs=DENSE_CFGS, kbreak=drop_k("w8"), group="amx")


for _shape in ((300, 320, 1280), (130, 64, 256), (200, 192, 160)):   # K = 160: a K tail of 32
    for _epi in ("blend", "res_rowvec_stats"):
        _amx(*_shape, _epi)


# ---- group conv: implicit-GEMM convolutions on e4m3 activations with one scale per image group (tile_cfg 0: one run each) ----
def _group_scales(n):
    return torch.logspace(-2, 0, n) if n > 1 else torch.tensor([0.03])


def _conv3x3(n, H, W, cin, cout, fps=1):
    def build():
        g = G(n + H + W + cin + cout)
        return I(a8=_codes(g, n, H * W, cin, amp=60.0), a_scale=_group_scales(n // fps), b=r32(g, cout), rv=r32(g, n, cout), r1=r16(g, n, H * W, cout),
                 **_weight(g, cout, cin, 3, 3, fan=9 * cin))

    def ref(i):
        x = deq8(i.a8) * d(i.a_scale).repeat_interleave(fps)[:, None, None]
        y = conv3x3_ref(x, deq_w(i), i.b, n, H, W)
        return [y + d(i.rv)[:, None, :], y + d(i.r1)]

    def run(ops, i):
        pw = ops.pack_conv3x3_fp8(i.w, i.b)
        _verify_pack(pw, ops._slab_major(i.w8.permute(0, 2, 3, 1).reshape(cout, 9, cin)), i.w_scale)
        return [ops.conv3x3_fp8(i.a8, i.a_scale, pw, n, H, W, frames_per_scale=fps, rowvec=i.rv),
                ops.conv3x3_fp8(i.a8, i.a_scale, pw, n, H, W, frames_per_scale=fps, res1=i.r1)]
    add(f"fp8_conv3x3_{n}x{H}x{W}_{cin}to{cout}" + (f"_fps{fps}" if fps > 1 else ""), build, ref, run, [("A", BF16)] * 2, kbreak=drop_k("w8"), group="conv")


_conv3x3(2, 6, 10, 64, 128)           # odd (slab, tap) unit count, 256x256 kernel
_conv3x3(3, 9, 16, 320, 320)          # 256x320 kernel
_conv3x3(4, 7, 9, 128, 320, fps=2)    # scale groups of 126 rows straddle tiles
_conv3x3(1, 5, 33, 64, 64)            # odd width


def _conv_t3(B, T_, S, cin, cout):
    def build():
        g = G(B + T_ + S + cin + cout)
        return I(a8=_codes(g, B * T_, S, cin, amp=60.0), a_scale=_group_scales(B), b=r32(g, cout), rv=r32(g, B * T_, cout), r2=r16(g, B * T_, S, cout),
                 **_weight(g, cout, cin, 3, 1, 1, fan=3 * cin))

    def ref(i):
        x = deq8(i.a8) * d(i.a_scale).repeat_interleave(T_)[:, None, None]
        y = conv_t3_ref(x, deq_w(i), i.b, B, T_, S)
        return [y + d(i.rv)[:, None, :], 0.7 * y + d(i.r2)]

    def run(ops, i):
        pw = ops.pack_conv_t3_fp8(i.w, i.b)
        _verify_pack(pw, ops._slab_major(i.w8[:, :, :, 0, 0].permute(0, 2, 1)), i.w_scale)
        return [ops.conv_t3_fp8(i.a8, i.a_scale, pw, T_, S, rowvec=i.rv), ops.conv_t3_fp8(i.a8, i.a_scale, pw, T_, S, alpha=0.7, res2=i.r2, beta=1.0)]

    def kbreak(i):   # the centre tap's 32-wide K run of the last slab: the last tap reads only zero padding from a clip's last frame, which is
        j = I(i)     # where the last row tile lies (all of it at T = 1), so dropping it there would change nothing
        j["w8"] = i.w8.clone()
        j["w8"][:, -32:, 1] = 0
        return j
    add(f"fp8_conv_t3_{B}x{T_}x{S}_{cin}to{cout}", build, ref, run, [("A", BF16)] * 2, kbreak=kbreak, group="conv")


_conv_t3(1, 25, 16, 64, 64)           # odd unit count
_conv_t3(2, 5, 40, 320, 320)
_conv_t3(2, 7, 33, 128, 320)
_conv_t3(3, 1, 20, 64, 64)            # T = 1: both outer taps are padding


# ---- group quant ----
def _quantize_rows(M, K):
    def build():
        big = (torch.randn(M, K + 24, generator=G(M + K)) * torch.logspace(-2, 2, M)[:, None]).to(BF16)   # rows of a strided view
        big[M // 2] = 0                                                                                  # an all-zero row must not divide by zero
        return I(big=big)
    add(f"fp8_quantize_rows_{M}x{K}", build, lambda i: [d(i.big[:, :K])], lambda ops, i: [ops.quantize_rows_fp8(i.big[:, :K])], [("Q", "rows")], group="quant")


for _shape in ((300, 320), (5, 64), (64, 5120), (257, 2432), (9, 8), (33, 72)):
    _quantize_rows(*_shape)


def _layernorm_quant(rows, C, ratio=0.0):
    def build():
        g = G(rows + C + int(ratio))
        x = torch.randn(rows, C, generator=g) * torch.logspace(-1, 1, rows)[:, None] + 0.7
        if ratio:   # |mean| / std = ratio in every row
            x = torch.randn(rows, C, generator=g) + ratio * (torch.randint(0, 2, (rows, 1), generator=g) * 2 - 1).float()
        return I(x=x.to(BF16), gamma=r32(g, C, scale=0.3, shift=1.0), beta=r32(g, C, scale=0.2))
    add(f"fp8_layernorm_quant_{rows}x{C}" + (f"_mean_over_std_{int(ratio)}" if ratio else ""), build,
        lambda i: [F.layer_norm(d(i.x), (C,), d(i.gamma), d(i.beta), 1e-5)], lambda ops, i: [ops.layernorm_quant_fp8(i.x, Norm(i.gamma, i.beta))],
        [("Q", "ln")], group="quant")


for _shape in ((257, 640), (129, 1280), (64, 64), (1000, 320)):
    _layernorm_quant(*_shape)
_layernorm_quant(300, 320, ratio=8.0)


def _groupnorm_fp8(n, S, C, C2, fpg, silu):
    def build():
        g = G(n + S + C + C2 + fpg)
        i = I(x=(torch.randn(n, S, C, generator=g) * torch.logspace(-1, 0.5, n)[:, None, None] * 1.5 + 0.7).to(BF16),
              gamma=r32(g, C + C2, scale=0.4, shift=1.0), beta=r32(g, C + C2, scale=0.3))
        if C2:
            i.update(x2=(torch.randn(n, S, C2, generator=g) * 0.8 - 0.3).to(BF16))
        return i

    def ref(i):
        x = torch.cat([d(i.x), d(i.x2)], 2) if C2 else d(i.x)
        y = F.group_norm(x.view(n // fpg, fpg * S, C + C2).permute(0, 2, 1), 32, d(i.gamma), d(i.beta), 1e-5)
        return [(F.silu(y) if silu else y).permute(0, 2, 1).reshape(n, S, C + C2)]
    add(f"fp8_groupnorm_{n}x{S}x{C}" + (f"+{C2}" if C2 else "") + f"_fpg{fpg}", build, ref,
        lambda ops, i: [ops.groupnorm_fp8(i.x, i.gamma, i.beta, 1e-5, silu, fpg, x2=i.x2 if C2 else None)], [("Q", "gn", 16.0 if C2 else 8.0, n // fpg)], group="quant")


for _shape in ((4, 144, 320, 0, 1, True), (6, 100, 64, 0, 1, False), (6, 64, 192, 0, 3, True), (2, 576, 640, 320, 1, True), (50, 16, 1280, 1280, 1, True),
               (10, 300, 320, 0, 5, True)):   # the six shapes of tests/test_fp8_gpu.py: test_groupnorm_fp8
    _groupnorm_fp8(*_shape)


# ---- group mx8: the LayerNorm-folded q|k|v projection whose q | k columns leave as MX fp8 (csrc/gemm.hip forces its 256x320 tile: one run) ----
def _mx8(M, C):
    def build():
        g = G(M + C)
        return I(x=r16(g, M, C, shift=0.3), w=r16(g, 3 * C, C, scale=C ** -0.5), b=r32(g, 3 * C), gamma=r32(g, C, scale=0.2, shift=1.0), beta=r32(g, C, scale=0.3))

    def ref(i):
        y = ln_fold_ref(i.x, i.w, i.b, i.gamma, i.beta)
        return [y[:, 2 * C:].contiguous(), y[:, :2 * C].contiguous()]

    def run(ops, i):
        v, c8, cs = ops.linear(i.x, rehome_pack(ops.pack_linear(i.w, i.b, ln=Norm(i.gamma, i.beta))), ln=ops.rowstats(i.x), mx8_cols=2 * C)
        return [v, (c8, cs)]
    add(f"fp8_mx8_qkv_lnfold_{M}x{C}", build, ref, run, [("A", BF16), ("MX",)], kbreak=drop_k(), group="mx8")


_mx8(300, 320)
_mx8(333, 640)


# ---- group attn: attn_spatial_fp8qk ----
def attn_rebased(q, k, v, QW, thr=6.0):
    """softmax(q k^T) v in float64 with the roundings of attn_spatial_fp8qk_kernel<NW, QW, false> (module docstring): q, k, v (n, heads, S, 64), q
    scaled so that a score is the base-2 exponent. Returns (output, number of (wave, tile) re-bases after the first tile)."""
    n, h, S, _ = q.shape
    s = q @ k.transpose(-1, -2)
    nt = (S + 63) // 64
    if nt * 64 != S:
        s, v = F.pad(s, (0, nt * 64 - S), value=float("-inf")), F.pad(v, (0, 0, 0, nt * 64 - S))
    upper = ((torch.arange(64) >> 3) & 1).bool()     # the keys of a tile held by lane half 1
    W = 32 * QW
    nw = (S + W - 1) // W
    limit = 2.0 ** (thr + 5)
    m = s[..., :64].amax(-1, keepdim=True)
    num, den, rebases = torch.zeros(n, h, S, 64, dtype=F64), torch.zeros(n, h, S, 1, dtype=F64), 0
    for t in range(nt):
        st, vt = s[..., 64 * t:64 * t + 64], v[..., 64 * t:64 * t + 64, :]
        p = torch.exp2(st - m).to(F32).to(BF16).double()
        bad = torch.maximum(p[..., ~upper].sum(-1), p[..., upper].sum(-1)) > limit
        if bad.any():
            wave = F.pad(bad, (0, nw * W - S)).view(n, h, nw, W).any(-1, keepdim=True).expand(n, h, nw, W).reshape(n, h, nw * W)[..., :S, None]
            m_new = torch.where(wave, torch.maximum(m, st.amax(-1, keepdim=True)), m)
            num, den, m = num * torch.exp2(m - m_new), den * torch.exp2(m - m_new), m_new
            p = torch.exp2(st - m).to(F32).to(BF16).double()
            rebases += int(wave.sum()) // W
        num, den = num + p @ vt, den + p.sum(-1, keepdim=True)
    return num / den, rebases


_ATTN_REF = {}


def _attn(n, heads, S, variant):
    """q8 | k8: column views of one (M, 2C) buffer of e4m3 bytes, their E8M0 scales (124..130) likewise; logits of standard deviation about 3.
    variant "scale": a softmax scale; "pre": scale = 0.0 with a power of two folded into q's block scales (the pre-scaled query);
    "mx_out": as "scale", output as MX fp8, judged against the bf16 output of the "scale" call."""
    M, C, nb = n * S, heads * 64, heads * 2
    pre = variant == "pre"

    def build():
        g = G(n + heads + S)
        qk8 = _codes(g, M, 2 * C, amp=120.0)
        sc = torch.randint(124, 131, (M, 2 * nb), generator=g, dtype=U8)
        v = torch.randn(M, C, generator=g).to(BF16)
        deq = mx_deq(qk8[:S, :64], sc[:S, :2]), mx_deq(qk8[:S, C:C + 64], sc[:S, nb:nb + 2])
        scale = 3.0 / (deq[0] @ deq[1].t()).std().item()
        if pre:
            sh = round(math.log2(scale * LOG2E))
            sc[:, :nb] = (sc[:, :nb].to(torch.int16) + sh).clamp(1, 254).to(U8)
            scale = 0.0
        return I(qk8=qk8, sc=sc, v=v, scale=scale)

    def ref(i):
        key = (n, heads, S, pre)
        if key not in _ATTN_REF:
            deq = mx_deq(i.qk8, i.sc)
            q, k, v = (x.view(n, S, heads, 64).transpose(1, 2) for x in (deq[:, :C], deq[:, C:], d(i.v)))
            if pre and S >= 4096:        # <8, 2, true>: base 0
                o = attn_ref(q, k, v, zero_base=True)
            else:                        # <.., false>: first-tile base, re-based as the kernel does; scale = 0 runs it with scale_log2 = 1
                o, _ = attn_rebased(q if pre else q * (torch.tensor(i.scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).item(), k, v, 2 if S >= 4096 else 1)
            _ATTN_REF[key] = o.transpose(1, 2).reshape(M, C)
        return [_ATTN_REF[key]]

    def run(ops, i):
        assert "VISTA_ATTN_RESCALE_THR" not in os.environ, "attn_rebased emulates the kernel's default re-base threshold (2^6), which this variable overrides"
        args = (i.qk8[:, :C], i.qk8[:, C:], i.sc[:, :nb], i.sc[:, nb:], i.v, n, heads, S)
        o = ops.attn_spatial_fp8qk(*args, scale=i.scale)
        if variant != "mx_out":
            return [o]
        o8, osc = ops.attn_spatial_fp8qk(*args, scale=i.scale, mx_out=True)
        assert osc.shape[1] % 4 == 0 and osc.shape[1] >= nb
        return [(o8, osc, o)]
    key = f"fp8_attn_{n}x{heads}x{S}_{variant}"
    add(key, build, ref, run, [("MX", "own")] if variant == "mx_out" else [("B", key)], group="attn")


for _shape in ((2, 5, 144), (2, 3, 200), (1, 1, 2120), (1, 2, 4104), (1, 1, 4096)):   # 128-row; 128-row ragged; 256-row ragged; 512-row ragged; 512-row whole
    for _variant in ("scale", "pre", "mx_out"):
        _attn(*_shape, _variant)


BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and not set(BY_NAME) & set(bc.BY_NAME)
