"""The bounds of the fp8 kernel parity suite must bite (no GPU needed): for every case of tests/_fp8_cases.py and every output
  1. the float64 reference cast once to the output's form passes the case's bound with no element excluded (Q / MX outputs: the reference
     quantised with round-to-nearest and the reference scale);
  2. bf16 outputs: the reference TRUNCATED toward zero to bf16 fails, and so does the correctly rounded value with its last mantissa bit cut (bound
     B through its cap, 1.5 x the rel-L2 of the rounded reference: both broken outputs lie above it);
  3. Q / MX outputs: codes rounded toward zero fail; MX blocks quantised at e_ref + 1 fail; at e_ref - 1 (which saturates) fail; scales rolled by
     one row (and, MX, by one block) inside the last 128-row tile fail;
  4. GEMM / conv cases: the last 128-row tile with the last 32 of K dropped fails; the double-rounded output, where the case has one, fails; the
     reference recomputed with a_scale (or the MX block scales of the activations) rolled by one row inside the last tile fails, and so does
     w_scale rolled by one channel inside the last 128-column tile -- which proves that the spread of the scales does its job.
A bound that does not separate 1 from 2, 3 and 4 proves nothing about a kernel that meets it."""
import os
import re

import pytest
import torch

from tests import _fp8_cases as fc

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_REF = {}


def _ref(case):
    if case.name not in _REF:
        i = case.build()
        _REF[case.name] = (i, case.ref(i))   # as returned: a reference may carry `sumabs` / `slack` for its bound (tests/_fp8_cases.py); never modified
    return _REF[case.name]


def _fails(spec, out, ref, tag, what):
    ok, fig = fc.check_any(spec, out, ref, tag)
    assert not ok, f"{tag} {spec[0]}: {what} passes the bound: {fig}"


def _roll_tail(t, r0, dim=0):
    """t with its entries from r0 on rolled by one along dim 0 (dim = 1: every row from r0 on rolled by one along dim 1). A last tile of a
    single row takes its neighbour from the row before."""
    t = t.clone()
    if dim == 0 and t.shape[0] - r0 < 2:
        r0 = t.shape[0] - 2
    t[r0:] = torch.roll(t[r0:], 1, dim)
    return t


def _quantised_broken_forms(spec, ref, tag):
    good = fc.perfect(spec, ref)
    rows = ref.reshape(-1, ref.shape[-1]).shape[0]
    if spec[0] == "Q":
        codes, s = good
        _fails(spec, (fc.q_good(spec, ref, codes_of=fc.toward_zero8)[0], s), ref, tag, "codes rounded toward zero")
        if s.numel() > 1:
            r0 = fc.last_tile_rows(s.numel()) if s.numel() == rows else 0   # per-row scales: inside the last tile; per image group: all of them
            assert not torch.equal(_roll_tail(s, r0), s)
            _fails(spec, (codes, _roll_tail(s, r0)), ref, tag, "scales rolled by one row")
        return
    own = good[2:]
    val = own[0].double() if own else ref.double()
    codes, sc = good[:2]
    e = fc.mx_e_ref(val)[0]
    t = val / torch.exp2(e).repeat_interleave(32, 1)
    _fails(spec, (fc.toward_zero8(t), sc) + own, ref, tag, "codes rounded toward zero")
    _fails(spec, fc.mx_quant(val, +1) + own, ref, tag, "blocks quantised at e_ref + 1")
    _fails(spec, fc.mx_quant(val, -1) + own, ref, tag, "blocks quantised at e_ref - 1")
    r0 = fc.last_tile_rows(rows)
    for dim in (0, 1):
        assert not torch.equal(_roll_tail(sc, r0, dim), sc)
        _fails(spec, (codes, _roll_tail(sc, r0, dim)) + own, ref, tag, f"scales rolled by one {'row' if dim == 0 else 'block'} in the last tile")


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_reference_passes_and_broken_outputs_fail(case):
    i, refs = _ref(case)
    assert len(refs) == len(case.specs)
    for k, (spec, ref) in enumerate(zip(case.specs, refs)):
        tag = f"{case.name}[{k}]"
        good = fc.perfect(spec, ref)
        if spec[0] == "B":
            cap = 1.5 * fc.rel_l2(good, ref)
            trunc, cut = fc.truncate_cast(("A", BF16), ref), fc.bitcut_cast(("A", BF16), ref)
            assert fc.rel_l2(trunc, ref) > cap and fc.rel_l2(cut, ref) > cap, (tag, fc.rel_l2(trunc, ref) / cap, fc.rel_l2(cut, ref) / cap)
            ok, fig = fc.check_any(spec, good, ref, tag)
            assert ok, f"{tag} B: the reference rounded once to bf16 misses the adopted bound: {fig}"
            continue
        ok, fig = fc.check_any(spec, good, ref, tag)
        assert ok, f"{tag} {spec[0]}: the reference cast once to the output's form misses the bound: {fig}"
        if spec[0] in ("Q", "MX"):
            _quantised_broken_forms(spec, ref, tag)
        elif fc.out_dtype(spec) is BF16:
            _fails(spec, fc.truncate_cast(spec, ref), ref, tag, "the reference truncated to bf16")
            _fails(spec, fc.bitcut_cast(spec, ref), ref, tag, "an output with its last mantissa bit cut")
    if case.kbreak is not None:
        broken = case.ref(case.kbreak(i))
        for k, (spec, ref, rb) in enumerate(zip(case.specs, refs, broken)):
            bad = fc.splice_last_tile(case, ref, rb)
            assert not torch.equal(bad, ref)
            _fails(spec, fc.perfect(spec, bad), ref, f"{case.name}[{k}]", "the last tile with 32 of K dropped")
    if case.dround is not None:
        for k, (spec, ref, dr) in enumerate(zip(case.specs, refs, case.dround(i))):
            _fails(spec, fc.perfect(spec, dr), ref, f"{case.name}[{k}]", "a double-rounded output")
    if case.group in ("dense", "geglu", "amx", "conv"):
        rows = refs[0].reshape(-1, refs[0].shape[-1]).shape[0]
        rolls = []
        if "a_mx" in i:
            rolls.append(("a_mx", _roll_tail(i.a_mx, fc.last_tile_rows(rows))))
        elif i.a_scale.numel() == rows:
            rolls.append(("a_scale", _roll_tail(i.a_scale, fc.last_tile_rows(rows))))
        elif i.a_scale.numel() > 1:      # convolutions: one scale per image group (a single group has no neighbour to take a scale from)
            rolls.append(("a_scale", torch.roll(i.a_scale, 1)))
        rolls.append(("w_scale", _roll_tail(i.w_scale, fc.last_tile_rows(i.w_scale.numel()))))
        for key, rolled in rolls:
            assert not torch.equal(rolled, i[key])
            j = fc.I(i)
            j[key] = rolled
            for k, (spec, ref, rb) in enumerate(zip(case.specs, refs, case.ref(j))):
                _fails(spec, fc.perfect(spec, rb), ref, f"{case.name}[{k}]", f"{key} rolled by one inside the last tile")


def test_case_table_covers_the_issue():
    names = set(fc.BY_NAME)
    count = lambda g: sum(c.group == g for c in fc.CASES)   # noqa: E731
    assert {c.group for c in fc.CASES} == set(fc.GROUPS) and all(count(g) == n for g, n in fc.GROUPS.items()), {g: count(g) for g in fc.GROUPS}
    assert fc.GROUPS == {"dense": 12, "geglu": 4, "amx": 6, "conv": 8, "quant": 17, "mx8": 2, "attn": 15}
    assert {f"fp8_linear_200x192x{K}_ktail" for K in (16, 80, 112, 144, 336)} <= names                                   # the K tails
    assert {"fp8_linear_strided_a_and_out", "fp8_linear_full_epilogue", "fp8_linear_emit_stats", "fp8_conv_t3_3x1x20_64to64",  # strided, epilogues, T = 1
            "fp8_amx_200x192x160_blend", "fp8_amx_200x192x160_res_rowvec_stats", "fp8_conv3x3_4x7x9_128to320_fps2", "fp8_layernorm_quant_300x320_mean_over_std_8",
            "fp8_geglu_200x64x256_mx_out", "fp8_attn_1x1x4096_pre", "fp8_attn_1x2x4104_mx_out"} <= names
    assert all(c.cfgs == fc.DENSE_CFGS for c in fc.CASES if c.group in ("dense", "amx")) and all(c.cfgs == fc.GEGLU_CFGS for c in fc.CASES if c.group == "geglu")
    assert all(c.cfgs == (0,) for c in fc.CASES if c.group in ("conv", "quant", "mx8", "attn"))
    assert all(c.kbreak is not None for c in fc.CASES if c.group in ("dense", "geglu", "amx", "conv", "mx8"))
    assert sum(c.dround is not None for c in fc.CASES) == 10     # the nine plain linear shapes and the full epilogue
    i = fc.BY_NAME["fp8_amx_200x192x160_blend"].build()
    assert i.a_mx.shape == (200, 8) and (i.a_mx[:, 5:] == 127).all() and int(i.a_mx[:, :5].min()) >= 119 and int(i.a_mx[:, :5].max()) <= 133
    i = fc.BY_NAME["fp8_linear_200x192x16_ktail"].build()
    assert i.a8.shape == (200, 48) and set(i.a8[:, 16:].unique().tolist()) == {0x7E, 0xFE}   # +-448 behind the K tail
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "fp8_kernel_parity.txt")) as f:
        profile = f.read()
    # the MFMA term of the fp32 bound: the worst figure of the probe of the instruction alone (profiles/fp8_mfma_sum_probe.txt), + 25 %
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "fp8_mfma_sum_probe.txt")) as f:
        text = f.read()
    for pattern, (measured, bound) in ((r"err/sum\|p\|=(\S+)", fc.MFMA_EPS), (r"rel_l2=(\S+)", fc.MFMA_REL)):
        probe = [float(x) for x in re.findall(r"^FP8MFMA .*" + pattern, text, re.M)]
        assert len(probe) >= 8 and abs(max(probe) / measured - 1) < 1e-3 and abs(bound / measured - 1.25) < 1e-2, (probe, measured, bound)
    for c in fc.CASES:
        _, refs = _ref(c)
        for k, (spec, ref) in enumerate(zip(c.specs, refs)):
            assert f"{c.name}[{k}] " in profile, f"profiles/fp8_kernel_parity.txt has no line for {c.name}[{k}]"
            if spec[0] == "B":     # a measured value + 25 %, and never above 1.5 x the output-rounding floor of its own reference
                measured, bound = fc.B_BOUNDS_FP8[spec[1]]
                assert abs(bound / measured - 1.25) < 1e-2, spec[1]
                floor = fc.rel_l2(fc.perfect(spec, ref), ref)
                assert floor <= measured and bound <= 1.5 * floor, (spec[1], measured, bound, floor)   # no output is closer to its reference than that reference rounded once
            if spec[0] == "F32":   # the fp32 outputs of the fp8 GEMM carry the MFMA term
                assert hasattr(ref, "sumabs") and ref.sumabs.shape == ref.shape, c.name
            if spec[0] == "MX":    # the reference alone puts at most 1 % of its blocks near a power of two, where e_ref +- 1 is accepted
                near = fc.mx_e_ref((fc.perfect(spec, ref)[2] if spec[1:] == ("own",) else ref).double())[1]
                assert near.float().mean().item() <= 0.01, (c.name, int(near.sum()), near.numel())


def test_a_plain_quantiser_emulation_meets_the_q_bound_and_a_truncating_one_does_not():
    """Rows spanning 2^-7 .. 2^7 at (300, 336): fp32 amax * (1 / 448), x * (1 / s), round-to-nearest cast -- what quantize_rows_kernel computes --
    stays within the Q tolerance; codes rounded toward zero sit at twice the tolerance with about half the elements outside."""
    g = fc.G(3)
    x = (torch.randn(300, 336, generator=g) * torch.logspace(-7, 7, 300, base=2.0)[:, None]).to(BF16)
    xf = x.float()
    s = xf.abs().amax(1) * torch.tensor(1.0 / 448.0, dtype=F32)
    t32 = xf * (1.0 / s)[:, None]
    ok, fig = fc.check_q(("Q", "rows"), (fc.q8(t32), s), x.double())
    assert ok and fig["code"] <= 1.0, fig
    ok, fig = fc.check_q(("Q", "rows"), (fc.toward_zero8(t32), s), x.double())
    assert not ok and fig["code"] > 1.9 and fig["bad"] > 0.4 * x.numel(), fig
