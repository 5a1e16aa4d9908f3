"""The bounds of the bf16 kernel parity suite must bite (no GPU needed): for every case of tests/_bf16_cases.py and every output
  1. the float64 reference rounded once (to nearest even) to the output's type passes the case's bound with no element excluded;
  2. 16-bit outputs: the reference TRUNCATED toward zero to bf16 fails it, and so does the correctly rounded value with its last mantissa bit cut
     (fp32 outputs are exempt). Bound B takes part through its cap: no adopted B bound exceeds 1.5 x the rel-L2 of the rounded reference (the
     table test below), and both broken outputs lie above that cap. A bitwise (X) output whose reference is exactly representable in bf16 --
     a copy kernel's -- cannot be truncated wrong; its bit-cut form still fails;
  3. GEMM / conv cases: the reference recomputed with the last 32 of K dropped for the rows of the last ragged 128-row tile ONLY fails it;
  4. the plain linear_* 16-bit cases and the full epilogue: the double-rounded output -- the product rounded to bf16 BEFORE bias and residuals are
     added -- fails it.
A bound that does not separate 1 from 2, 3 and 4 proves nothing about a kernel that meets it. tests/test_kernels_gpu.py: close() passes all of 2 and 4."""
import os

import pytest
import torch

from tests import _bf16_cases as bc

BF16, F32 = torch.bfloat16, torch.float32
_REF = {}


def _ref(case):
    if case.name not in _REF:
        i = case.build()
        _REF[case.name] = (i, [r.clone() for r in case.ref(i)])
    return _REF[case.name]


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_reference_passes_and_broken_outputs_fail(case):
    i, refs = _ref(case)
    assert len(refs) == len(case.specs)
    for k, (spec, ref) in enumerate(zip(case.specs, refs)):
        tag = f"{case.name}[{k}]"
        good = bc.storage_cast(spec, ref)
        ok, fig = bc.check_any(spec, good, ref, tag)
        assert ok, f"{tag} {spec[0]}: the rounded reference itself misses the bound: {fig}"
        if bc.out_dtype(spec) is F32:
            continue
        assert bc.out_dtype(spec) is BF16
        trunc, cut = bc.truncate_cast(spec, ref), bc.bitcut_cast(spec, ref)
        if spec[0] == "B":
            cap = 1.5 * bc.rel_l2(good, ref)
            assert bc.rel_l2(trunc, ref) > cap and bc.rel_l2(cut, ref) > cap, (tag, bc.rel_l2(trunc, ref) / cap, bc.rel_l2(cut, ref) / cap)
            continue
        if not (spec[0] == "X" and torch.equal(trunc, good)):
            ok, fig = bc.check_any(spec, trunc, ref, tag)
            assert not ok, f"{tag} {spec[0]}: the reference truncated to bf16 passes the bound: {fig}"
        ok, fig = bc.check_any(spec, cut, ref, tag)
        assert not ok, f"{tag} {spec[0]}: an output with its last mantissa bit cut passes the bound: {fig}"
    if case.kbreak is not None:
        broken = case.ref(case.kbreak(i))
        for k, (spec, ref, rb) in enumerate(zip(case.specs, refs, broken)):
            bad = bc.splice_last_tile(case, ref, rb)
            assert not torch.equal(bad, ref)
            ok, fig = bc.check_any(spec, bc.storage_cast(spec, bad), ref, f"{case.name}[{k}]")
            assert not ok, f"{case.name}[{k}] {spec[0]}: the last tile with 32 of K dropped passes the bound: {fig}"
    if case.dround is not None:
        for k, (spec, ref, dr) in enumerate(zip(case.specs, refs, case.dround(i))):
            ok, fig = bc.check_any(spec, bc.storage_cast(spec, dr), ref, f"{case.name}[{k}]")
            assert not ok, f"{case.name}[{k}] {spec[0]}: a double-rounded output passes the bound: {fig}"


def test_case_table_covers_the_issue():
    names = set(bc.BY_NAME)
    groups = {c.group for c in bc.CASES}
    assert groups == {"gemm", "splitk", "ff", "lnfold", "norm", "layout", "attn", "vt", "firststage"}
    count = lambda g: sum(c.group == g for c in bc.CASES)
    assert count("ff") == 18 and count("attn") == 20 and count("vt") == 3 and count("firststage") == 14 and count("lnfold") == 4
    assert {"attn_temporal_1x3x4099x5", "attn_temporal_2x31x5x1", "groupnorm_large_mean", "layout_past_the_grid_stride_wrap", "rowwise_elementwise_3x349531",
            "sampler_prepare_2x13111x320_uc_replace", "sampler_update_29x9041x4", "conv3d_1x4x16x24_64to4", "softmax_rows_7x16384", "attn_small_1x2x300x128",
            "linear_act_gelu_257x5120x1280", "vt_attn_spatial_1x1x2120"} <= names
    assert not {n for n in names if n.startswith(("alt_", "subnormal", "overflow"))}, "fp16-specific cases stay fp16-only"
    assert sum(c.dround is not None for c in bc.CASES) == 6
    assert all(c.cfgs == (0, 1, 2, 3) for c in bc.CASES if c.name.startswith("conv3d"))
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "bf16_kernel_parity.txt")) as f:
        profile = f.read()
    for c in bc.CASES:
        _, refs = _ref(c)
        for k, (spec, ref) in enumerate(zip(c.specs, refs)):
            assert f"{c.name}[{k}] " in profile, f"profiles/bf16_kernel_parity.txt has no line for {c.name}[{k}]"
            if spec[0] == "B":     # a measured value + 25 %, and never above 1.5 x the output-rounding floor of its own reference
                measured, bound = bc.B_BOUNDS[spec[1]]
                assert abs(bound / measured - 1.25) < 1e-2, spec[1]
                floor = bc.rel_l2(bc.storage_cast(spec, ref), ref)
                assert bound <= 1.5 * floor, (spec[1], bound, floor)
            if spec[0] == "LN":    # measured + 25 %; check_ln_fold holds every element to close() besides, so nothing loosens
                measured, bound = bc.LN_BOUNDS[f"{c.name}[{k}]"]
                assert abs(bound / measured - 1.25) < 1e-2, c.name


def test_groupnorm_large_mean_routes_raw_sums_leave_margin():
    """The two bf16 GroupNorm routes that keep raw fp32 sums across the ABI (statistics from a conv3x3 epilogue's 64-row partials; groupnorm_sharded's
    32-row partials) at |group mean| = 10 .. 30 std of (2, 48 x 48, 320) (tests/_kernel_cases.py: gn_route_inputs): a plain-torch emulation of raw
    fp32 (sum, sum of squares) -> E[x^2] - mean^2 on the conv's stored output stays within 0.8 x bound A's tolerance, so the GPU test
    (tests/test_bf16_kernels_gpu.py) can hold both routes to bound A itself."""
    i = bc.gn_route_inputs()
    y = bc.conv3x3_ref(i.x, i.w, i.b, i.n, i.H, i.W).to(F32).to(BF16)
    group_mean = y.double().view(i.n, -1, 32, i.C // 32).mean((1, 3)).abs()
    group_std = y.double().view(i.n, -1, 32, i.C // 32).std((1, 3))
    assert (group_mean / group_std).min() > 0.9 * bc.GN_ROUTE_MEAN[0] and (group_mean / group_std).max() < 1.1 * bc.GN_ROUTE_MEAN[1]
    ref = bc.gn_route_ref(y, i.gamma, i.beta)
    for chunk in (64, 32):
        ok, fig = bc.check(("A", BF16), bc.gn_raw_sum_emulation(y, i.gamma, i.beta, chunk), ref)
        print(f"raw fp32 sums in {chunk}-row chunks: {fig}")
        assert ok and fig["elem"] <= 0.8, (chunk, fig)
