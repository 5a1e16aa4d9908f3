"""The bounds of the fp16 kernel parity suite must bite (no GPU needed): for every case of tests/_f16_cases.py
  1. the float64 reference rounded once to the storage type passes the case's bound with no element excluded;
  2. the reference rounded to bf16 where fp16 is due (tests/_f16_cases.py: wrong_type_cast) fails it;
  3. GEMM / conv cases: the reference recomputed with the last 32 of K dropped for the rows of the last ragged 128-row tile ONLY fails it.
A bound that does not separate 1 from 2 and 3 proves nothing about a kernel that meets it."""
import pytest
import torch

from tests import _f16_cases as fc

_REF = {}


def _ref(case):
    if case.name not in _REF:
        i = case.build()
        _REF[case.name] = (i, [r.clone() for r in case.ref(i)])
    return _REF[case.name]


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_reference_passes_and_broken_outputs_fail(case):
    i, refs = _ref(case)
    assert len(refs) == len(case.specs)
    for k, (spec, ref) in enumerate(zip(case.specs, refs)):
        ok, fig = fc.check_any(spec, fc.storage_cast(spec, ref), ref)
        assert ok, f"{case.name}[{k}] {spec[0]}: the rounded reference itself misses the bound: {fig}"
        ok, fig = fc.check_any(spec, fc.wrong_type_cast(spec, ref), ref)
        assert not ok, f"{case.name}[{k}] {spec[0]}: a bf16-rounded output passes the bound: {fig}"
    if case.kbreak is not None:
        broken = case.ref(case.kbreak(i))
        for k, (spec, ref, rb) in enumerate(zip(case.specs, refs, broken)):
            bad = fc.splice_last_tile(case, ref, rb)
            assert not torch.equal(bad, ref)
            ok, fig = fc.check_any(spec, fc.storage_cast(spec, bad), ref)
            assert not ok, f"{case.name}[{k}] {spec[0]}: the last tile with 32 of K dropped passes the bound: {fig}"


def test_case_table_covers_the_issue():
    names = set(fc.BY_NAME)
    groups = {c.group for c in fc.CASES}
    assert groups == {"gemm", "splitk", "ff", "lnfold", "norm", "layout", "attn", "range"}
    assert sum(c.group == "ff" for c in fc.CASES) == 18 and sum(c.group == "attn" for c in fc.CASES) == 20
    assert {"alt_qkv_lnfold_C320_M300", "alt_qkv_lnfold_C640_M4173", "alt_boundary_32_of_320", "alt_boundary_288_of_320"} <= names
    for c in fc.CASES:   # every B bound is a measured value + 25 %
        for spec in c.specs:
            if spec[0] == "B":
                measured, bound = fc.B_BOUNDS[spec[1]]
                assert abs(bound / measured - 1.25) < 1e-2, spec[1]
