"""The folded upsample convolution on the MI355X (ops.pack_upconv2x2 / ops.upconv2x2; csrc/gemm_pipe.hip, UPCONV2X2) at the smallest shapes at which
each part of it can still go wrong (tests/_upconv_cases.py: GPU_SHAPES), in both storage builds, on the forced pipelined variant (tile_cfg 7: the
launcher's own size rule would hand shapes this small to the nine-tap form).

Every case runs on poisoned outputs inside guard bands (tests/_guard.py): an output row the scatter never writes is a NaN, a store outside the
tensor a damaged guard byte. Checks per shape: bound A of tests/_kernel_cases.py for every element against the float64 reference built from the
values the kernel is handed (the storage-type inputs and the pack's own folded, rounded class weights); two runs bitwise equal; image k of the
n-image call bitwise the same image run alone; agreement with ops.conv3x3(..., ups=2) on the nine-tap pack within the sum of the two bounds; and
both tile orders bitwise equal. tests/test_upconv_fold_cpu.py proves that the bound separates a correct output from a broken one.

The cross-check with the nine-tap form. Each output is held to bound A against ITS OWN reference, and the two references are not the same numbers: one
pack rounds the four folded weights, the other the nine taps (relative L2 between the two float64 references: 1.2-1.6e-3 in bf16, 1.6-2.0e-4 in fp16).
The sum of the two rel-L2 bounds is asserted as it stands (it has room for that distance). Element by element the sum of the two tolerances alone has
none where |ref| is small: two PERFECT outputs -- each reference rounded once to the storage type -- already differ by 1.9-3.5 x that sum at these
shapes (computed on the CPU), so the distance |ref - ref9| of the two float64 references, which no kernel has touched, is added to it: the triangle
inequality through the two references, under which the perfect outputs sit at 0.69-0.78. The figure without that term is printed beside it."""
import os

import pytest
import torch

from tests import _guard
from tests import _kernel_cases as kc
from tests import _upconv_cases as uc

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
_CASES = {F16: None, BF16: None}


def _table(st):
    if _CASES[st] is None:
        _CASES[st] = kc.make_cases(st)
    return _CASES[st]


@pytest.fixture(params=[BF16, F16], ids=["bf16", "fp16"])
def storage(request):
    from vista_amd import build, ops
    if not os.path.exists(build.LIB_F16):
        pytest.fail("vista_amd/lib/libvista_hip_f16.so is missing: __graft_entry__.build() links both storage variants")
    saved = (ops.TILE_CFG, ops.UPCONV_CLASS_FASTEST)
    try:
        with ops.storage(request.param), _guard.guarded(ops):
            ops.TILE_CFG = 7
            yield ops, request.param
            _guard.verify()
    finally:
        ops.TILE_CFG, ops.UPCONV_CLASS_FASTEST = saved


def _tol_a(ref, st):
    u = kc._unit(st)
    return 1.25 * u * ref.abs() + 0.25 * u * ref.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("shape", uc.GPU_SHAPES, ids=[uc.shape_id(s) for s in uc.GPU_SHAPES])
def test_folded_upsample_conv(shape, storage):
    ops, st = storage
    n, H, W, cin, cout, rowvec = shape
    cases = _table(st)
    host = uc.inputs(st, n, H, W, cin, cout, rowvec)
    i = _guard.embed(host)
    rv = i.rv if rowvec else None
    pw = ops.pack_upconv2x2(i.w, i.b)
    assert ops.upconv2x2_fits(i.x, pw, n, H, W, rowvec=rv), "the forced pipelined variant takes every shape of this table"
    out, Ho, Wo = ops.upconv2x2(i.x, pw, n, H, W, rowvec=rv)
    assert (Ho, Wo) == (2 * H, 2 * W) and tuple(out.shape) == (n, 4 * H * W, cout) and out.dtype is st

    # parity: bound A against the float64 reference of the values the kernel was handed
    ref = uc.folded_ref(host.x, ops.unpack_upconv2x2(pw, cout).cpu(), host.b, n, H, W, host.get("rv"))
    ok, fig = cases.check(("A", st), out, ref)
    print(f"UPCONVPARITY {uc.shape_id(shape)} {st}: {fig}")
    assert ok, fig

    # repeatability, and the other tile order: bitwise
    again = ops.upconv2x2(i.x, pw, n, H, W, rowvec=rv)[0]
    assert torch.equal(again, out), "two runs must be bitwise equal"
    ops.UPCONV_CLASS_FASTEST = not ops.UPCONV_CLASS_FASTEST
    try:
        other = ops.upconv2x2(i.x, pw, n, H, W, rowvec=rv)[0]
    finally:
        ops.UPCONV_CLASS_FASTEST = not ops.UPCONV_CLASS_FASTEST
    assert torch.equal(other, out), "the tile order must not change a bit of the output"

    # batch independence: image k of the n-image call == the same image run alone
    for k in sorted({0, n - 1}):
        alone = ops.upconv2x2(i.x[k:k + 1], pw, 1, H, W, rowvec=None if rv is None else rv[k:k + 1])[0]
        assert torch.equal(alone[0], out[k]), f"image {k} depends on its batch"

    # cross-check with the nine-tap form on the unfolded weights: within the sum of the two bounds, element by element
    nine = ops.conv3x3(i.x, ops.pack_conv3x3(i.w, i.b), n, H, W, ups=2, rowvec=rv)[0]
    ref9 = uc.nine_tap_ref(host.x, host.w.to(st), host.b, n, H, W, host.get("rv"))
    ok9, fig9 = cases.check(("A", st), nine, ref9)
    diff = (out.cpu().double() - nine.cpu().double()).abs()
    worst = (diff / (_tol_a(ref, st) + _tol_a(ref9, st))).max().item()
    worst_refs = (diff / (_tol_a(ref, st) + _tol_a(ref9, st) + (ref - ref9).abs())).max().item()
    r, r_bound = kc.rel_l2(out.cpu(), nine.cpu()), fig["rel_l2_bound"] + fig9["rel_l2_bound"]
    print(f"UPCONVPARITY {uc.shape_id(shape)} {st}: nine-tap {fig9}; folded vs nine-tap elem/(sum of bounds)={worst:.4f} "
          f"(with the references' own distance: {worst_refs:.4f}) rel_l2={r:.4g} bound={r_bound:.4g} refs rel_l2={kc.rel_l2(ref, ref9):.4g}")
    assert ok9, fig9
    assert r <= r_bound and worst_refs <= 1.0


def test_a_folded_pack_is_refused_by_the_nine_tap_call_and_declined_shapes_raise(storage):
    """No quiet change of algorithm: ops.conv3x3 refuses a folded pack, ops.upconv2x2 a nine-tap one, and a shape the pipelined kernel does not take
    (Cout % 320 != 0) answers upconv2x2_fits False and raises from upconv2x2."""
    from vista_amd._lib import VistaHipError
    ops, st = storage
    n, H, W, cin = 2, 9, 16, 64
    x = _guard.put(torch.randn(n, H * W, cin).to(st))
    w = torch.randn(128, cin, 3, 3) * (9 * cin) ** -0.5
    pw4, pw9 = ops.pack_upconv2x2(w, None), ops.pack_conv3x3(w, None)
    with pytest.raises(ValueError):
        ops.conv3x3(x, pw4, n, H, W, ups=2)
    with pytest.raises(ValueError):
        ops.upconv2x2(x, pw9, n, H, W)
    assert not ops.upconv2x2_fits(x, pw4, n, H, W)
    with pytest.raises(VistaHipError):
        ops.upconv2x2(x, pw4, n, H, W)
