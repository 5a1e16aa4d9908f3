"""The folded upsample convolution without a GPU: the fold identity in float64, the content of the weight pack in both storage types, that folding
does not cost accuracy, what the loaded library's validation accepts and refuses, and that the bound of tests/test_upconv_fold_gpu.py (bound A of
tests/_kernel_cases.py) passes the emulated reference and fails a broken output."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import _kernel_cases as kc
from tests import _upconv_cases as uc

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64


@pytest.mark.parametrize("n,cin,H,W", [(1, 3, 1, 1), (2, 5, 1, 7), (2, 8, 5, 3), (1, 4, 9, 16)])
def test_fold_identity_in_float64(n, cin, H, W):
    """The scatter of the four 2x2 convolutions with the UNROUNDED fold equals conv2d(interpolate(x, 2, "nearest"), w, b, padding=1) to <= 1e-12
    relative; (1, 3, 1, 1): every neighbour out of range."""
    from vista_amd import ops
    g = kc.G(n + cin + H + W)
    cout = 6
    x = torch.randn(n, cin, H, W, generator=g, dtype=F64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=F64)
    b = torch.randn(cout, generator=g, dtype=F64)
    wc = ops.fold_upconv2x2(w)
    assert wc.shape == (4, cout, cin, 2, 2) and wc.dtype == F64
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    got = uc.scatter_2x2(x, wc, b)
    rel = kc.rel_l2(got, ref)
    worst = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"UPCONV fold identity {n}x{cin}x{H}x{W}: rel_l2={rel:.3g} worst/max={worst:.3g}")
    assert rel <= 1e-12 and worst <= 1e-12


def _fold_by_hand(w):
    """The documented fold written independently of ops.fold_upconv2x2: class 2a + b, rows {w[0], w[1] + w[2]} for a = 0 and {w[0] + w[1], w[2]}
    for a = 1, columns by the same rule with b; rows summed first, then columns, in w's arithmetic."""
    rows = {0: (w[:, :, 0], w[:, :, 1] + w[:, :, 2]), 1: (w[:, :, 0] + w[:, :, 1], w[:, :, 2])}
    out = torch.zeros(4, w.shape[0], w.shape[1], 2, 2, dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                r = rows[a][dy]
                cols = (r[:, :, 0], r[:, :, 1] + r[:, :, 2]) if b == 0 else (r[:, :, 0] + r[:, :, 1], r[:, :, 2])
                for dx in (0, 1):
                    out[2 * a + b, :, :, dy, dx] = cols[dx]
    return out


@pytest.mark.parametrize("st", [BF16, F16], ids=["bf16", "fp16"])
def test_pack_content(st):
    """Unpacking pack_upconv2x2 gives the fp32 fold rounded once to the storage type; padding rows are zero; the four classes sit in the documented
    order (class 2a + b at rows [(2a + b) Np, (2a + b + 1) Np)), each [Cout][Cin/64][2 dy + dx][64]; one fp32 bias vector."""
    from vista_amd import ops
    g = kc.G(11)
    cout, cin = 40, 128
    w = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(cout, generator=g)
    with ops.storage(st):
        pw = ops.pack_upconv2x2(w, b, device="cpu")
        back = ops.unpack_upconv2x2(pw, cout)
    Np = max(ops.ceil_to(cout, 256), ops.ceil_to(cout, 320))
    assert pw.wt.dtype is st and pw.wt.shape == (4 * Np, 4 * cin) and pw.K == 4 * cin and pw.N == cout and pw.classes == 4
    want = _fold_by_hand(w).to(st)
    assert torch.equal(back, want), "the pack must hold the fp32 fold rounded once"
    rows = pw.wt.view(4, Np, 4 * cin)
    assert torch.equal(rows[:, cout:], torch.zeros(4, Np - cout, 4 * cin, dtype=st)), "padding rows must be zero"
    # the layout, element by element: class c, output channel o, input channel ci, tap (dy, dx) at row c * Np + o, column (ci // 64) * 256 + (2 dy + dx) * 64 + ci % 64
    for c, o, ci, dy, dx in ((0, 0, 0, 0, 0), (1, 7, 65, 1, 0), (2, 39, 127, 0, 1), (3, 13, 64, 1, 1)):
        assert pw.wt[c * Np + o, (ci // 64) * 256 + (2 * dy + dx) * 64 + ci % 64] == want[c, o, ci, dy, dx]
    assert pw.bias.dtype is F32 and pw.bias.shape == (Np,) and torch.equal(pw.bias[:cout], b) and not pw.bias[cout:].any()
    # folding from the fp32 master weights, not from rounded ones
    assert not torch.equal(back, _fold_by_hand(w.to(st).float()).to(st))
    with pytest.raises(ValueError):
        ops.pack_upconv2x2(torch.randn(8, 48, 3, 3), None, device="cpu")   # Cin % 64


@pytest.mark.parametrize("n,H,W,cin,cout", [(2, 9, 16, 128, 64), (1, 18, 32, 64, 96), (2, 5, 7, 320, 32)])
def test_accuracy_is_not_degraded(n, H, W, cin, cout):
    """bf16 inputs, weights rounded once to bf16 (the fold: folded in fp32 first), float64 accumulation, one output rounding: the folded form's
    relative L2 against the float64 nine-tap reference of the master weights is within 1.1 x the nine-tap form's own. At the three UNet shapes the
    folded form measured 2.87-2.89e-3 against 2.83-2.90e-3."""
    from vista_amd import ops
    i = uc.inputs(BF16, n, H, W, cin, cout)
    ref = uc.nine_tap_ref(i.x, i.w, i.b, n, H, W)
    nine = uc.nine_tap_ref(i.x, i.w.to(BF16), i.b, n, H, W).to(F32).to(BF16)
    fold = uc.folded_ref(i.x, ops.fold_upconv2x2(i.w).to(BF16), i.b, n, H, W).to(F32).to(BF16)
    e9, e4 = kc.rel_l2(nine, ref), kc.rel_l2(fold, ref)
    print(f"UPCONV accuracy {n}x{H}x{W}x{cin}x{cout}: nine-tap rel_l2={e9:.4g} folded rel_l2={e4:.4g} ratio={e4 / e9:.4f}")
    assert e4 <= 1.1 * e9


def _desc(ops, n, H, W, cin, cout, folded=True):
    one = C.c_void_p(4096)
    d = ops.VkGemmDesc()
    d.A = d.Wt = d.out = d.bias = one
    d.M, d.N, d.K, d.lda, d.ldc, d.alpha = n * 4 * H * W, cout, (4 if folded else 9) * cin, cin, cout, 1.0
    d.amode, d.epi = (ops.AMODE_UPCONV2X2 if folded else ops.AMODE_CONV3X3), ops.EPI_LINEAR
    d.Cin, d.H, d.Wd, d.Hout, d.Wout, d.stride, d.ups = cin, H, W, 2 * H, 2 * W, 1, 2
    d.splitk_ws, d.splitk_ws_bytes = one, 160 << 20
    return d


def test_validation_through_the_loaded_library():
    """vk_gemm_tile_choice (host arithmetic; the library loads without a GPU): the new mode is taken by the pipelined kernel (7 * 16 + 1) at the three
    BASELINE shapes, refused with each option it does not support, declined where the nine-tap form would not run on that kernel in one launch,
    and a nine-tap ups == 2 descriptor is still accepted."""
    from vista_amd import _lib, ops
    lib = _lib.load()
    one = C.c_void_p(4096)
    choice = lambda d: lib.vk_gemm_tile_choice(C.byref(d))   # noqa: E731
    for s in uc.BASELINE_SHAPES:
        assert choice(_desc(ops, *s)) == 7 * 16 + 1, s
        d = _desc(ops, *s)
        d.tile_cfg = 8                                        # the class-fastest order
        assert choice(d) == 7 * 16 + 1, s
        d = _desc(ops, *s)
        d.rowvec, d.ldv, d.rows_per_vec = one, s[4], 4 * s[1] * s[2]
        assert choice(d) == 7 * 16 + 1, s
        assert choice(_desc(ops, *s, folded=False)) == 7 * 16 + 1, "the nine-tap form with the fused upsample is unchanged"
    s = uc.BASELINE_SHAPES[1]

    def refused(**kw):
        d = _desc(ops, *s)
        for k, v in kw.items():
            setattr(d, k, v)
        return choice(d) < 0
    assert refused(res1=one, ld_res1=s[4]) and refused(res2=one, ld_res2=s[4], beta=1.0)
    assert refused(gnstat_out=one, gn_rows=4 * s[1] * s[2])
    assert refused(rowstat_out=one)
    assert refused(out_f32=1)
    assert refused(mx8_out=one, mx8_scales=one, mx8_cols=320, ld_mx8=320, ld_mx8s=10)
    assert refused(halo_prev=one) and refused(halo_next=one)
    assert refused(m_begin=256) and refused(m_end=s[0] * 2 * s[1] * s[2])
    for cfg in (1, 2, 3, 4, 5, 6, 16, 64):                   # the sixteen-wave and the other tile variants
        assert refused(tile_cfg=cfg), cfg
    assert refused(K=9 * s[3]) and refused(ups=1) and refused(stride=2) and refused(asym_pad=1) and refused(Hout=s[1]) and refused(M=s[0] * 4 * s[1] * s[2] + 4)
    assert refused(rowvec=one, ldv=s[4], rows_per_vec=s[1] * s[2])
    # declined (the caller runs the nine-tap form): the VAE decoder's widths, a rank whose M is small enough for split-K, a forced variant 7 on N % 320 != 0
    assert choice(_desc(ops, 1, 72, 128, 512, 512)) < 0 and choice(_desc(ops, 1, 144, 256, 256, 256)) < 0 and choice(_desc(ops, 1, 288, 512, 128, 128)) < 0
    assert choice(_desc(ops, 2, 9, 16, 1280, 1280)) < 0
    nine = _desc(ops, 2, 9, 16, 1280, 1280, folded=False)
    assert choice(nine) % 16 > 1, "the nine-tap form of that shape splits K"
    d = _desc(ops, 2, 9, 16, 64, 128)
    d.tile_cfg = 7
    assert choice(d) < 0
    d = _desc(ops, 2, 9, 16, 64, 320)                         # what the GPU tests run: small shapes on the forced variant 7
    d.tile_cfg = 7
    assert choice(d) == 7 * 16 + 1
    assert lib.vk_abi_version() == 9


def _broken_outputs(ops, i, n, H, W, st):
    wc = ops.fold_upconv2x2(i.w).to(st)
    swapped = wc[[0, 2, 1, 3]]                                # two classes swapped
    unsummed = wc.clone()
    unsummed[0, :, :, 1, :] = ops.fold_upconv2x2(torch.stack([i.w[:, :, 0], i.w[:, :, 1], torch.zeros_like(i.w[:, :, 2])], 2)).to(st)[0, :, :, 1, :]
    return wc, {"classes swapped": swapped, "tap left unsummed": unsummed}   # class (0, b), dy = 1: w[1] alone instead of w[1] + w[2]


@pytest.mark.parametrize("st", [BF16, F16], ids=["bf16", "fp16"])
def test_the_bound_judges_correctly(st):
    """Bound A, as the GPU test applies it (reference: float64 from the storage-type inputs and the pack's own rounded class weights), passes that
    reference rounded once to the storage type and fails an output computed with two classes swapped or with one tap's weights left unsummed."""
    from vista_amd import ops
    cases = kc.make_cases(st)
    n, H, W, cin, cout, _ = uc.GPU_SHAPES[0]
    i = uc.inputs(st, n, H, W, cin, cout)
    wc, broken = _broken_outputs(ops, i, n, H, W, st)
    ref = uc.folded_ref(i.x, wc, i.b, n, H, W)
    ok, fig = cases.check(("A", st), ref.to(F32).to(st), ref)
    print(f"UPCONV bound A on the emulated reference: {fig}")
    assert ok, fig
    for what, wb in broken.items():
        ok, fig = cases.check(("A", st), uc.folded_ref(i.x, wb, i.b, n, H, W).to(F32).to(st), ref)
        print(f"UPCONV bound A on a broken output ({what}): {fig}")
        assert not ok, what
