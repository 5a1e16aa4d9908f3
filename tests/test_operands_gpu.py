"""Refusals of the operand contract (include/vista_hip.h; vista_amd/ops.py: _operand / _dense), held in place on the GPU: every hot-path wrapper is
first called once with operands inside their contract (the call must work), then once per bad operand -- a base address the kernels' widest access
cannot take, a bad leading dimension, the wrong dtype, stride(-1) != 1, one row or one column short, geometry arguments that overstate x, a short
or 16-bit gamma. Each bad call must raise ValueError naming the operand BEFORE anything is launched: afterwards every poisoned output arena of the
context is still entirely 0xFF and verify() passes. The C entry points, handed the same live pointers through ctypes, must answer VK_EINVAL.

Every bad operand is a view of a larger live arena (tests/_guard.py), a "short" tensor a view of a full-size one: whatever address the mistaken
extent or alignment could reach is memory this test owns. Nothing here finds out what a misaligned launch does -- the checks come first."""
import ctypes as C

import pytest
import torch

from tests import _guard

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
EINVAL = -22
COUNT = {"python": 0, "c": 0}


@pytest.fixture(params=[BF16, F16], ids=["bf16", "fp16"])
def ctx(request):
    from vista_amd import ops
    with ops.storage(request.param), _guard.guarded(ops) as s:
        yield ops, request.param, s
        _guard.verify()
        print(f"OPERANDS gpu refusals so far: python={COUNT['python']} c={COUNT['c']}")


def rnd(*shape, dtype, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def good(*shape, dtype, seed=0, scale=1.0):
    return _guard.put(rnd(*shape, dtype=dtype, seed=seed, scale=scale), label="good")


def untouched(s, what):
    """Nothing was launched: every poisoned allocation of the context is still all 0xFF, every guard and input intact."""
    torch.cuda.synchronize()
    for a in s.arenas:
        if a.role == "empty" and getattr(a, "expect_poison", True):
            assert bool((a.interior() == _guard.POISON).all()), f"{what}: {a} was written although the call was refused"
    _guard.verify()


def launched(s, result, keep=()):
    """A call that is expected to work was made (result: its output, finite): what it allocated -- output, statistics, workspaces -- is written from here
    on and no evidence about later calls; the poisoned outputs in `keep` (handed to no working call) stay under watch."""
    for t in (result if isinstance(result, (tuple, list)) else (result,)):
        if torch.is_tensor(t):
            assert torch.isfinite(t.float()).all(), "the call inside the contract left an element unwritten"
    kept = {t.untyped_storage().data_ptr() for t in keep}
    for a in s.arenas:
        if a.base.untyped_storage().data_ptr() not in kept:
            a.expect_poison = False


def refuse(s, fn, name, what):
    with pytest.raises(ValueError, match=None if name is None else f"^(PackedWeight\\.)?{name}: "):
        fn()
    COUNT["python"] += 1
    untouched(s, f"{what} ({name})")


def bad_views(t, align, ld_mult, rows=True, cols=True, other=None):
    """Bad stand-ins for the 2-D operand t (rows, cols), each a view of a live arena that owns every address the view's mistaken layout could reach:
    skewN = N bytes off (the skews of 2, 4, 8 that t's element size can express and `align` excludes), ld = rows ld_mult / 2 elements too far
    apart, dtype = the other 16-bit type (fp32 operands: bf16), stride = every second column of a twice as wide arena, row_short / col_short."""
    r, c = t.shape
    item = t.element_size()
    out = {}
    big = _guard.put(torch.zeros(r + 2, c + 16, dtype=t.dtype), label="bad operand's arena")
    for skew in (2, 4, 8):
        if skew % item == 0 and skew % align:
            out[f"skew{skew}"] = big.view(-1)[skew // item:skew // item + r * c].view(r, c)
    if ld_mult > 1:
        wide = _guard.put(torch.zeros(r + 1, c + ld_mult // 2, dtype=t.dtype), label="bad operand's arena")
        out["ld"] = wide[:r, :c]
        assert out["ld"].stride(0) % ld_mult and out["ld"].data_ptr() % 16 == 0
    other = other or (F32 if t.dtype is not F32 else BF16)
    out["dtype"] = _guard.put(torch.zeros(r, c, dtype=other), label="bad operand's arena")
    out["stride"] = _guard.put(torch.zeros(r, 2 * c, dtype=t.dtype), label="bad operand's arena")[:, ::2]
    if rows and r > 1:
        out["row_short"] = t[:r - 1]
    if cols:
        out["col_short"] = t[:, :c - 4]
    return out


def sixteen_bit_other(st):
    return F16 if st is BF16 else BF16


# ------------------------------------------------------------------------------------------------ GEMM family
def test_linear_refuses_bad_operands(ctx):
    ops, st, s = ctx
    M, N, K, rpv = 40, 64, 64, 10
    x, r1, r2 = good(M, K, dtype=st), good(M, N, dtype=st, seed=1), good(M, N, dtype=st, seed=2)
    rv, rv2 = good(M // rpv, N, dtype=F32, seed=3), good(M // rpv, N, dtype=F32, seed=4)
    pw = ops.pack_linear(rnd(N, K, dtype=st, seed=5, scale=K ** -0.5), rnd(N, dtype=F32, seed=6))
    out = _guard.empty((M, N), st)
    out32 = _guard.empty((M, N), F32)
    kw = dict(rowvec=rv, rows_per_vec=rpv, res1=r1, res2=r2, alpha=0.5, beta=0.5, rowvec2=rv2)
    launched(s, ops.linear(x, pw, **kw), keep=(out, out32))
    o16 = sixteen_bit_other(st)
    for k, v in bad_views(x, 16, 8, rows=False, other=o16).items():
        refuse(s, lambda: ops.linear(v, pw, out=out), None if k == "col_short" else "x", f"linear x {k}")
    for k, v in bad_views(out, 8, 4, other=o16).items():
        refuse(s, lambda: ops.linear(x, pw, out=v), "out", f"linear out {k}")
    for k, v in bad_views(out32, 16, 4, other=torch.float64).items():
        refuse(s, lambda: ops.linear(x, pw, out=v, out_f32=True), "out", f"linear fp32 out {k}")
    for name, t in (("res1", r1), ("res2", r2)):
        for k, v in bad_views(t, 8, 4, other=o16).items():
            refuse(s, lambda: ops.linear(x, pw, out=out, **{**kw, name: v}), name, f"linear {name} {k}")
    for name, t in (("rowvec", rv), ("rowvec2", rv2)):
        for k, v in bad_views(t, 16, 4).items():
            older = name == "rowvec2" and k in ("ld", "stride")   # (refused by the older rule that rowvec and rowvec2 share one row stride: no operand name in that message)
            refuse(s, lambda: ops.linear(x, pw, out=out, **{**kw, name: v}), None if older else name, f"linear {name} {k}")
    x2 = good(M, K, dtype=st, seed=7)
    pw2 = ops.pack_linear(rnd(N, 2 * K, dtype=st, seed=8, scale=K ** -0.5), None)
    launched(s, ops.linear(x, pw2, x2=x2), keep=(out, out32))
    for k, v in bad_views(x2, 16, 8, rows=True, cols=False, other=o16).items():
        refuse(s, lambda: ops.linear(x, pw2, x2=v, out=out), None if k == "row_short" else "x2", f"linear x2 {k}")
    # the C entry point with the same live pointers: every pointer below lies inside an arena of this test
    lib = ops._lib.load()

    def c_desc(**over):
        d = ops.VkGemmDesc()
        d.A, d.lda, d.Wt, d.bias, d.out, d.ldc = ops._p(x), K, ops._p(pw.wt), ops._p(pw.bias), ops._p(out), N
        d.M, d.N, d.K, d.alpha = M, pw.N, pw.K, 1.0
        for k, v in over.items():
            setattr(d, k, v)
        return d
    for what, over in (("A + 2", dict(A=C.c_void_p(x.data_ptr() + 2))), ("A + 8", dict(A=C.c_void_p(x.data_ptr() + 8))),
                       ("Wt + 2", dict(Wt=C.c_void_p(pw.wt.data_ptr() + 2))), ("out + 2", dict(out=C.c_void_p(out.data_ptr() + 2))),
                       ("out + 4", dict(out=C.c_void_p(out.data_ptr() + 4))), ("ldc 62", dict(ldc=N - 2)), ("bias + 4", dict(bias=C.c_void_p(pw.bias.data_ptr() + 4))),
                       ("fp32 out + 8", dict(out=C.c_void_p(out32.data_ptr() + 8), out_f32=1)), ("res1 + 4", dict(res1=C.c_void_p(r1.data_ptr() + 4), ld_res1=N)),
                       ("ld_res1 62", dict(res1=ops._p(r1), ld_res1=N - 2)), ("rowvec + 8", dict(rowvec=C.c_void_p(rv.data_ptr() + 8), ldv=N, rows_per_vec=rpv)),
                       ("ldv 62", dict(rowvec=ops._p(rv), ldv=N - 2, rows_per_vec=rpv))):
        assert lib.vk_gemm_bf16(C.byref(c_desc(**over)), ops._stream()) == EINVAL, what
        COUNT["c"] += 1
    untouched(s, "vk_gemm_bf16 through ctypes")


def test_ff_fused_refuses_bad_operands(ctx):
    ops, st, s = ctx
    M, Cw, H = 40, 320, 128
    x, r1 = good(M, Cw, dtype=st), good(M, Cw, dtype=st, seed=1)
    pin = ops.pack_geglu(rnd(2 * H, Cw, dtype=st, seed=2, scale=Cw ** -0.5), rnd(2 * H, dtype=F32, seed=3))
    pout = _guard.rehome_pack(ops.pack_ff_out(rnd(Cw, H, dtype=st, seed=4, scale=H ** -0.5), rnd(Cw, dtype=F32, seed=5)))
    out = _guard.empty((M, Cw), st)
    launched(s, ops.ff_fused(x, pin, pout, res1=r1), keep=(out,))
    o16 = sixteen_bit_other(st)
    for k, v in bad_views(x, 16, 8, rows=False, other=o16).items():
        refuse(s, lambda: ops.ff_fused(v, pin, pout, out=out), None if k == "col_short" else "x", f"ff_fused x {k}")
    for k, v in bad_views(out, 8, 4, other=o16).items():
        refuse(s, lambda: ops.ff_fused(x, pin, pout, out=v), "out", f"ff_fused out {k}")
    for k, v in bad_views(r1, 8, 4, other=o16).items():
        refuse(s, lambda: ops.ff_fused(x, pin, pout, out=out, res1=v), "res1", f"ff_fused res1 {k}")
    # the C entry point with the same live pointers
    lib = ops._lib.load()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731

    def c_descs(**over):
        g, d = ops.VkGemmDesc(), ops.VkGemmDesc()
        g.A, g.lda, g.amode, g.epi = ptr(x), Cw, ops.AMODE_DENSE, ops.EPI_GEGLU
        g.Wt, g.bias, g.M, g.N, g.K, g.out, g.ldc, g.alpha = ptr(pin.wt), ptr(pin.bias), M, pin.N, pin.K, ptr(out), Cw, 1.0
        d.A, d.lda, d.amode, d.epi = ptr(x), Cw, ops.AMODE_DENSE, ops.EPI_LINEAR
        d.Wt, d.bias, d.M, d.N, d.K, d.out, d.ldc, d.alpha = ptr(pout.wt), ptr(pout.bias), M, pout.N, pout.K, ptr(out), Cw, 1.0
        for k, v in over.items():
            setattr(g if k.startswith("g_") else d, k[2:], v)
        return g, d
    for what, over in (("geglu A + 2", dict(g_A=ptr(x, 2))), ("geglu A + 8", dict(g_A=ptr(x, 8))), ("geglu Wt + 8", dict(g_Wt=ptr(pin.wt, 8))),
                       ("geglu bias + 4", dict(g_bias=ptr(pin.bias, 4))), ("out Wt + 2", dict(o_Wt=ptr(pout.wt, 2))), ("out + 2", dict(o_out=ptr(out, 2))),
                       ("out + 4", dict(o_out=ptr(out, 4))), ("ldc 318", dict(o_ldc=Cw - 2)), ("out bias + 8", dict(o_bias=ptr(pout.bias, 8))),
                       ("res1 + 4", dict(o_res1=ptr(r1, 4), o_ld_res1=Cw)), ("ld_res1 318", dict(o_res1=ptr(r1), o_ld_res1=Cw - 2))):
        g, d = c_descs(**over)
        assert lib.vk_ff_fused_bf16(C.byref(g), C.byref(d), ops._stream()) == EINVAL, what
        COUNT["c"] += 1
    untouched(s, "vk_ff_fused_bf16 through ctypes")


def _flat_skews(t, align):
    """t (dense, any rank) 2 / 4 / 8 bytes off, as views of a larger live arena."""
    item = t.element_size()
    big = _guard.put(torch.zeros(t.numel() + 64, dtype=t.dtype), label="bad operand's arena")
    return {f"skew{k}": big[k // item:k // item + t.numel()].view(t.shape) for k in (2, 4, 8) if k % item == 0 and k % align}


def test_convolutions_refuse_bad_operands(ctx):
    ops, st, s = ctx
    n, H, W, Cin, N = 2, 4, 8, 64, 64
    S = H * W
    o16 = sixteen_bit_other(st)
    x, r1, rv = good(n, S, Cin, dtype=st), good(n * S, N, dtype=st, seed=1), good(n, N, dtype=F32, seed=2)
    out = _guard.empty((n * S, N), st)
    pw = ops.pack_conv3x3(rnd(N, Cin, 3, 3, dtype=st, seed=3, scale=(9 * Cin) ** -0.5), rnd(N, dtype=F32, seed=4))
    launched(s, ops.conv3x3(x, pw, n, H, W, rowvec=rv, res1=r1)[0], keep=(out,))
    for k, v in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.conv3x3(v, pw, n, H, W, out=out), "x", f"conv3x3 x {k}")
    refuse(s, lambda: ops.conv3x3(x, pw, n + 1, H, W, out=out), "x", "conv3x3: n_img overstates x")
    refuse(s, lambda: ops.conv3x3(x, pw, n, H + 1, W, out=out), "x", "conv3x3: H overstates x")
    refuse(s, lambda: ops.conv3x3(x.view(o16), pw, n, H, W, out=out), "x", "conv3x3 x dtype")
    refuse(s, lambda: ops.conv3x3(_guard.put(torch.zeros(n, S, 2 * Cin, dtype=st))[:, :, :Cin], pw, n, H, W, out=out), "x", "conv3x3 x not contiguous")
    for k, v in bad_views(out, 8, 4, other=o16).items():
        refuse(s, lambda: ops.conv3x3(x, pw, n, H, W, out=v), "out", f"conv3x3 out {k}")
    for k, v in bad_views(r1, 8, 4, other=o16).items():
        refuse(s, lambda: ops.conv3x3(x, pw, n, H, W, out=out, res1=v), "res1", f"conv3x3 res1 {k}")
    for k, v in bad_views(rv, 16, 4).items():
        refuse(s, lambda: ops.conv3x3(x, pw, n, H, W, out=out, rowvec=v), "rowvec", f"conv3x3 rowvec {k}")
    # temporal 3x1x1: (b t) = n frames of one clip
    pt = ops.pack_conv_t3(rnd(N, Cin, 3, 1, 1, dtype=st, seed=5, scale=(3 * Cin) ** -0.5), rnd(N, dtype=F32, seed=6))
    launched(s, ops.conv_t3(x, pt, n, S, res1=r1), keep=(out,))
    for k, v in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.conv_t3(v, pt, n, S, out=out), "x", f"conv_t3 x {k}")
    refuse(s, lambda: ops.conv_t3(x, pt, n, S + 8, out=out), None, "conv_t3: S overstates x")
    refuse(s, lambda: ops.conv_t3(x, pt, n + 1, S, out=out), None, "conv_t3: T does not divide the frames")
    halo = good(1, S, Cin, dtype=st, seed=7)
    for k, v in _flat_skews(halo, 16).items():
        refuse(s, lambda: ops.conv_t3(x, pt, n, S, out=out, halo_prev=v), "halo_prev", f"conv_t3 halo_prev {k}")
    for k, v in bad_views(out, 8, 4, other=o16, cols=True).items():
        refuse(s, lambda: ops.conv_t3(x, pt, n, S, out=v), "out", f"conv_t3 out {k}")
    # folded upsample convolution: refused operands only (the small shape is one the library declines anyway; the checks come first)
    pu = ops.pack_upconv2x2(rnd(320, Cin, 3, 3, dtype=st, seed=8, scale=(9 * Cin) ** -0.5), None)
    outu = _guard.empty((n * 4 * S, 320), st)
    for k, v in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.upconv2x2(v, pu, n, H, W, out=outu), "x", f"upconv2x2 x {k}")
    refuse(s, lambda: ops.upconv2x2(x, pu, n + 1, H, W, out=outu), "x", "upconv2x2: n_img overstates x")
    for k, v in bad_views(outu, 8, 4, other=o16).items():
        refuse(s, lambda: ops.upconv2x2(x, pu, n, H, W, out=v), "out", f"upconv2x2 out {k}")
    # 3x3x3
    p3 = ops.pack_conv3d(rnd(N, Cin, 3, 3, 3, dtype=st, seed=9, scale=(27 * Cin) ** -0.5), None)
    launched(s, ops.conv3d(x, p3, n, H, W), keep=(out, outu))
    for k, v in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.conv3d(v, p3, n, H, W, out=out), "x", f"conv3d x {k}")
    refuse(s, lambda: ops.conv3d(x, p3, n, H + 1, W, out=out), "x", "conv3d: H overstates x")


def test_linear_vt_and_rowstats_refuse_bad_operands(ctx):
    ops, st, s = ctx
    n, S, Cw = 2, 16, 64
    o16 = sixteen_bit_other(st)
    x = good(n * S, Cw, dtype=st)
    pw = ops.pack_linear(rnd(Cw, Cw, dtype=st, seed=1, scale=Cw ** -0.5), None)
    launched(s, ops.linear_vt(x, pw, S))
    vt = _guard.empty((n, Cw, S), st)
    for k, v in bad_views(x, 16, 8, rows=False, other=o16).items():
        refuse(s, lambda: ops.linear_vt(v, pw, S, out=vt), "x", f"linear_vt x {k}")
    for k, v in _flat_skews(vt, 8).items():
        refuse(s, lambda: ops.linear_vt(x, pw, S, out=v), "out", f"linear_vt out {k}")
    refuse(s, lambda: ops.linear_vt(x, pw, S + 1, out=vt), None, "linear_vt: S does not divide the rows")
    launched(s, ops.rowstats(x).t, keep=(vt,))
    for k, v in bad_views(x, 16, 8, rows=False, cols=False, other=o16).items():
        refuse(s, lambda: ops.rowstats(v), "x", f"rowstats x {k}")
    lib = ops._lib.load()
    st_out = ops.torch.empty((1, n * S, 2), dtype=F32, device="cuda")
    assert lib.vk_rowstats_bf16(C.c_void_p(x.data_ptr() + 2), ops._p(st_out), n * S, Cw, Cw, ops._stream()) == EINVAL
    assert lib.vk_rowstats_bf16(ops._p(x), C.c_void_p(st_out.data_ptr() + 4), n * S, Cw, Cw, ops._stream()) == EINVAL
    COUNT["c"] += 2
    untouched(s, "vk_rowstats_bf16 through ctypes")


# ------------------------------------------------------------------------------------------------ attention
def test_attention_refuses_bad_operands(ctx):
    ops, st, s = ctx
    n, heads, S = 1, 1, 16
    c = heads * 64
    o16 = sixteen_bit_other(st)
    qkv = good(n * S, 3 * c, dtype=st)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    launched(s, ops.attn_spatial(q, k, v, n, heads, S, v_rows=True))
    dense = good(n * S, c, dtype=st, seed=1)
    for name in ("q", "k", "v"):
        for kind, b in bad_views(dense, 16, 8, other=o16).items():
            args = {"q": q, "k": k, "v": v, name: b}
            refuse(s, lambda: ops.attn_spatial(args["q"], args["k"], args["v"], n, heads, S, v_rows=True), name, f"attn_spatial {name} {kind}")
    refuse(s, lambda: ops.attn_spatial(q, k, v, n, heads, S + 8, v_rows=True), "q", "attn_spatial: S overstates q")
    lib = ops._lib.load()
    o = _guard.empty((n * S, c), st)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    for what, a in (("q + 8", (ptr(q, 8), ptr(k), ptr(v), ptr(o))), ("k + 2", (ptr(q), ptr(k, 2), ptr(v), ptr(o))), ("v + 4", (ptr(q), ptr(k), ptr(v, 4), ptr(o))),
                    ("o + 4", (ptr(q), ptr(k), ptr(v), ptr(o, 4)))):
        assert lib.vk_attn_spatial_qkv_bf16(*a, n, heads, S, 3 * c, 3 * c, 3 * c, c, C.c_float(0.125), ops._stream()) == EINVAL, what
        assert lib.vk_attn_spatial_qkv_log2_bf16(*a, n, heads, S, 3 * c, 3 * c, 3 * c, c, ops._stream()) == EINVAL, what
        COUNT["c"] += 2
    if st is BF16:   # the V^T form exists in the bf16 build only
        vt = good(n, c, S, dtype=st, seed=2)
        launched(s, ops.attn_spatial(q, k, vt, n, heads, S), keep=(o,))
        for kind, b in _flat_skews(vt, 16).items():
            refuse(s, lambda: ops.attn_spatial(q, k, b, n, heads, S), "vt", f"attn_spatial vt {kind}")
        refuse(s, lambda: ops.attn_spatial(q, k, vt[:, :, :S - 8], n, heads, S), "vt", "attn_spatial vt short")
        assert lib.vk_attn_spatial_bf16(ptr(q), ptr(k), ptr(vt, 8), ptr(o), n, heads, S, 3 * c, 3 * c, c, C.c_float(0.125), ops._stream()) == EINVAL
        COUNT["c"] += 1
    # temporal: (B, T, S, heads) = (1, 4, 4, 1)
    B, T, St = 1, 4, 4
    launched(s, ops.attn_temporal(qkv, B, T, St, heads), keep=(o,))
    for kind, b in bad_views(qkv, 16, 8, other=o16).items():
        refuse(s, lambda: ops.attn_temporal(b, B, T, St, heads), "qkv", f"attn_temporal qkv {kind}")
    refuse(s, lambda: ops.attn_temporal(qkv, B, T + 1, St, heads), "qkv", "attn_temporal: T overstates qkv")
    refuse(s, lambda: ops.attn_temporal(qkv, B, T - 1, St, heads), "qkv", "attn_temporal: T understates qkv")
    assert lib.vk_attn_temporal_bf16(ptr(qkv, 2), ptr(o), B, T, St, heads, 3 * c, c, 2 * c, c, C.c_float(0.125), ops._stream()) == EINVAL
    assert lib.vk_attn_temporal_bf16(ptr(qkv), ptr(o, 2), B, T, St, heads, 3 * c, c, 2 * c, c, C.c_float(0.125), ops._stream()) == EINVAL
    # small dense attention, D = 64
    launched(s, ops.attn_small(qkv, n, heads, S, 64), keep=(o,))
    for kind, b in bad_views(qkv, 16, 8, other=o16).items():
        refuse(s, lambda: ops.attn_small(b, n, heads, S, 64), "qkv", f"attn_small qkv {kind}")
    assert lib.vk_attn_small_bf16(ptr(qkv, 8), ptr(o), n, heads, S, 64, 3 * c, c, 2 * c, c, C.c_float(0.125), ops._stream()) == EINVAL
    assert lib.vk_attn_small_bf16(ptr(qkv), ptr(o, 8), n, heads, S, 64, 3 * c, c, 2 * c, c, C.c_float(0.125), ops._stream()) == EINVAL
    COUNT["c"] += 4
    # row softmax
    x = good(8, 64, dtype=F32, seed=3)
    launched(s, ops.softmax_rows(x), keep=(o,))
    y = _guard.empty((8, 64), st)
    for kind, b in bad_views(x, 16, 4, cols=False, rows=False).items():
        refuse(s, lambda: ops.softmax_rows(b, out=y), "x", f"softmax_rows x {kind}")
    for kind, b in bad_views(y, 8, 4, other=o16).items():
        refuse(s, lambda: ops.softmax_rows(x, out=b), "out", f"softmax_rows out {kind}")
    assert lib.vk_softmax_rows_f32_bf16(ptr(x, 4), ptr(y), 8, 64, 64, 64, ops._stream()) == EINVAL
    assert lib.vk_softmax_rows_f32_bf16(ptr(x), ptr(y, 4), 8, 64, 64, 64, ops._stream()) == EINVAL
    COUNT["c"] += 2
    untouched(s, "attention entry points through ctypes")


# ------------------------------------------------------------------------------------------------ norms, layout, sampler
def test_norms_refuse_bad_operands(ctx):
    ops, st, s = ctx
    n, S, Cw = 2, 32, 64
    o16 = sixteen_bit_other(st)
    x = good(n, S, Cw, dtype=st)
    gamma, beta = good(Cw, dtype=F32, seed=1), good(Cw, dtype=F32, seed=2)
    launched(s, ops.groupnorm(x, gamma, beta, 1e-5, True))
    affine = {"gamma short": (gamma[:Cw - 1], beta, "gamma"), "beta short": (gamma, beta[:Cw - 8], "beta"), "gamma 16-bit": (gamma.to(BF16), beta, "gamma"),
              "beta 16-bit": (gamma, beta.to(BF16), "beta"), "gamma strided": (_guard.put(torch.zeros(2 * Cw))[::2], beta, "gamma")}
    for kind, b in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.groupnorm(b, gamma, beta, 1e-5, True), "x", f"groupnorm x {kind}")
    refuse(s, lambda: ops.groupnorm(x.view(o16), gamma, beta, 1e-5, True), "x", "groupnorm x dtype")
    for kind, (g_, b_, name) in affine.items():
        refuse(s, lambda: ops.groupnorm(x, g_, b_, 1e-5, True), name, f"groupnorm {kind}")
    out = _guard.empty((n, S, Cw), st)
    for kind, b in _flat_skews(out, 16).items():
        refuse(s, lambda: ops.groupnorm(x, gamma, beta, 1e-5, True, out=b), "out", f"groupnorm out {kind}")
    refuse(s, lambda: ops.groupnorm(x, gamma, beta, 1e-5, True, out=out[:, :S - 1]), "out", "groupnorm out short")
    # concat form: 32 + 32 channels
    a, b2 = good(n, S, 32, dtype=st, seed=3), good(n, S, 32, dtype=st, seed=4)
    launched(s, ops.groupnorm_cat(a, b2, gamma, beta, 1e-5, False), keep=(out,))
    for kind, b in _flat_skews(a, 16).items():
        refuse(s, lambda: ops.groupnorm_cat(b, b2, gamma, beta, 1e-5, False), "a", f"groupnorm_cat a {kind}")
        refuse(s, lambda: ops.groupnorm_cat(a, b, gamma, beta, 1e-5, False), "b", f"groupnorm_cat b {kind}")
    refuse(s, lambda: ops.groupnorm_cat(a, b2, gamma[:32], beta, 1e-5, False), "gamma", "groupnorm_cat gamma short")
    # sharded form (identity all-reduce)
    launched(s, ops.groupnorm_sharded(x, gamma, beta, 1e-5, False, 1, lambda t: t, (Cw // 32) * S), keep=(out,))
    for kind, b in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.groupnorm_sharded(b, gamma, beta, 1e-5, False, 1, lambda t: t, (Cw // 32) * S), "x", f"groupnorm_sharded x {kind}")
    refuse(s, lambda: ops.groupnorm_sharded(x, gamma, beta[:Cw - 1], 1e-5, False, 1, lambda t: t, (Cw // 32) * S), "beta", "groupnorm_sharded beta short")
    # LayerNorm with a per-image pre-add
    av = good(n, Cw, dtype=F32, seed=5)
    launched(s, ops.layernorm(x, gamma, beta, addvec=av, rows_per_vec=S, want_sum=True), keep=(out,))
    for kind, b in _flat_skews(x, 16).items():
        refuse(s, lambda: ops.layernorm(b, gamma, beta), "x", f"layernorm x {kind}")
    for kind, (g_, b_, name) in affine.items():
        refuse(s, lambda: ops.layernorm(x, g_, b_), name, f"layernorm {kind}")
    for kind, b in bad_views(av, 4, 1).items():
        if kind.startswith("skew") or kind == "ld":
            continue
        refuse(s, lambda: ops.layernorm(x, gamma, beta, addvec=b, rows_per_vec=S), "addvec", f"layernorm addvec {kind}")
    refuse(s, lambda: ops.layernorm(x.view(o16), gamma, beta), "x", "layernorm x dtype")
    # the C entry points
    lib = ops._lib.load()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    ws = ops.torch.empty((n + n * ((S + 31) // 32)) * 64, dtype=F32, device="cuda")
    for what, xy in (("x + 2", (ptr(x, 2), ptr(out))), ("x + 8", (ptr(x, 8), ptr(out))), ("y + 8", (ptr(x), ptr(out, 8)))):
        assert lib.vk_groupnorm_silu_bf16(*xy, ptr(gamma), ptr(beta), ptr(ws), n, S, Cw, 1, C.c_float(1e-5), 1, ops._stream()) == EINVAL, what
        assert lib.vk_layernorm_bf16(*xy, None, ptr(gamma), ptr(beta), None, n * S, Cw, 0, 0, C.c_float(1e-5), ops._stream()) == EINVAL, what
        COUNT["c"] += 2
    assert lib.vk_groupnorm_silu_cat_bf16(ptr(a, 8), ptr(b2), ptr(out), ptr(gamma), ptr(beta), ptr(ws), n, S, 32, 32, 1, C.c_float(1e-5), 0, ops._stream()) == EINVAL
    assert lib.vk_groupnorm_silu_cat_bf16(ptr(a), ptr(b2, 8), ptr(out), ptr(gamma), ptr(beta), ptr(ws), n, S, 32, 32, 1, C.c_float(1e-5), 0, ops._stream()) == EINVAL
    COUNT["c"] += 2
    untouched(s, "norm entry points through ctypes")


def test_layout_and_sampler_ops_refuse_bad_operands(ctx):
    ops, st, s = ctx
    n, S = 2, 32
    o16 = sixteen_bit_other(st)
    a, b = good(n, S, 64, dtype=st), good(n, S, 32, dtype=st, seed=1)
    launched(s, ops.concat_channels(a, b))
    for kind, v in _flat_skews(a, 16).items():
        refuse(s, lambda: ops.concat_channels(v, b), "a", f"concat_channels a {kind}")
    for kind, v in _flat_skews(b, 16).items():
        refuse(s, lambda: ops.concat_channels(a, v), "b", f"concat_channels b {kind}")
    refuse(s, lambda: ops.concat_channels(a.view(o16), b), "a", "concat_channels a dtype")
    refuse(s, lambda: ops.concat_channels(a, b[:1]), None, "concat_channels: b one image short")
    lib = ops._lib.load()
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    cat = _guard.empty((n, S, 96), st)
    for what, args in (("a + 2", (ptr(a, 2), ptr(b), ptr(cat))), ("b + 8", (ptr(a), ptr(b, 8), ptr(cat))), ("out + 4", (ptr(a), ptr(b), ptr(cat, 4)))):
        assert lib.vk_concat_channels_bf16(*args, n * S, 64, 32, ops._stream()) == EINVAL, what
        COUNT["c"] += 1
    # NCHW <-> tokens
    T, H, W = 2, 4, 8
    x4 = good(T, 4, H, W, dtype=F32, seed=2)
    launched(s, ops.nchw_to_tokens(x4, 8), keep=(cat,))
    refuse(s, lambda: ops.nchw_to_tokens(x4.to(BF16), 8), "x", "nchw_to_tokens x dtype")
    tok = _guard.empty((T, H * W, 8), st)
    assert lib.vk_nchw_to_tokens_bf16(ptr(x4), ptr(tok, 8), T, 4, H * W, 8, ops._stream()) == EINVAL
    assert lib.vk_nchw_to_tokens_bf16(ptr(x4, 2), ptr(tok), T, 4, H * W, 8, ops._stream()) == EINVAL
    COUNT["c"] += 2
    t32 = good(T * H * W, 8, dtype=F32, seed=3)
    launched(s, ops.tokens_to_nchw(t32, T, 4, H, W), keep=(cat, tok))
    for kind, v in bad_views(t32, 4, 1, cols=False).items():
        if kind.startswith("skew") or kind == "ld":
            continue
        refuse(s, lambda: ops.tokens_to_nchw(v, T, 4, H, W), "x", f"tokens_to_nchw x {kind}")
    refuse(s, lambda: ops.tokens_to_nchw(t32, T + 1, 4, H, W), "x", "tokens_to_nchw: n_img overstates x")
    refuse(s, lambda: ops.tokens_to_nchw(t32, T, 12, H, W), "x", "tokens_to_nchw: C overstates x")
    # timestep embeddings and the embedding combine
    ts = good(T, dtype=F32, seed=4)
    launched(s, ops.timestep_embedding(ts, 64), keep=(cat, tok))
    refuse(s, lambda: ops.timestep_embedding(ts.to(BF16), 64), "t", "timestep_embedding t dtype")
    e1, e2, e3 = (good(T, 64, dtype=F32, seed=k) for k in (5, 6, 7))
    mk = good(T, dtype=F32, seed=8)
    launched(s, ops.emb_combine(e1, e2, e3, mk), keep=(cat, tok))
    refuse(s, lambda: ops.emb_combine(e1[:1], e2, e3, mk), "a", "emb_combine a short")
    refuse(s, lambda: ops.emb_combine(e1, e2, e3.to(BF16), mk), "c", "emb_combine c dtype")
    refuse(s, lambda: ops.emb_combine(e1, e2, e3, mk[:1]), "mask", "emb_combine mask short")
    assert lib.vk_emb_combine(ptr(e1, 2), ptr(e2), ptr(e3), ptr(mk), ptr(t32), None, T, 64, ops._stream()) == EINVAL
    assert lib.vk_timestep_embedding_f32(ptr(ts, 2), ptr(t32), T, 64, C.c_float(10000.0), ops._stream()) == EINVAL
    COUNT["c"] += 2
    # sampler
    xs = _guard.scratch(x4, "sampler x")
    cf, mask = good(T, 4, H, W, dtype=F32, seed=9), good(T, dtype=F32, seed=10)
    cu, cc = good(T, 4, H, W, dtype=F32, seed=11), good(T, 4, H, W, dtype=F32, seed=12)
    launched(s, ops.sampler_prepare(xs, cf, mask, cu, cc, 8, 0.5, False), keep=(cat, tok))
    refuse(s, lambda: ops.sampler_prepare(xs, cf[:1], mask, cu, cc, 8, 0.5, True), "cond_frame", "sampler_prepare cond_frame short")
    refuse(s, lambda: ops.sampler_prepare(xs, cf, mask[:1], cu, cc, 8, 0.5, True), "mask", "sampler_prepare mask short")
    refuse(s, lambda: ops.sampler_prepare(xs, cf, mask, cu.to(BF16), cc, 8, 0.5, True), "concat_uc", "sampler_prepare concat_uc dtype")
    refuse(s, lambda: ops.sampler_prepare(xs, cf, mask, cu, cc[:, :, :H - 1], 8, 0.5, True), "concat_c", "sampler_prepare concat_c short")
    net = good(2 * T, H * W, 8, dtype=F32, seed=13)
    scale = good(T, dtype=F32, seed=14)
    launched(s, ops.sampler_update(xs, net, scale, 1.0, 0.5, 2.0, 1.0), keep=(cat, tok))
    refuse(s, lambda: ops.sampler_update(xs, net[:T], scale, 1.0, 0.5, 2.0, 1.0), "net_out", "sampler_update net_out: one guidance half short")
    refuse(s, lambda: ops.sampler_update(xs, net, scale[:1], 1.0, 0.5, 2.0, 1.0), "scale", "sampler_update scale short")
    refuse(s, lambda: ops.sampler_update(xs, net.to(BF16), scale, 1.0, 0.5, 2.0, 1.0), "net_out", "sampler_update net_out dtype")
    nin = _guard.empty((2 * T, H * W, 8), st)
    assert lib.vk_sampler_prepare(ptr(xs), ptr(cf), ptr(mask), ptr(cu), ptr(cc), ptr(nin, 8), T, H * W, 8, C.c_float(0.5), 0, ops._stream()) == EINVAL
    assert lib.vk_sampler_update(ptr(xs), ptr(net, 2), ptr(scale), T, H * W, 8, C.c_float(1.0), C.c_float(0.5), C.c_float(2.0), C.c_float(1.0), ops._stream()) == EINVAL
    COUNT["c"] += 2
    untouched(s, "layout and sampler entry points through ctypes")


def test_a_misaligned_weight_pack_is_refused_when_it_is_made(ctx):
    ops, st, s = ctx
    big = _guard.put(torch.zeros(320 * 64 + 64, dtype=st))
    with pytest.raises(ValueError, match=r"^PackedWeight\.wt: "):
        ops.PackedWeight(big[4:4 + 320 * 64].view(320, 64), None, 64, 64)
    COUNT["python"] += 1
    untouched(s, "PackedWeight")
