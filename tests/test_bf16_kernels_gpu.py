"""Per-kernel parity of the default bf16-storage build (libvista_hip.so) against float64 references of the very bf16 values the kernels are handed,
at format-derived bounds: the case table of tests/_bf16_cases.py (tests/_kernel_cases.py: make_cases(torch.bfloat16)) under every forced block tile,
and the bf16 twins of the hand-written tests of tests/test_f16_kernels_gpu.py that do not depend on the storage type. ops.storage(torch.bfloat16)
around every test, so the module also runs in a VISTA_ACT_DTYPE=fp16 process. Bound A: derived from the number format (u = 2^-8); bounds B and
LN: measured on the MI355X + 25 %, B capped at 1.5 x the output-rounding floor (profiles/bf16_kernel_parity.txt); tests/test_bf16_bounds_cpu.py
proves that the bounds separate a correct output from a truncated, bit-cut, K-dropped or double-rounded one -- which tests/test_kernels_gpu.py:
close() (1.6e-2 |ref| + 2e-2 rms) does not. Every test prints its figures (`BF16PARITY ...`) before it asserts."""
import os

import pytest
import torch

from tests import _bf16_cases as fc
from tests import _parity_edges as edges

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(autouse=True)
def bf16_storage():
    from vista_amd import build, ops
    if not os.path.exists(build.LIB):
        pytest.fail("vista_amd/lib/libvista_hip.so is missing: __graft_entry__.build() links both storage variants")
    saved = (ops.TILE_CFG, ops.SPLITK_WS_BYTES)
    try:
        with ops.storage(BF16):
            yield ops
    finally:
        ops.TILE_CFG, ops.SPLITK_WS_BYTES = saved


# ------------------------------------------------------------------------------------------------ the case table
_REF = {}


def _inputs_and_ref(case):
    """Computed once per case and shared by its tile variants; never modified."""
    if case.name not in _REF:
        i = case.build()
        _REF[case.name] = (i, case.ref(i))
    return _REF[case.name]


def _judge(case, outs, refs, tag):
    fails = []
    assert len(outs) == len(refs) == len(case.specs)
    for k, (spec, out, ref) in enumerate(zip(case.specs, outs, refs)):
        ok, fig = fc.check_any(spec, out, ref, f"{case.name}[{k}]")
        print(f"BF16PARITY {case.name}[{k}] {spec[0]} {tag} " + " ".join(f"{a}={b:.4g}" if isinstance(b, float) else f"{a}={b}" for a, b in fig.items()))
        if not ok:
            fails.append((k, spec[0], fig))
    assert not fails, f"{case.name} {tag}: {fails}"


_PARAMS = [pytest.param(c, cfg, id=f"{c.name}-cfg{cfg}") for c in fc.CASES for cfg in c.cfgs]


@pytest.mark.parametrize("case,cfg", _PARAMS)
def test_case(case, cfg, bf16_storage):
    """One case of tests/_bf16_cases.py (GEMM-family cases: under every forced block-tile variant of the case; a variant that does not take a
    problem falls back to the launcher's choice) against its float64 reference. Bounds B and LN: measured on the MI355X + 25 %, every pair in
    tests/_kernel_cases.py (B_BOUNDS_BF16, LN_BOUNDS_BF16) and in profiles/bf16_kernel_parity.txt."""
    ops = bf16_storage
    i, refs = _inputs_and_ref(case)
    ops.TILE_CFG = cfg
    outs = case.run(ops, fc.to_device(i, "cuda"))
    ops.TILE_CFG = 0
    _judge(case, outs, refs, f"cfg{cfg}")


# ------------------------------------------------------------------------------------------------ helpers of the hand-written tests
def rnd(*shape, scale=1.0, seed=0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _norm(Cc, seed=7):
    g = torch.Generator().manual_seed(seed)
    return fc.Norm((1 + 0.2 * torch.randn(Cc, generator=g)).cuda(), (0.1 * torch.randn(Cc, generator=g)).cuda())


def _check_stats(st, out):
    """RowStats slabs summed over parts == float64 (sum, sum of squares) of the kernel's own bf16 output rows (tolerance of tests/test_kernels_gpu.py)."""
    o = out.double()
    got = st.t.sum(0).double()
    ref = torch.stack([o.sum(1), o.pow(2).sum(1)], 1)
    tol = 2e-5 * torch.stack([o.abs().sum(1), o.pow(2).sum(1)], 1) + 1e-6
    worst = ((got - ref).abs() / tol).max().item()
    print(f"BF16PARITY rowstats worst/tol={worst:.3g}")
    assert worst <= 1.0, f"row sums off: {worst:.3g} of the tolerance"


def _forced(ops, cfg, fn):
    ops.TILE_CFG = cfg
    try:
        return fn()
    finally:
        ops.TILE_CFG = 0


# ------------------------------------------------------------------------------------------------ halo frames
def test_conv_t3_halo_frames_are_bitwise_the_slice_of_the_whole_clip(bf16_storage):
    ops = bf16_storage
    B, T, S, Cc = 2, 8, 40, 128
    x = rnd(B * T, S, Cc)
    pw = ops.pack_conv_t3(rnd(Cc, Cc, 3, 1, 1, scale=(3 * Cc) ** -0.5, seed=1), rnd(Cc, seed=2).float())
    full = ops.conv_t3(x, pw, T, S).view(B, T, S, Cc)
    x4 = x.view(B, T, S, Cc)
    for t0, t1 in ((0, 3), (3, 7), (7, 8)):
        loc = x4[:, t0:t1].reshape(B * (t1 - t0), S, Cc).contiguous()
        prev = x4[:, t0 - 1].contiguous() if t0 > 0 else None
        nxt = x4[:, t1].contiguous() if t1 < T else None
        out = ops.conv_t3(loc, pw, t1 - t0, S, halo_prev=prev, halo_next=nxt).view(B, t1 - t0, S, Cc)
        assert torch.equal(out, full[:, t0:t1]), (t0, t1)


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("name", ["splitk_dense_4032x1280x5120", "splitk_conv3x3_50x9x16x1280"])
def test_splitk_with_and_without_workspace(name, bf16_storage):
    """Both runs within bound A / F32; the 16-bit results at most one bf16 ulp apart (another fp32 summation order); the fp32 form repeatable
    bit for bit and NOT equal to the plain kernel's -- which proves that the split path ran."""
    ops = bf16_storage
    case = fc.BY_NAME[name]
    i, refs = _inputs_and_ref(case)
    ig = fc.to_device(i, "cuda")
    split = case.run(ops, ig)
    again = case.run(ops, ig)
    ops.SPLITK_WS_BYTES = 0
    plain = case.run(ops, ig)
    _judge(case, split, refs, "split")
    _judge(case, plain, refs, "plain")
    # one bf16 ulp apart: both fp32 values lie within the F32 bound of the reference (asserted above), i.e. within 4e-5 (|ref| + rms) of each
    # other, and their roundings then differ by at most that plus one ulp of the larger one
    s16, p16, ref = split[0].double().cpu(), plain[0].double().cpu(), refs[0].double()
    ulp = torch.maximum(s16.abs(), p16.abs()).clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -7
    tol = ulp + 4e-5 * (ref.abs() + ref.pow(2).mean().sqrt())
    apart = ((s16 - p16).abs() / tol).max().item()
    print(f"BF16PARITY {name} split-vs-plain worst/(ulp + fp32 slack)={apart:.3g} differing={int((split[0] != plain[0]).sum())}")
    assert apart <= 1.0
    assert torch.equal(split[1], again[1]) and torch.equal(split[0], again[0]), "split-K must be repeatable"
    assert not torch.equal(split[1], plain[1]), "the split-K path was not taken (its fp32 summation order differs from the plain kernel's)"


# ------------------------------------------------------------------------------------------------ bitwise equalities between kernels
def _kind_fn(ops, kind, n, H, W, Cc):
    S = H * W
    M = n * S
    x = rnd(M, Cc)
    x3 = x.view(n, S, Cc)
    res = rnd(M, Cc, seed=3)
    rv = rnd(n, Cc, seed=5).float()
    if kind == "dense+res+stats":
        pw = ops.pack_linear(rnd(Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(Cc, seed=2).float())
        return lambda **kw: ops.linear(x, pw, res1=res, rowvec=rv, rows_per_vec=S, emit_stats=True, **kw)
    if kind == "dense_strided_A":
        xs = rnd(M, 3 * Cc, seed=11)[:, Cc:2 * Cc]
        pw = ops.pack_linear(rnd(Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(Cc, seed=2).float())
        return lambda **kw: ops.linear(xs, pw, res1=res, **kw)
    if kind == "dense_K4N+res+stats":
        h4 = rnd(M, 4 * Cc, seed=9)
        pw = ops.pack_linear(rnd(Cc, 4 * Cc, scale=(4 * Cc) ** -0.5, seed=1), rnd(Cc, seed=2).float())
        return lambda **kw: ops.linear(h4, pw, res1=res, rowvec=rv, rows_per_vec=S, emit_stats=True, **kw)
    if kind == "qkv_lnfold":
        pw = ops.pack_linear(rnd(3 * Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(3 * Cc, seed=2).float(), ln=_norm(Cc))
        st = ops.rowstats(x)
        return lambda **kw: ops.linear(x, pw, ln=st, **kw)
    if kind == "ff_out+blend":
        h4 = rnd(M, 4 * Cc, seed=9)
        pw = ops.pack_linear(rnd(Cc, 4 * Cc, scale=(4 * Cc) ** -0.5, seed=1), rnd(Cc, seed=2).float())
        return lambda **kw: ops.linear(h4, pw, res1=res, alpha=0.4, res2=x, rowvec2=rv, beta=0.6, rows_per_vec=S, **kw)
    if kind == "geglu_lnfold":
        pw = ops.pack_geglu(rnd(8 * Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(8 * Cc, seed=2).float(), ln=_norm(Cc))
        st = ops.rowstats(x)
        return lambda **kw: ops.linear(x, pw, ln=st, **kw)
    if kind.startswith("conv3x3"):
        pw = ops.pack_conv3x3(rnd(Cc, Cc, 3, 3, scale=(9 * Cc) ** -0.5, seed=1), rnd(Cc, seed=2).float())
        if kind == "conv3x3+emb+res":
            return lambda **kw: ops.conv3x3(x3, pw, n, H, W, rowvec=rv, res1=x3, **kw)[0]
        if kind == "conv3x3_ups2":
            return lambda **kw: ops.conv3x3(x3, pw, n, H, W, ups=2, rowvec=rv, **kw)[0]
        return lambda **kw: ops.conv3x3(x3, pw, n, H, W, stride=2, **kw)[0]
    pw = ops.pack_conv_t3(rnd(Cc, Cc, 3, 1, 1, scale=(3 * Cc) ** -0.5, seed=1), rnd(Cc, seed=2).float())
    return lambda **kw: ops.conv_t3(x3, pw, n, S, res2=x3, alpha=0.3, beta=1.0, **kw)


def _same_bits(a, b, what):
    if isinstance(a, tuple):
        (a, sa), (b, sb) = a, b
        assert sa.parts == sb.parts and torch.equal(sa.t, sb.t), f"{what}: row-sum slabs differ"
        _check_stats(sa, a)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


DENSE_KINDS = ["dense+res+stats", "dense_strided_A", "qkv_lnfold", "ff_out+blend", "geglu_lnfold"]
CONV_KINDS = ["conv3x3+emb+res", "conv3x3_stride2", "conv3x3_ups2", "conv_t3+blend"]
# (n, H, W, C): ragged last tile, tiles spanning 3-4 images. The stride-2 conv needs even H, W: it runs at (5, 10, 12, 640) in the second shape.
BITWISE_SHAPES = [(3, 20, 24, 320), (5, 9, 13, 640)]


@pytest.mark.parametrize("kind", DENSE_KINDS + CONV_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", BITWISE_SHAPES)
def test_pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(kind, n, H, W, Cc, bf16_storage):
    """tile_cfg 7 (gemm_pipe.hip) == tile_cfg 4, outputs and row-sum slabs."""
    ops = bf16_storage
    if kind == "conv3x3_stride2" and (H % 2 or W % 2):
        H, W = 10, 12
    fn = _kind_fn(ops, kind, n, H, W, Cc)
    _same_bits(_forced(ops, 7, fn), _forced(ops, 4, fn), f"{kind} cfg 7 vs 4")


@pytest.mark.parametrize("kind", DENSE_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", BITWISE_SHAPES)
def test_two_per_cu_kernel_is_bitwise_the_pipelined_kernel(kind, n, H, W, Cc, bf16_storage):
    """tile_cfg bit 4 (gemm_pipe2.hip) == tile_cfg 7 for the dense kinds."""
    ops = bf16_storage
    fn = _kind_fn(ops, kind, n, H, W, Cc)
    _same_bits(_forced(ops, 16, fn), _forced(ops, 7, fn), f"{kind} cfg 16 vs 7")


@pytest.mark.parametrize("kind", ["qkv_lnfold", "dense_K4N+res+stats", "conv3x3+emb+res", "conv_t3+blend"])
def test_tail_split_is_bitwise_the_single_launch(kind, bf16_storage):
    """tile_cfg bit 6 at (29, 36, 64), C = 320: 261 row tiles of 256 -> whole rounds on the pipelined kernel + the rest as 128x160 tiles."""
    ops = bf16_storage
    n, H, W, Cc = 29, 36, 64, 320
    N = 3 * Cc if kind == "qkv_lnfold" else Cc
    tiles = ((n * H * W + 255) // 256) * (N // 320)
    assert tiles // 256 >= 1 and 0 < tiles % 256 <= 0.4 * 256   # a shape the rule splits
    fn = _kind_fn(ops, kind, n, H, W, Cc)
    _same_bits(_forced(ops, 64, fn), _forced(ops, 7, fn), f"{kind} tail split vs single launch")


# ------------------------------------------------------------------------------------------------ the streaming GEMM, forced
@pytest.mark.parametrize("kind", ["plain", "res+rowvec+stats", "qkv_lnfold"])
def test_gemm_stream_forced(kind, bf16_storage):
    """tile_cfg 6 at M = 32 * 300 + 7 against float64 (bound A) and bitwise against the tiled kernel."""
    ops = bf16_storage
    M, S, Cc = 32 * 300 + 7, 288, 320
    g = fc.G(31)
    N = 3 * Cc if kind.startswith("qkv") else Cc
    x, w, b, res = fc.r16(g, M, Cc), fc.r16(g, N, Cc, scale=Cc ** -0.5), fc.r32(g, N), fc.r16(g, M, Cc)
    rv = fc.r32(g, (M + S - 1) // S, Cc)
    gamma, beta = fc.r32(g, Cc, scale=0.2, shift=1.0), fc.r32(g, Cc, scale=0.1)
    kw, ln = {}, None
    if kind.startswith("qkv"):
        ref = fc.ln_fold_ref(x, w, b, gamma, beta)
        pw = ops.pack_linear(w.cuda(), b.cuda(), ln=fc.Norm(gamma.cuda(), beta.cuda()))
        ln = ops.rowstats(x.cuda())
    else:
        ref = fc.d(x) @ fc.d(w).t() + fc.d(b)
        pw = ops.pack_linear(w.cuda(), b.cuda())
        if kind != "plain":
            ref = ref + fc.d(res) + fc.d(rv).repeat_interleave(S, 0)[:M]
            kw.update(res1=res.cuda(), rowvec=rv.cuda(), rows_per_vec=S, emit_stats=True)
    xg = x.cuda()
    o6 = _forced(ops, 6, lambda: ops.linear(xg, pw, ln=ln, **kw))
    o4 = _forced(ops, 4, lambda: ops.linear(xg, pw, ln=ln, **kw))
    if isinstance(o6, tuple):
        (o6, s6), (o4, s4) = o6, o4
        assert s6.parts == 1, "the streaming kernel combines its waves' row sums into one slab"
        _check_stats(s6, o6)
    assert torch.equal(o6, o4), "streaming and tiled kernels must agree bit for bit"
    ok, fig = fc.check(("A", BF16), o6, ref)
    print(f"BF16PARITY gemm_stream_{kind}[0] {fig}")
    assert ok, (kind, fig)


# ------------------------------------------------------------------------------------------------ statistics outputs
@pytest.mark.parametrize("rows,Cc", [(257, 640), (64, 64)])
def test_rowstats_are_the_sums_of_the_input(rows, Cc, bf16_storage):
    ops = bf16_storage
    x = (rnd(rows, Cc).float() + 2.0).to(BF16)
    st = ops.rowstats(x)
    assert st.parts == 1
    _check_stats(st, x)
    big = rnd(rows, 2 * Cc, seed=3)
    _check_stats(ops.rowstats(big[:, Cc:]), big[:, Cc:])   # strided rows


@pytest.mark.parametrize("cfg", fc.TILE_CFGS)
def test_emit_stats_are_the_sums_of_the_rounded_output(cfg, bf16_storage):
    """The row sums a GEMM epilogue emits are those of its own bf16-ROUNDED output (what the next LayerNorm fold reads), not of the fp32 value."""
    ops = bf16_storage
    M, N, K = 777, 320, 320
    x = rnd(M, K)
    pw = ops.pack_linear(rnd(N, K, scale=K ** -0.5, seed=1), rnd(N, seed=2).float())
    r1, rv = rnd(M, N, seed=4), rnd(3, N, seed=5).float()
    out, st = _forced(ops, cfg, lambda: ops.linear(x, pw, res1=r1, rowvec=rv, rows_per_vec=(M + 2) // 3, emit_stats=True))
    assert out.dtype is BF16 and st.M == M and st.t.shape == (st.parts, M, 2)
    _check_stats(st, out)


def test_conv_epilogue_groupnorm_statistics(bf16_storage):
    """One shape of tests/test_gnstat_gpu.py ("conv+res", C = 320, 3 images of 16x16, pipelined kernel): the folded partials equal float64 group
    sums of the convolution's own bf16 output, to that file's tolerance (2e-5 of sqrt(count * sum of squares) / of the sum of squares)."""
    from vista_amd import _lib
    ops = bf16_storage
    assert ops.GN_EPI
    Cc, n, H, W = 320, 3, 16, 16
    S = H * W
    x, res = rnd(n, S, Cc, seed=3), rnd(n, S, Cc, seed=5)
    pw = ops.pack_conv3x3(rnd(Cc, Cc, 3, 3, scale=(9 * Cc) ** -0.5, seed=6), rnd(Cc, seed=7).float())
    base = _forced(ops, 7, lambda: ops.conv3x3(x, pw, n, H, W, res1=res)[0])
    gn = ops.GnPartials()
    out = _forced(ops, 7, lambda: ops.conv3x3(x, pw, n, H, W, res1=res, gn=gn)[0])
    assert gn.t is not None and gn.nchunks == S // 64 and torch.equal(out, base)
    sums = torch.empty(n * 64, dtype=F32, device="cuda")
    _lib.check(_lib.load().vk_groupnorm_finalize_partials(ops._p(gn.t.clone()), ops._p(sums), n, gn.nchunks, 1, ops._stream()), "vk_groupnorm_finalize_partials")
    got = sums.view(n, 64).double().cpu()
    o = out.view(n, S, 32, Cc // 32).double().cpu()
    ref_s, ref_q = o.sum((1, 3)), o.pow(2).sum((1, 3))
    count = (Cc // 32) * S
    es = ((got[:, :32] - ref_s).abs() / ((count * ref_q).sqrt() + 1e-6)).max().item()
    eq = ((got[:, 32:] - ref_q).abs() / (ref_q + 1e-6)).max().item()
    print(f"BF16PARITY gnstat sums={es:.3g} sumsq={eq:.3g} bound=2e-5")
    assert es <= 2e-5 and eq <= 2e-5
    # and the norm from those partials against float64 GroupNorm + SiLU of that output (bound A)
    gamma, beta = 1.0 + 0.2 * rnd(Cc, seed=10).float(), 0.2 * rnd(Cc, seed=11).float()
    got_y = ops.groupnorm(out.view(n, S, Cc), gamma, beta, 1e-5, True, gn=gn)
    assert gn.t is None
    y = torch.nn.functional.silu(torch.nn.functional.group_norm(out.view(n, S, Cc).double().cpu().transpose(1, 2), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5))
    ok, fig = fc.check(("A", BF16), got_y, y.transpose(1, 2))
    print(f"BF16PARITY groupnorm_from_partials {fig}")
    assert ok, fig


# ------------------------------------------------------------------------------------------------ norms: bitwise relation
@pytest.mark.parametrize("name", ["groupnorm_cat_3x144x640+320", "groupnorm_cat_2x100x64+128"])
def test_groupnorm_cat_is_bitwise_groupnorm_of_the_concat(name, bf16_storage):
    ops = bf16_storage
    i = fc.to_device(_inputs_and_ref(fc.BY_NAME[name])[0], "cuda")
    silu = name.startswith("groupnorm_cat_3")
    got = ops.groupnorm_cat(i.a, i.b, i.gamma, i.beta, 1e-5, silu)
    want = ops.groupnorm(torch.cat([i.a, i.b], 2).contiguous(), i.gamma, i.beta, 1e-5, silu)
    assert torch.equal(got, want), "same arithmetic in the same order: bitwise equal"


# ------------------------------------------------------------------------------------------------ temporal attention: launch-geometry edges
def test_attn_temporal_one_key_is_bitwise_v(bf16_storage):
    edges.temporal_one_key_is_bitwise_v(bf16_storage, BF16)


def test_attn_temporal_narrow_store_is_bitwise_the_wide_store(bf16_storage):
    edges.temporal_narrow_store_is_bitwise_the_wide_store(bf16_storage, BF16)


# ------------------------------------------------------------------------------------------------ GroupNorm at a large mean: the raw-sum routes
@pytest.mark.parametrize("route", ["conv_epilogue_partials", "sharded_identity_allreduce"])
def test_groupnorm_large_mean_routes(route, bf16_storage):
    """|group mean| = 10 .. 30 std on (2, 48 x 48, 320), put there by a conv3x3 bias (tests/_kernel_cases.py: gn_route_inputs): GroupNorm of the
    conv's stored output with statistics (a) from the conv's own epilogue partials, (b) from groupnorm_sharded with an identity all-reduce,
    against float64 group_norm of that stored tensor, bound A. Both routes keep raw fp32 (sum, sum of squares); a plain-torch emulation of such
    sums stays within 0.8 x the tolerance at this range (tests/test_bf16_bounds_cpu.py)."""
    ops = bf16_storage
    i = fc.gn_route_inputs()
    n, H, W, Cc = i.n, i.H, i.W, i.C
    ig = fc.to_device(i, "cuda")
    pw = ops.pack_conv3x3(ig.w, ig.b)
    gn = ops.GnPartials() if route == "conv_epilogue_partials" else None
    y = _forced(ops, 7, lambda: ops.conv3x3(ig.x, pw, n, H, W, gn=gn)[0]).view(n, H * W, Cc)
    if gn is not None:
        assert ops.GN_EPI and gn.t is not None and gn.nchunks == H * W // 64, "the conv's epilogue did not emit its GroupNorm partials"
        got = ops.groupnorm(y, ig.gamma, ig.beta, 1e-5, False, gn=gn)
        assert gn.t is None
    else:
        got = ops.groupnorm_sharded(y, ig.gamma, ig.beta, 1e-5, False, 1, lambda sums: None, (Cc // 32) * H * W)
    ok, fig = fc.check(("A", BF16), got, fc.gn_route_ref(y.cpu(), i.gamma, i.beta))
    print(f"BF16PARITY groupnorm_large_mean_{route}[0] A cfg0 " + " ".join(f"{a}={b:.4g}" if isinstance(b, float) else f"{a}={b}" for a, b in fig.items()))
    assert ok, fig
