"""Per-kernel parity of the fp16-storage build (libvista_hip_f16.so) at the edge shapes of tests/test_kernels_gpu.py, in this process:
ops.storage(torch.float16) switches the enclosed ops.* calls to the fp16 library. Cases, float64 references and bounds: tests/_f16_cases.py (bound A:
derived from the number formats; bound B: measured on the MI355X + 25 %, profiles/f16_kernel_parity.txt); tests/test_f16_bounds_cpu.py proves that
the bounds separate a correct output from a broken one. Every test prints its figures (`F16PARITY ...`) before it asserts."""
import ctypes as C
import os

import pytest
import torch

from tests import _f16_cases as fc

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@pytest.fixture(autouse=True)
def f16_storage():
    from vista_amd import build, ops
    if not os.path.exists(build.LIB_F16):
        pytest.fail("vista_amd/lib/libvista_hip_f16.so is missing: __graft_entry__.build() links both storage variants")
    saved = (ops.TILE_CFG, ops.SPLITK_WS_BYTES)
    try:
        with ops.storage(F16):
            yield ops
    finally:
        ops.TILE_CFG, ops.SPLITK_WS_BYTES = saved


def test_storage_context_selects_the_f16_library_and_restores(f16_storage):
    """Inside ops.storage(torch.float16): the fp16 library and ops.ACT = float16, whatever the state before; the previous state -- here bf16, entered
    by hand so that it differs in every process -- is back when the context ends."""
    from vista_amd import _lib
    ops = f16_storage
    assert _lib.load().vk_act_dtype() == 1 and ops.ACT is F16 and ops.BF16 is F16 and _lib.CURRENT == "fp16"   # the fixture's context
    with ops.storage(BF16):
        assert _lib.load().vk_act_dtype() == 0 and ops.ACT is BF16 and _lib.CURRENT == "bf16"
        with ops.storage(F16):
            assert _lib.load().vk_act_dtype() == 1 and ops.ACT is F16 and ops.BF16 is F16 and _lib.CURRENT == "fp16"
            x = torch.ones(128, 64, dtype=F16, device="cuda")
            assert ops.linear(x, ops.pack_linear(torch.eye(64), None)).dtype is F16
        assert _lib.load().vk_act_dtype() == 0 and ops.ACT is BF16 and ops.BF16 is BF16 and _lib.CURRENT == "bf16"
    assert _lib.load().vk_act_dtype() == 1 and ops.ACT is F16 and _lib.CURRENT == "fp16"
    assert sorted(_lib._libs) == ["bf16", "fp16"]


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
        ok, fig = fc.check_any(spec, out, ref)
        print(f"F16PARITY {case.name}[{k}] {spec[0]} {tag} " + " ".join(f"{a}={b:.4g}" if isinstance(b, float) else f"{a}={b}" for a, b in fig.items()))
        if not ok:
            fails.append((k, spec[0], fig))
    assert not fails, f"{case.name} {tag}: {fails}"


_PARAMS = [pytest.param(c, cfg, id=f"{c.name}-cfg{cfg}") for c in fc.CASES for cfg in (fc.TILE_CFGS if c.tiles else (0,))]


@pytest.mark.parametrize("case,cfg", _PARAMS)
def test_case(case, cfg, f16_storage):
    """One case of tests/_f16_cases.py (GEMM-family cases: under every forced block-tile variant; a variant that does not take a problem falls
    back to the launcher's choice) against its float64 reference. Bound B (measured on the MI355X -> bound = + 25 %; each pair: _f16_cases.B_BOUNDS):
    ff_* 2.09e-4 .. 2.17e-4 -> 2.62e-4 .. 2.72e-4; attn_spatial_* (diffuse rows, first-tile base) 2.07e-4 .. 2.17e-4 -> 2.59e-4 .. 2.71e-4;
    attn_zero_base_gain12 3.84e-4 -> 4.80e-4, _gain400 4.65e-5 -> 5.81e-5 (most rows are one exact bf16 V value), attn_max_free_fallback_gain60
    1.03e-4 -> 1.29e-4, attn_spike_forces_rescale 5.35e-4 -> 6.68e-4; attn_temporal_* 3.88e-4 .. 5.58e-4 -> 4.85e-4 .. 6.97e-4."""
    ops = f16_storage
    i, refs = _inputs_and_ref(case)
    ops.TILE_CFG = cfg
    outs = case.run(ops, fc.to_device(i, "cuda"))
    ops.TILE_CFG = 0
    _judge(case, outs, refs, f"cfg{cfg}")


# ------------------------------------------------------------------------------------------------ helpers of the hand-written tests
def rnd(*shape, scale=1.0, seed=0, dtype=F16):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _norm(Cc, seed=7):
    g = torch.Generator().manual_seed(seed)
    return fc.Norm((1 + 0.2 * torch.randn(Cc, generator=g)).cuda(), (0.1 * torch.randn(Cc, generator=g)).cuda())


def _check_stats(st, out):
    """RowStats slabs summed over parts == float64 (sum, sum of squares) of the kernel's own fp16 output rows (tolerance of the bf16 suite)."""
    o = out.double()
    got = st.t.sum(0).double()
    ref = torch.stack([o.sum(1), o.pow(2).sum(1)], 1)
    tol = 2e-5 * torch.stack([o.abs().sum(1), o.pow(2).sum(1)], 1) + 1e-6
    worst = ((got - ref).abs() / tol).max().item()
    print(f"F16PARITY rowstats worst/tol={worst:.3g}")
    assert worst <= 1.0, f"row sums off: {worst:.3g} of the tolerance"


def _forced(ops, cfg, fn):
    ops.TILE_CFG = cfg
    try:
        return fn()
    finally:
        ops.TILE_CFG = 0


# ------------------------------------------------------------------------------------------------ alt_cols_from: refusals, launcher choice
def test_alt_cols_from_refusals(f16_storage):
    from vista_amd._lib import VistaHipError
    ops = f16_storage
    x = rnd(300, 320)
    pw = ops.pack_linear(rnd(320, 320, scale=320 ** -0.5, seed=1), None)
    for bad in (16, 48, 320, 352):   # not a multiple of 32; >= N
        with pytest.raises(VistaHipError):
            ops.linear(x, pw, alt_cols_from=bad)
    with pytest.raises(VistaHipError):
        ops.linear(x, pw, alt_cols_from=64, out_f32=True)
    with pytest.raises(VistaHipError):
        ops.linear(x, pw, alt_cols_from=64, emit_stats=True)
    assert ops.linear(x, pw, alt_cols_from=64).dtype is F16


def test_alt_cols_from_keeps_the_launcher_off_the_streaming_kernel(f16_storage):
    ops = f16_storage
    lib = ops._lib.load()
    x = rnd(65536 * 2, 320)
    pw = ops.pack_linear(rnd(320, 320, seed=1), rnd(320, seed=2).float())
    out = torch.empty_like(x)

    def choice(alt, force=0):
        dsc = ops.VkGemmDesc()
        dsc.A, dsc.lda, dsc.amode, dsc.epi = ops._p(x), 320, 0, 0
        ops._fill_epilogue(dsc, pw, out, x.shape[0], None, 0, x, None, 1.0, 0.0)
        dsc.alt_cols_from, dsc.tile_cfg = alt, force
        return lib.vk_gemm_tile_choice(C.byref(dsc)) // 16
    if os.environ.get("VISTA_GEMM_STREAM", "1") != "0":
        assert choice(0) == 6
    assert choice(0, 6) == 6
    assert choice(32) not in (6, 0) and choice(288) != 6 and choice(32, 6) != 6


# ------------------------------------------------------------------------------------------------ halo frames
def test_conv_t3_halo_frames_are_bitwise_the_slice_of_the_whole_clip(f16_storage):
    ops = f16_storage
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
def test_splitk_with_and_without_workspace(name, f16_storage):
    """Both runs within bound A / F32; the 16-bit results at most one fp16 ulp apart (another fp32 summation order; measured: the dense case
    agrees bit for bit, the conv case differs in 19915 of 9.2 M elements, each by one ulp or by the fp32 difference itself near zero); the fp32 form repeatable
    bit for bit and NOT equal to the plain kernel's -- which proves that the split path ran."""
    ops = f16_storage
    case = fc.BY_NAME[name]
    i, refs = _inputs_and_ref(case)
    ig = fc.to_device(i, "cuda")
    split = case.run(ops, ig)
    again = case.run(ops, ig)
    ops.SPLITK_WS_BYTES = 0
    plain = case.run(ops, ig)
    _judge(case, split, refs, "split")
    _judge(case, plain, refs, "plain")
    # one fp16 ulp apart: both fp32 values lie within the F32 bound of the reference (asserted above), i.e. within 4e-5 (|ref| + rms) of each
    # other, and their roundings then differ by at most that plus one ulp of the larger one
    s16, p16, ref = split[0].double().cpu(), plain[0].double().cpu(), refs[0].double()
    ulp = torch.maximum(s16.abs(), p16.abs()).clamp_min(2.0 ** -14).log2().floor().exp2() * 2.0 ** -10
    tol = ulp + 4e-5 * (ref.abs() + ref.pow(2).mean().sqrt())
    apart = ((s16 - p16).abs() / tol).max().item()
    print(f"F16PARITY {name} split-vs-plain worst/(ulp + fp32 slack)={apart:.3g} differing={int((split[0] != plain[0]).sum())}")
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
        return lambda **kw: ops.linear(x, pw, ln=st, alt_cols_from=2 * Cc, **kw)
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
def test_pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(kind, n, H, W, Cc, f16_storage):
    """tile_cfg 7 (gemm_pipe.hip) == tile_cfg 4, outputs and row-sum slabs, inside the fp16 build; the q|k|v kind carries alt_cols_from."""
    ops = f16_storage
    if kind == "conv3x3_stride2" and (H % 2 or W % 2):
        H, W = 10, 12
    fn = _kind_fn(ops, kind, n, H, W, Cc)
    _same_bits(_forced(ops, 7, fn), _forced(ops, 4, fn), f"{kind} cfg 7 vs 4")


@pytest.mark.parametrize("kind", DENSE_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", BITWISE_SHAPES)
def test_two_per_cu_kernel_is_bitwise_the_pipelined_kernel(kind, n, H, W, Cc, f16_storage):
    """tile_cfg bit 4 (gemm_pipe2.hip) == tile_cfg 7 for the dense kinds."""
    ops = f16_storage
    fn = _kind_fn(ops, kind, n, H, W, Cc)
    _same_bits(_forced(ops, 16, fn), _forced(ops, 7, fn), f"{kind} cfg 16 vs 7")


@pytest.mark.parametrize("kind", ["qkv_lnfold", "dense_K4N+res+stats", "conv3x3+emb+res", "conv_t3+blend"])
def test_tail_split_is_bitwise_the_single_launch(kind, f16_storage):
    """tile_cfg bit 6 at (29, 36, 64), C = 320: 261 row tiles of 256 -> whole rounds on the pipelined kernel + the rest as 128x160 tiles."""
    ops = f16_storage
    n, H, W, Cc = 29, 36, 64, 320
    N = 3 * Cc if kind == "qkv_lnfold" else Cc
    tiles = ((n * H * W + 255) // 256) * (N // 320)
    assert tiles // 256 >= 1 and 0 < tiles % 256 <= 0.4 * 256   # a shape the rule splits
    fn = _kind_fn(ops, kind, n, H, W, Cc)
    _same_bits(_forced(ops, 64, fn), _forced(ops, 7, fn), f"{kind} tail split vs single launch")


# ------------------------------------------------------------------------------------------------ ff_fused against the two-kernel form
@pytest.mark.parametrize("M", [128, 1000, 4173])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("mode", ["plain", "res", "blend"])
def test_ff_fused_against_the_two_kernel_form(M, ln, mode, f16_storage):
    """Same products, same fp16 rounding of the hidden activation; only the fp32 summation order of the out-projection differs: the relation the
    bf16 suite asserts (relative L2 distance < 2e-3), and with emit_stats the row sums of the two forms within 1e-3 and those of the fused kernel
    equal to the sums of its own output."""
    ops = f16_storage
    case = fc.BY_NAME[f"ff_{M}_{'ln' if ln else 'noln'}_{mode}"]
    i, _ = _inputs_and_ref(case)
    fus, two = case.run(ops, fc.to_device(i, "cuda"))
    dist = ((fus.double() - two.double()).norm() / two.double().norm()).item()
    print(f"F16PARITY {case.name} fused-vs-two-kernel rel_l2={dist:.4g} bound=0.002")
    assert dist < 2e-3
    if mode == "res":
        ig = fc.to_device(i, "cuda")
        pin = ops.pack_geglu(ig.w1, ig.b1, ln=fc.Norm(ig.gamma, ig.beta) if ln else None)
        st = ops.rowstats(ig.x) if ln else None
        two, st2 = ops.linear(ops.linear(ig.x, pin, ln=st), ops.pack_linear(ig.w2, ig.b2), res1=ig.x, emit_stats=True)
        fus2, stf = ops.ff_fused(ig.x, pin, ops.pack_ff_out(ig.w2, ig.b2), ln=st, res1=ig.x, emit_stats=True)
        assert torch.equal(fus2, fus), "emitting the row sums changed the output"
        assert stf.parts == 2 and stf.t.shape == (2, M, 2)
        s2, sf = st2.t.sum(0), stf.t.sum(0)
        assert ((s2 - sf).abs().max() / s2.abs().max()).item() < 1e-3
        _check_stats(stf, fus2)


# ------------------------------------------------------------------------------------------------ the streaming GEMM, forced
@pytest.mark.parametrize("kind", ["plain", "res+rowvec+stats", "qkv_lnfold", "qkv_lnfold+alt"])
def test_gemm_stream_forced(kind, f16_storage):
    """tile_cfg 6 at M = 32 * 300 + 7 against float64 (bound A) and bitwise against the tiled kernel. With alt_cols_from the streaming kernel
    refuses the launch, so the forced variant falls back to the tiled kernels: same bits as tile_cfg 4, V block in bf16."""
    ops = f16_storage
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
        if kind.endswith("alt"):
            kw["alt_cols_from"] = 2 * Cc
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
    outs, refs, specs = [o6], [ref], [("A", F16)]
    if kind.endswith("alt"):
        outs, refs = [o6[:, :2 * Cc].contiguous(), o6[:, 2 * Cc:].contiguous().view(BF16)], [ref[:, :2 * Cc].contiguous(), ref[:, 2 * Cc:].contiguous()]
        specs = [("A", F16), ("A", BF16)]
    for k, (spec, out, r) in enumerate(zip(specs, outs, refs)):
        ok, fig = fc.check(spec, out, r)
        print(f"F16PARITY gemm_stream_{kind}[{k}] {fig}")
        assert ok, (kind, k, fig)


# ------------------------------------------------------------------------------------------------ statistics outputs
@pytest.mark.parametrize("rows,Cc", [(257, 640), (64, 64)])
def test_rowstats_are_the_sums_of_the_input(rows, Cc, f16_storage):
    ops = f16_storage
    x = (rnd(rows, Cc).float() + 2.0).to(F16)
    st = ops.rowstats(x)
    assert st.parts == 1
    _check_stats(st, x)
    big = rnd(rows, 2 * Cc, seed=3)
    _check_stats(ops.rowstats(big[:, Cc:]), big[:, Cc:])   # strided rows


@pytest.mark.parametrize("cfg", fc.TILE_CFGS)
def test_emit_stats_are_the_sums_of_the_rounded_output(cfg, f16_storage):
    """The row sums a GEMM epilogue emits are those of its own fp16-ROUNDED output (what the next LayerNorm fold reads), not of the fp32 value."""
    ops = f16_storage
    M, N, K = 777, 320, 320
    x = rnd(M, K)
    pw = ops.pack_linear(rnd(N, K, scale=K ** -0.5, seed=1), rnd(N, seed=2).float())
    r1, rv = rnd(M, N, seed=4), rnd(3, N, seed=5).float()
    out, st = _forced(ops, cfg, lambda: ops.linear(x, pw, res1=r1, rowvec=rv, rows_per_vec=(M + 2) // 3, emit_stats=True))
    assert out.dtype is F16 and st.M == M and st.t.shape == (st.parts, M, 2)
    _check_stats(st, out)


def test_conv_epilogue_groupnorm_statistics(f16_storage):
    """One shape of tests/test_gnstat_gpu.py ("conv+res", C = 320, 3 images of 16x16, pipelined kernel): the folded partials equal float64 group
    sums of the convolution's own fp16 output, to that file's tolerance (2e-5 of sqrt(count * sum of squares) / of the sum of squares)."""
    from vista_amd import _lib
    ops = f16_storage
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
    print(f"F16PARITY gnstat sums={es:.3g} sumsq={eq:.3g} bound=2e-5")
    assert es <= 2e-5 and eq <= 2e-5
    # and the norm from those partials against float64 GroupNorm + SiLU of that output (bound A)
    gamma, beta = 1.0 + 0.2 * rnd(Cc, seed=10).float(), 0.2 * rnd(Cc, seed=11).float()
    got_y = ops.groupnorm(out.view(n, S, Cc), gamma, beta, 1e-5, True, gn=gn)
    assert gn.t is None
    y = torch.nn.functional.silu(torch.nn.functional.group_norm(out.view(n, S, Cc).double().cpu().transpose(1, 2), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5))
    ok, fig = fc.check(("A", F16), got_y, y.transpose(1, 2))
    print(f"F16PARITY groupnorm_from_partials {fig}")
    assert ok, fig


# ------------------------------------------------------------------------------------------------ norms: bitwise relation
@pytest.mark.parametrize("name", ["groupnorm_cat_3x144x640+320", "groupnorm_cat_2x100x64+128"])
def test_groupnorm_cat_is_bitwise_groupnorm_of_the_concat(name, f16_storage):
    ops = f16_storage
    i = fc.to_device(_inputs_and_ref(fc.BY_NAME[name])[0], "cuda")
    silu = name.startswith("groupnorm_cat_3")
    got = ops.groupnorm_cat(i.a, i.b, i.gamma, i.beta, 1e-5, silu)
    want = ops.groupnorm(torch.cat([i.a, i.b], 2).contiguous(), i.gamma, i.beta, 1e-5, silu)
    assert torch.equal(got, want), "same arithmetic in the same order: bitwise equal"


# ------------------------------------------------------------------------------------------------ what the fp16 build refuses
def test_attn_spatial_with_a_vt_tensor_raises(f16_storage):
    from vista_amd._lib import VistaHipError
    ops = f16_storage
    q, k = rnd(144, 64), rnd(144, 64, seed=1)
    vt = rnd(1, 64, 144, seed=2)
    with pytest.raises(VistaHipError):
        ops.attn_spatial(q, k, vt, 1, 1, 144)


def test_fp8_entry_points_raise(f16_storage):
    """BASELINE config 5 (fp8) exists in the bf16 build only: the fp16 library's fp8 entry points answer VK_EINVAL before any launch."""
    from vista_amd._lib import VistaHipError
    ops = f16_storage
    M, K, N = 256, 256, 320
    xq = torch.zeros(M, K, dtype=torch.uint8, device="cuda")
    pw8 = ops.pack_linear_fp8(torch.randn(N, K) * K ** -0.5, None)
    with pytest.raises(VistaHipError):
        ops.linear_fp8(xq, torch.ones(M, device="cuda"), pw8)
    S = 64
    q8 = torch.zeros(S, 64, dtype=torch.uint8, device="cuda")
    sc = torch.full((S, 2), 127, dtype=torch.uint8, device="cuda")
    with pytest.raises(VistaHipError):
        ops.attn_spatial_fp8qk(q8, q8, sc, sc, rnd(S, 64), 1, 1, S)
