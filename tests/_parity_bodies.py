"""The storage-independent bodies of the two kernel parity modules (tests/test_f16_kernels_gpu.py, tests/test_bf16_kernels_gpu.py), each written
once: a body takes the ops module inside the caller's ops.storage(...) context and the caller's case module fc (tests._f16_cases or
tests._bf16_cases); whatever depends on the storage type -- the print tag, dtypes, ulp constants, alt_cols_from -- follows from fc.T.ST. Every
body prints its figures (`F16PARITY ...` / `BF16PARITY ...`) before it asserts. Nothing here imports vista_amd or touches a GPU at import time.

Every case runs on poisoned outputs inside guard bands (tests/_guard.py): case_under_tile runs its case inside guarded(ops) on embed(inputs) and
ends with verify(); the hand-written bodies run inside the guarded context of their module's storage fixture, which verifies at teardown, and
put their own operands into arenas (rnd). An element a kernel does not store is a NaN in the judged output, a store past an output, a
statistics slab or a workspace a damaged guard, a load past an operand a NaN in the result, an input written without leave a failure."""
import ctypes as C
import math

import torch

from tests import _guard

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _tag(fc):
    if getattr(fc, "TAG", None):   # tests/_fp8_cases.py: the fp8 table runs under bf16 storage with a tag of its own
        return fc.TAG              # "FP8PARITY"
    return "F16PARITY" if fc.T.ST is F16 else "BF16PARITY"


# ------------------------------------------------------------------------------------------------ the case table
_REF = {}


def inputs_and_ref(fc, case):
    """Computed once per (storage type, case) -- the two tables share most case names -- and shared by the case's tile variants; never modified."""
    key = (fc.T.ST, case.name)
    if key not in _REF:
        i = case.build()
        _REF[key] = (i, case.ref(i))
    return _REF[key]


def judge(fc, case, outs, refs, tag):
    fails = []
    assert len(outs) == len(refs) == len(case.specs)
    for k, (spec, out, ref) in enumerate(zip(case.specs, outs, refs)):
        ok, fig = fc.check_any(spec, out, ref, f"{case.name}[{k}]")
        print(f"{_tag(fc)} {case.name}[{k}] {spec[0]} {tag} " + " ".join(f"{a}={b:.4g}" if isinstance(b, float) else f"{a}={b}" for a, b in fig.items()))
        if not ok:
            fails.append((k, spec[0], fig))
    assert not fails, f"{case.name} {tag}: {fails}"


def case_under_tile(ops, fc, case, cfg, device="cuda"):
    """One run, on embedded inputs and poisoned outputs: judged against the float64 reference with the case's bounds, then every guard byte
    and every input must be what it was. (device: tests/test_extent_cpu.py drives plain-torch stand-ins through this very body on the CPU.)"""
    i, refs = inputs_and_ref(fc, case)
    with _guard.guarded(ops):
        ops.TILE_CFG = cfg
        try:
            outs = case.run(ops, _guard.embed(i, device, layout=case.layout))
        finally:
            ops.TILE_CFG = 0
        judge(fc, case, outs, refs, f"cfg{cfg}")
        _guard.verify()


# ------------------------------------------------------------------------------------------------ helpers of the hand-written tests
def rnd(fc, *shape, scale=1.0, seed=0, dtype=None):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return _guard.put((torch.randn(*shape, generator=g) * scale).to(dtype or fc.T.ST), label="rnd")


def _norm(fc, Cc, seed=7):
    g = torch.Generator().manual_seed(seed)
    return fc.Norm(_guard.put(1 + 0.2 * torch.randn(Cc, generator=g), label="gamma"), _guard.put(0.1 * torch.randn(Cc, generator=g), label="beta"))


def check_stats(fc, st, out):
    """RowStats slabs summed over parts == float64 (sum, sum of squares) of the kernel's own 16-bit output rows (tolerance of
    tests/test_kernels_gpu.py)."""
    o = out.double()
    got = st.t.sum(0).double()
    ref = torch.stack([o.sum(1), o.pow(2).sum(1)], 1)
    tol = 2e-5 * torch.stack([o.abs().sum(1), o.pow(2).sum(1)], 1) + 1e-6
    worst = ((got - ref).abs() / tol).max().item()
    print(f"{_tag(fc)} rowstats worst/tol={worst:.3g}")
    assert worst <= 1.0, f"row sums off: {worst:.3g} of the tolerance"


def forced(ops, cfg, fn):
    ops.TILE_CFG = cfg
    try:
        return fn()
    finally:
        ops.TILE_CFG = 0


# ------------------------------------------------------------------------------------------------ halo frames
def conv_t3_halo_frames_are_bitwise_the_slice_of_the_whole_clip(ops, fc):
    B, T, S, Cc = 2, 8, 40, 128
    x = rnd(fc, B * T, S, Cc)
    pw = ops.pack_conv_t3(rnd(fc, Cc, Cc, 3, 1, 1, scale=(3 * Cc) ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
    full = ops.conv_t3(x, pw, T, S).view(B, T, S, Cc)
    x4 = x.view(B, T, S, Cc)
    for t0, t1 in ((0, 3), (3, 7), (7, 8)):
        loc = x4[:, t0:t1].reshape(B * (t1 - t0), S, Cc).contiguous()
        prev = x4[:, t0 - 1].contiguous() if t0 > 0 else None
        nxt = x4[:, t1].contiguous() if t1 < T else None
        out = ops.conv_t3(loc, pw, t1 - t0, S, halo_prev=prev, halo_next=nxt).view(B, t1 - t0, S, Cc)
        assert torch.equal(out, full[:, t0:t1]), (t0, t1)


# ------------------------------------------------------------------------------------------------ split-K
def _run_recording_choices(ops, case, ig):
    """case.run with every GEMM launch's (K slices, M, N) recorded: vk_gemm_tile_choice asked about the very descriptor of the launch."""
    asked, gemm = [], ops._gemm

    def recording(desc, *a, **k):
        ops._prepare(desc)
        choice = ops._lib.load().vk_gemm_tile_choice(C.byref(desc))
        assert choice > 0, choice
        asked.append((choice % 16, desc.M, desc.N))
        return gemm(desc, *a, **k)
    ops._gemm = recording
    try:
        return case.run(ops, ig), asked
    finally:
        ops._gemm = gemm


def splitk_with_and_without_workspace(ops, fc, name):
    """The split runs with the workspace at exactly slices x M x N x 4 bytes (slices from vk_gemm_tile_choice, asked again at that size), its
    back guard intact. Both runs within bound A / F32; the 16-bit results at most one ulp of the storage type apart (another fp32 summation
    order); the fp32 form repeatable bit for bit -- across the two workspace sizes -- and NOT equal to the plain kernel's -- which proves that
    the split path ran."""
    case = fc.BY_NAME[name]
    i, refs = inputs_and_ref(fc, case)
    ig = _guard.embed(i)
    again, asked = _run_recording_choices(ops, case, ig)          # the default workspace: what the launcher asks of each launch
    # (the fp32-output launch is the one this body proves split, below; the launcher's rules keep the dense case's 16-bit launch whole)
    assert len(asked) == 2 and asked[1][0] > 1, f"the launcher does not split this case: (slices, M, N) = {asked}"
    ops.SPLITK_WS_BYTES = max(s * M * N * 4 for s, M, N in asked if s > 1)   # exactly what include/vista_hip.h states a split needs, behind it the back guard
    ops._SPLITK_WS.ws.clear()
    split, taken = _run_recording_choices(ops, case, ig)
    print(f"{_tag(fc)} {name} split-K (slices, M, N)={asked} workspace={ops.SPLITK_WS_BYTES} bytes")
    assert taken == asked, f"with the workspace at its stated size the launcher chose {taken}, not {asked}"
    ops.SPLITK_WS_BYTES = 0
    plain, none = _run_recording_choices(ops, case, ig)
    assert all(s == 1 for s, _, _ in none)
    judge(fc, case, split, refs, "split")
    judge(fc, case, plain, refs, "plain")
    # one ulp apart: both fp32 values lie within the F32 bound of the reference (asserted above), i.e. within 4e-5 (|ref| + rms) of each
    # other, and their roundings then differ by at most that plus one ulp of the larger one
    fi = torch.finfo(fc.T.ST)
    s16, p16, ref = split[0].double().cpu(), plain[0].double().cpu(), refs[0].double()
    ulp = torch.maximum(s16.abs(), p16.abs()).clamp_min(fi.tiny).log2().floor().exp2() * fi.eps
    tol = ulp + 4e-5 * (ref.abs() + ref.pow(2).mean().sqrt())
    apart = ((s16 - p16).abs() / tol).max().item()
    print(f"{_tag(fc)} {name} split-vs-plain worst/(ulp + fp32 slack)={apart:.3g} differing={int((split[0] != plain[0]).sum())}")
    assert apart <= 1.0
    assert torch.equal(split[1], again[1]) and torch.equal(split[0], again[0]), "split-K must be repeatable"
    assert not torch.equal(split[1], plain[1]), "the split-K path was not taken (its fp32 summation order differs from the plain kernel's)"


# ------------------------------------------------------------------------------------------------ bitwise equalities between kernels
DENSE_KINDS = ["dense+res+stats", "dense_strided_A", "qkv_lnfold", "ff_out+blend", "geglu_lnfold"]
CONV_KINDS = ["conv3x3+emb+res", "conv3x3_stride2", "conv3x3_ups2", "conv_t3+blend"]
# (n, H, W, C): ragged last tile, tiles spanning 3-4 images. The stride-2 conv needs even H, W: it runs at (5, 10, 12, 640) in the second shape.
BITWISE_SHAPES = [(3, 20, 24, 320), (5, 9, 13, 640)]


def _kind_fn(ops, fc, kind, n, H, W, Cc):
    S = H * W
    M = n * S
    x = rnd(fc, M, Cc)
    x3 = x.view(n, S, Cc)
    res = rnd(fc, M, Cc, seed=3)
    rv = _guard.put(rnd(fc, n, Cc, seed=5).float(), label="rowvec")
    if kind == "dense+res+stats":
        pw = ops.pack_linear(rnd(fc, Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
        return lambda **kw: ops.linear(x, pw, res1=res, rowvec=rv, rows_per_vec=S, emit_stats=True, **kw)
    if kind == "dense_strided_A":
        xs = rnd(fc, M, 3 * Cc, seed=11)[:, Cc:2 * Cc]
        pw = ops.pack_linear(rnd(fc, Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
        return lambda **kw: ops.linear(xs, pw, res1=res, **kw)
    if kind == "dense_K4N+res+stats":
        h4 = rnd(fc, M, 4 * Cc, seed=9)
        pw = ops.pack_linear(rnd(fc, Cc, 4 * Cc, scale=(4 * Cc) ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
        return lambda **kw: ops.linear(h4, pw, res1=res, rowvec=rv, rows_per_vec=S, emit_stats=True, **kw)
    if kind == "qkv_lnfold":
        pw = _guard.rehome_pack(ops.pack_linear(rnd(fc, 3 * Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(fc, 3 * Cc, seed=2).float(), ln=_norm(fc, Cc)))
        st = ops.rowstats(x)
        alt = {"alt_cols_from": 2 * Cc} if fc.T.ST is F16 else {}   # the fp16 build's q|k|v launch stores its V block as bf16; the bf16 build has no such field to set
        return lambda **kw: ops.linear(x, pw, ln=st, **alt, **kw)
    if kind == "ff_out+blend":
        h4 = rnd(fc, M, 4 * Cc, seed=9)
        pw = ops.pack_linear(rnd(fc, Cc, 4 * Cc, scale=(4 * Cc) ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
        return lambda **kw: ops.linear(h4, pw, res1=res, alpha=0.4, res2=x, rowvec2=rv, beta=0.6, rows_per_vec=S, **kw)
    if kind == "geglu_lnfold":
        pw = _guard.rehome_pack(ops.pack_geglu(rnd(fc, 8 * Cc, Cc, scale=Cc ** -0.5, seed=1), rnd(fc, 8 * Cc, seed=2).float(), ln=_norm(fc, Cc)))
        st = ops.rowstats(x)
        return lambda **kw: ops.linear(x, pw, ln=st, **kw)
    if kind.startswith("conv3x3"):
        pw = ops.pack_conv3x3(rnd(fc, Cc, Cc, 3, 3, scale=(9 * Cc) ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
        if kind == "conv3x3+emb+res":
            return lambda **kw: ops.conv3x3(x3, pw, n, H, W, rowvec=rv, res1=x3, **kw)[0]
        if kind == "conv3x3_ups2":
            return lambda **kw: ops.conv3x3(x3, pw, n, H, W, ups=2, rowvec=rv, **kw)[0]
        return lambda **kw: ops.conv3x3(x3, pw, n, H, W, stride=2, **kw)[0]
    pw = ops.pack_conv_t3(rnd(fc, Cc, Cc, 3, 1, 1, scale=(3 * Cc) ** -0.5, seed=1), rnd(fc, Cc, seed=2).float())
    return lambda **kw: ops.conv_t3(x3, pw, n, S, res2=x3, alpha=0.3, beta=1.0, **kw)


def _same_bits(fc, a, b, what):
    if isinstance(a, tuple):
        (a, sa), (b, sb) = a, b
        assert sa.parts == sb.parts and torch.equal(sa.t, sb.t), f"{what}: row-sum slabs differ"
        check_stats(fc, sa, a)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(ops, fc, kind, n, H, W, Cc):
    """tile_cfg 7 (gemm_pipe.hip) == tile_cfg 4, outputs and row-sum slabs."""
    if kind == "conv3x3_stride2" and (H % 2 or W % 2):
        H, W = 10, 12
    fn = _kind_fn(ops, fc, kind, n, H, W, Cc)
    _same_bits(fc, forced(ops, 7, fn), forced(ops, 4, fn), f"{kind} cfg 7 vs 4")


def two_per_cu_kernel_is_bitwise_the_pipelined_kernel(ops, fc, kind, n, H, W, Cc):
    """tile_cfg bit 4 (gemm_pipe2.hip) == tile_cfg 7 for the dense kinds."""
    fn = _kind_fn(ops, fc, kind, n, H, W, Cc)
    _same_bits(fc, forced(ops, 16, fn), forced(ops, 7, fn), f"{kind} cfg 16 vs 7")


def tail_split_is_bitwise_the_single_launch(ops, fc, kind):
    """tile_cfg bit 6 at (29, 36, 64), C = 320: 261 row tiles of 256 -> whole rounds on the pipelined kernel + the rest as 128x160 tiles."""
    n, H, W, Cc = 29, 36, 64, 320
    N = 3 * Cc if kind == "qkv_lnfold" else Cc
    tiles = ((n * H * W + 255) // 256) * (N // 320)
    assert tiles // 256 >= 1 and 0 < tiles % 256 <= 0.4 * 256   # a shape the rule splits
    fn = _kind_fn(ops, fc, kind, n, H, W, Cc)
    _same_bits(fc, forced(ops, 64, fn), forced(ops, 7, fn), f"{kind} tail split vs single launch")


# ------------------------------------------------------------------------------------------------ the streaming GEMM, forced
def gemm_stream_forced(ops, fc, kind):
    """tile_cfg 6 at M = 32 * 300 + 7 against float64 (bound A) and bitwise against the tiled kernel. With alt_cols_from (kind "qkv_lnfold+alt",
    fp16 build only) the streaming kernel refuses the launch, so the forced variant falls back to the tiled kernels: same bits as tile_cfg 4, the
    q|k columns checked as the storage type and the V block as bf16."""
    ST = fc.T.ST
    M, S, Cc = 32 * 300 + 7, 288, 320
    g = fc.G(31)
    N = 3 * Cc if kind.startswith("qkv") else Cc
    x, w, b, res = fc.r16(g, M, Cc), fc.r16(g, N, Cc, scale=Cc ** -0.5), fc.r32(g, N), fc.r16(g, M, Cc)
    rv = fc.r32(g, (M + S - 1) // S, Cc)
    gamma, beta = fc.r32(g, Cc, scale=0.2, shift=1.0), fc.r32(g, Cc, scale=0.1)
    kw, ln = {}, None
    xg = _guard.put(x, label="x")
    if kind.startswith("qkv"):
        ref = fc.ln_fold_ref(x, w, b, gamma, beta)
        pw = _guard.rehome_pack(ops.pack_linear(w.cuda(), b.cuda(), ln=fc.Norm(gamma.cuda(), beta.cuda())))
        ln = ops.rowstats(xg)
        if kind.endswith("alt"):
            kw["alt_cols_from"] = 2 * Cc
    else:
        ref = fc.d(x) @ fc.d(w).t() + fc.d(b)
        pw = ops.pack_linear(w.cuda(), b.cuda())
        if kind != "plain":
            ref = ref + fc.d(res) + fc.d(rv).repeat_interleave(S, 0)[:M]
            kw.update(res1=_guard.put(res, label="res1"), rowvec=_guard.put(rv, label="rowvec"), rows_per_vec=S, emit_stats=True)
    o6 = forced(ops, 6, lambda: ops.linear(xg, pw, ln=ln, **kw))
    o4 = forced(ops, 4, lambda: ops.linear(xg, pw, ln=ln, **kw))
    if isinstance(o6, tuple):
        (o6, s6), (o4, s4) = o6, o4
        assert s6.parts == 1, "the streaming kernel combines its waves' row sums into one slab"
        check_stats(fc, s6, o6)
    assert torch.equal(o6, o4), "streaming and tiled kernels must agree bit for bit"
    outs, refs, specs = [o6], [ref], [("A", ST)]
    if kind.endswith("alt"):
        outs, refs = [o6[:, :2 * Cc].contiguous(), o6[:, 2 * Cc:].contiguous().view(BF16)], [ref[:, :2 * Cc].contiguous(), ref[:, 2 * Cc:].contiguous()]
        specs = [("A", ST), ("A", BF16)]
    for k, (spec, out, r) in enumerate(zip(specs, outs, refs)):
        ok, fig = fc.check(spec, out, r)
        print(f"{_tag(fc)} gemm_stream_{kind}[{k}] {fig}")
        assert ok, (kind, k, fig)


# ------------------------------------------------------------------------------------------------ statistics outputs
def rowstats_are_the_sums_of_the_input(ops, fc, rows, Cc):
    x = (rnd(fc, rows, Cc).float() + 2.0).to(fc.T.ST)
    st = ops.rowstats(x)
    assert st.parts == 1
    check_stats(fc, st, x)
    big = rnd(fc, rows, 2 * Cc, seed=3)
    check_stats(fc, ops.rowstats(big[:, Cc:]), big[:, Cc:])   # strided rows


def emit_stats_are_the_sums_of_the_rounded_output(ops, fc, cfg):
    """The row sums a GEMM epilogue emits are those of its own 16-bit-ROUNDED output (what the next LayerNorm fold reads), not of the fp32 value."""
    M, N, K = 777, 320, 320
    x = rnd(fc, M, K)
    pw = ops.pack_linear(rnd(fc, N, K, scale=K ** -0.5, seed=1), rnd(fc, N, seed=2).float())
    r1, rv = rnd(fc, M, N, seed=4), _guard.put(rnd(fc, 3, N, seed=5).float(), label="rowvec")
    out, st = forced(ops, cfg, lambda: ops.linear(x, pw, res1=r1, rowvec=rv, rows_per_vec=(M + 2) // 3, emit_stats=True))
    assert out.dtype is fc.T.ST and st.M == M and st.t.shape == (st.parts, M, 2)
    check_stats(fc, st, out)


def conv_epilogue_groupnorm_statistics(ops, fc):
    """One shape of tests/test_gnstat_gpu.py ("conv+res", C = 320, 3 images of 16x16, pipelined kernel): the folded partials equal float64 group
    sums of the convolution's own 16-bit output, to that file's tolerance (2e-5 of sqrt(count * sum of squares) / of the sum of squares)."""
    assert ops.GN_EPI
    Cc, n, H, W = 320, 3, 16, 16
    S = H * W
    x, res = rnd(fc, n, S, Cc, seed=3), rnd(fc, n, S, Cc, seed=5)
    pw = ops.pack_conv3x3(rnd(fc, Cc, Cc, 3, 3, scale=(9 * Cc) ** -0.5, seed=6), rnd(fc, Cc, seed=7).float())
    base = forced(ops, 7, lambda: ops.conv3x3(x, pw, n, H, W, res1=res)[0])
    gn = ops.GnPartials()
    out = forced(ops, 7, lambda: ops.conv3x3(x, pw, n, H, W, res1=res, gn=gn)[0])
    assert gn.t is not None and gn.nchunks == S // 64 and torch.equal(out, base)
    sums = ops.torch.empty(n * 64, dtype=F32, device="cuda")   # (the fixture's guarded context: an arena)
    ops.check(ops._lib.load().vk_groupnorm_finalize_partials(ops._p(_guard.scratch(gn.t, "partial")), ops._p(sums), n, gn.nchunks, 1, ops._stream()), "vk_groupnorm_finalize_partials")
    got = sums.view(n, 64).double().cpu()
    o = out.view(n, S, 32, Cc // 32).double().cpu()
    ref_s, ref_q = o.sum((1, 3)), o.pow(2).sum((1, 3))
    count = (Cc // 32) * S
    es = ((got[:, :32] - ref_s).abs() / ((count * ref_q).sqrt() + 1e-6)).max().item()
    eq = ((got[:, 32:] - ref_q).abs() / (ref_q + 1e-6)).max().item()
    print(f"{_tag(fc)} gnstat sums={es:.3g} sumsq={eq:.3g} bound=2e-5")
    assert es <= 2e-5 and eq <= 2e-5
    # and the norm from those partials against float64 GroupNorm + SiLU of that output (bound A)
    gamma, beta = 1.0 + 0.2 * rnd(fc, Cc, seed=10).float(), 0.2 * rnd(fc, Cc, seed=11).float()
    got_y = ops.groupnorm(out.view(n, S, Cc), gamma, beta, 1e-5, True, gn=gn)
    assert gn.t is None
    y = torch.nn.functional.silu(torch.nn.functional.group_norm(out.view(n, S, Cc).double().cpu().transpose(1, 2), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5))
    ok, fig = fc.check(("A", fc.T.ST), got_y, y.transpose(1, 2))
    print(f"{_tag(fc)} groupnorm_from_partials {fig}")
    assert ok, fig


# ------------------------------------------------------------------------------------------------ norms: bitwise relation
def groupnorm_cat_is_bitwise_groupnorm_of_the_concat(ops, fc, name):
    i = _guard.embed(inputs_and_ref(fc, fc.BY_NAME[name])[0])
    silu = name.startswith("groupnorm_cat_3")
    got = ops.groupnorm_cat(i.a, i.b, i.gamma, i.beta, 1e-5, silu)
    want = ops.groupnorm(torch.cat([i.a, i.b], 2).contiguous(), i.gamma, i.beta, 1e-5, silu)
    assert torch.equal(got, want), "same arithmetic in the same order: bitwise equal"


# ------------------------------------------------------------------------------------------------ temporal attention: launch-geometry edges
def _qkv(fc, rows, heads, seed):
    """(rows, 3 * heads * 64) [q | k | v]: q, k values of the storage type, v bf16 values, as bits of the storage type."""
    st = fc.T.ST
    g = fc.G(seed)
    c = heads * 64
    q, k = (torch.randn(rows, c, generator=g).to(st) for _ in range(2))
    v = torch.randn(rows, c, generator=g).to(BF16)
    return torch.cat([q, k, v.view(st)], 1).contiguous(), v


def attn_temporal_one_key_is_bitwise_v(ops, fc):
    """(B, T, S, heads) = (1, 1, 64, 2): one key, so P = 1 and the output is V itself, cast to the output type, bit for bit."""
    st = fc.T.ST
    qkv, v = _qkv(fc, 64, 2, 41)
    o = ops.attn_temporal(_guard.put(qkv, label="qkv"), 1, 1, 64, 2)
    assert o.dtype is st and torch.equal(o.cpu(), v.float().to(st)), f"{int((o.cpu() != v.float().to(st)).sum())} of {o.numel()} elements differ from V"


def attn_temporal_narrow_store_is_bitwise_the_wide_store(ops, fc, B=2, T=7, S=9, heads=3):
    """The kernel's 8-byte store path (output rows whose stride is not a multiple of 8 elements) is unreachable from ops.attn_temporal, whose
    output is contiguous: vk_attn_temporal_bf16 through ctypes with an output view of row stride heads * 64 + 4. Bitwise the wide-store result;
    the four pad columns of every row keep their sentinel."""
    st = fc.T.ST
    c = heads * 64
    rows = B * T * S
    qkv = _guard.put(_qkv(fc, rows, heads, 43)[0], label="qkv")
    wide = ops.attn_temporal(qkv, B, T, S, heads)
    sentinel = torch.tensor(-1234.0).to(st)
    pad = ops.torch.full((rows, c + 4), sentinel.item(), dtype=st, device="cuda")   # (the fixture's guarded context: an arena)
    assert pad.stride(0) % 8 == 4 and pad.stride(0) % 4 == 0
    ops.check(ops._lib.load().vk_attn_temporal_bf16(ops._p(qkv), ops._p(pad), B, T, S, heads, qkv.stride(0), c, 2 * c, pad.stride(0),
                                                     C.c_float(1.0 / math.sqrt(64)), ops._stream()), "vk_attn_temporal_bf16")
    torch.cuda.synchronize()
    assert torch.equal(pad[:, :c], wide), f"{int((pad[:, :c] != wide).sum())} of {wide.numel()} elements differ between the 8-byte and the 16-byte store path"
    assert (pad[:, c:] == sentinel.cuda()).all(), "the store wrote past the output columns"
