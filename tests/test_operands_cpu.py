"""The operand contract of the GEMM family (include/vista_hip.h, beside vk_gemm_bf16), pinned without a GPU through the four plan queries --
vk_gemm_tile_choice, vk_gemm_tail_split, vk_gemm_rowstat_parts, vk_gemm_gnstat_fit are host arithmetic and launch nothing, so the pointers here are
made up and never dereferenced (as in tests/test_upconv_fold_cpu.py); no made-up address is ever handed to an entry point that can launch.

The table below is written from the header, not read from the library: base alignment in bytes of every operand, and the multiple its leading
dimension must be. For every loader (amode), epilogue, output type and forced tile variant 0-7, every operand is moved 2, 4 and 8 bytes off a
4096-byte boundary and every leading dimension is grown by 1, 2 and 4 elements: the library must answer VK_EINVAL exactly where the table says so,
from all four queries alike, and plan a launch everywhere else -- on another kernel where the operand only costs a fast path (a declined fast path
is not an error). The extent rules that existed untested (P_LIMIT of vk_gemm_pipe_fit, the 32-bit row offsets of epi_fast_everywhere) are pinned
just under and just over each limit."""
import ctypes as C

import pytest

EINVAL = -22
BASE = 1 << 20
DENSE, CONV3X3, TEMPORAL3, CONV3D, UPCONV = 0, 1, 2, 3, 4
LINEAR, GEGLU, TRANS = 0, 1, 2
AMODES = {DENSE: "dense", CONV3X3: "conv3x3", TEMPORAL3: "temporal3", CONV3D: "conv3d", UPCONV: "upconv2x2"}
M, N, K = 260, 320, 192   # the shapes of the GPU layout cases (tests/_kernel_cases.py: operand_*)


@pytest.fixture(scope="module")
def lib():
    from vista_amd import _lib
    return _lib.load()


def desc(amode=DENSE, epi=LINEAR, f32=False, cfg=0, **kw):
    """A descriptor every operand of which sits on a 4096-byte boundary, with every optional operand the loader / epilogue admits left out."""
    from vista_amd import _lib
    d = _lib.VkGemmDesc()
    p = C.c_void_p(BASE)
    d.A = d.Wt = d.out = d.bias = p
    d.amode, d.epi, d.out_f32, d.tile_cfg, d.alpha = amode, epi, int(f32), cfg, 1.0
    d.splitk_ws, d.splitk_ws_bytes = p, 160 << 20
    d.N, d.ld_res1, d.ld_res2, d.ldv = N, N, N, N
    d.ldc = N // 2 if epi == GEGLU else N
    if amode == DENSE:
        d.M, d.K, d.lda, d.rows_per_vec, d.S = M, K, K, 130, M
    elif amode == CONV3X3:
        d.M, d.K, d.Cin, d.H, d.Wd, d.Hout, d.Wout, d.stride, d.ups, d.rows_per_vec, d.lda = 288, 576, 64, 9, 16, 9, 16, 1, 1, 144, 64
    elif amode == TEMPORAL3:
        d.M, d.K, d.Cin, d.T, d.S, d.rows_per_vec, d.lda = 432, 192, 64, 3, 144, 144, 64
    elif amode == CONV3D:
        d.M, d.K, d.Cin, d.T, d.H, d.Wd, d.rows_per_vec, d.lda = 288, 1728, 64, 2, 9, 16, 144, 64
    else:
        d.M, d.K, d.Cin, d.H, d.Wd, d.Hout, d.Wout, d.stride, d.ups, d.rows_per_vec, d.lda = 1152, 256, 64, 9, 16, 18, 32, 1, 2, 576, 64
    d.gn_rows = d.rows_per_vec
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def queries(lib, d):
    return [f(C.byref(d)) for f in (lib.vk_gemm_tile_choice, lib.vk_gemm_tail_split, lib.vk_gemm_rowstat_parts, lib.vk_gemm_gnstat_fit)]


def agree(lib, d, refused):
    """All four queries on d: VK_EINVAL from each (refused), or a plan from each -- vk_gemm_rowstat_parts answers VK_EINVAL by design for a launch
    that cannot emit row sums (fp32 out, GEGLU / TRANS), whatever the operands, and so do that query and vk_gemm_gnstat_fit for the folded upsample
    convolution, which emits neither (both plan the launch as emitting). -> the tile choice."""
    choice, tail, parts, gn = queries(lib, d)
    no_rowsums = bool(d.out_f32) or d.epi != LINEAR or d.amode == UPCONV
    if refused:
        assert (choice, tail, parts, gn) == (EINVAL,) * 4, (choice, tail, parts, gn)
    else:
        assert choice > 0 and tail >= 0 and (gn == EINVAL if d.amode == UPCONV else gn >= 0) and (parts == EINVAL if no_rowsums else parts > 0), (choice, tail, parts, gn)
    return choice


# operand -> (alignment in bytes (fp32 out / EPI_TRANS vectors: see align()), fields that switch the operand on)
OPTIONAL = {
    "A2": (16, dict(k_split=64, lda2=128)), "halo_prev": (16, {}), "halo_next": (16, {}),
    "res1": (8, {}), "res2": (8, dict(beta=1.0)), "rowvec": (16, {}), "rowvec2": (16, dict(res2=C.c_void_p(BASE), beta=1.0)),
    "ln_colsum": (16, dict(ln_stats=C.c_void_p(BASE), ln_parts=1, ln_eps=1e-5)), "ln_stats": (8, dict(ln_colsum=C.c_void_p(BASE), ln_parts=1, ln_eps=1e-5)),
    "rowstat_out": (8, {}), "gnstat_out": (4, {}),
}
ALWAYS = {"A": 16, "Wt": 16, "out": 8, "bias": 16, "splitk_ws": 16}


def align(name, epi, f32):
    if name == "out":
        return 16 if f32 else 8
    if name in ("bias", "ln_colsum") and epi == TRANS:
        return 4
    return ALWAYS[name] if name in ALWAYS else OPTIONAL[name][0]


def admitted(name, amode, epi, f32):
    """Optional operands a (loader, epilogue, output type) takes at all (anything else is refused whatever its address: not this file's subject)."""
    if amode == UPCONV:
        return name == "rowvec"
    if name in ("A2", "ln_colsum", "ln_stats"):
        return amode == DENSE
    if name.startswith("halo"):
        return amode == TEMPORAL3
    if name == "rowstat_out":
        return epi == LINEAR and not f32
    if name == "rowvec2":
        return epi == LINEAR
    return True


def combos():
    for amode in AMODES:
        for epi in ((LINEAR, GEGLU, TRANS) if amode == DENSE else (LINEAR,)):
            for f32 in ((False, True) if epi == LINEAR and amode != UPCONV else (False,)):
                yield amode, epi, f32


COUNTS = {"refused": 0, "planned": 0}


@pytest.mark.parametrize("amode,epi,f32", list(combos()), ids=lambda v: str(v))
def test_base_alignment_of_every_operand(amode, epi, f32, lib):
    """Byte skews 2, 4, 8 of every operand, forced variants 0-7: VK_EINVAL exactly where skew % alignment != 0, from all four queries."""
    tried = 0
    for cfg in range(8):
        if queries(lib, desc(amode, epi, f32, cfg))[0] < 0:
            assert amode == UPCONV and cfg not in (7,), (AMODES[amode], cfg)   # the folded upsample convolution exists on the pipelined kernel only
            continue
        for name in list(ALWAYS) + list(OPTIONAL):
            if name in OPTIONAL and not admitted(name, amode, epi, f32):
                continue
            on = OPTIONAL[name][1] if name in OPTIONAL else {}
            agree(lib, desc(amode, epi, f32, cfg, **on, **{name: C.c_void_p(BASE)}), refused=False)
            for skew in (2, 4, 8):
                refused = skew % align(name, epi, f32) != 0
                if amode == UPCONV and name == "out":
                    refused = True   # the one kernel that carries this mode stores 16 bytes: it declines the narrow out, and a declined mode is VK_EINVAL (the caller runs the nine-tap form)
                agree(lib, desc(amode, epi, f32, cfg, **on, **{name: C.c_void_p(BASE + skew)}), refused)
                COUNTS["refused" if refused else "planned"] += 1
                tried += 1
    assert tried >= 3 * len(ALWAYS)
    print(f"OPERANDS cpu {AMODES[amode]} epi{epi} f32={f32}: {tried} (operand, skew, variant) answers as the table says")


LD_RULES = {"lda": 8, "lda2": 8, "ldc": 4, "ld_res1": 4, "ld_res2": 4, "ldv": 4}
LD_NEEDS = {"lda": {}, "lda2": dict(A2=C.c_void_p(BASE), k_split=64), "ldc": {}, "ld_res1": dict(res1=C.c_void_p(BASE)),
            "ld_res2": dict(res2=C.c_void_p(BASE), beta=1.0), "ldv": dict(rowvec=C.c_void_p(BASE))}


@pytest.mark.parametrize("amode,epi,f32", list(combos()), ids=lambda v: str(v))
def test_leading_dimension_of_every_operand(amode, epi, f32, lib):
    """Leading dimensions + 1, + 2, + 4 (and + 8) elements, forced variants 0-7: VK_EINVAL exactly where the sum is no multiple of the operand's rule.
    lda / lda2 exist for the DENSE loader only (the convolutions' rows are Cin % 64 elements), ldc is not read by EPI_TRANS."""
    for cfg in range(8):
        base = desc(amode, epi, f32, cfg)
        if queries(lib, base)[0] < 0:
            continue
        for field, mult in LD_RULES.items():
            if field in ("lda", "lda2") and amode != DENSE:
                continue
            if amode == UPCONV and field in ("ld_res1", "ld_res2"):
                continue
            for plus in (1, 2, 4, 8):
                d = desc(amode, epi, f32, cfg, **LD_NEEDS[field])
                setattr(d, field, getattr(d, field) + plus)
                refused = (getattr(d, field) % mult != 0) and not (field == "ldc" and epi == TRANS)
                if field == "lda2":
                    d.lda2 = 128 + plus
                    refused = d.lda2 % mult != 0
                if amode == UPCONV and field == "ldc" and d.ldc % 8:
                    refused = True   # (declined by the only kernel of the mode: rows that are not 16-byte aligned)
                agree(lib, d, refused)
                COUNTS["refused" if refused else "planned"] += 1


def test_the_probe_of_the_issue(lib):
    """The dense 260 x 320 x 192 descriptor over the forced variants: the aligned answers, what a refused operand answers, and the two supported
    narrow operands -- planned under every variant, the pipelined kernel (7) giving way to the sixteen-wave one (4)."""
    def over(**kw):
        return [queries(lib, desc(cfg=cfg, **kw))[0] for cfg in range(8)]
    aligned = [17, 17, 33, 49, 65, 81, 17, 113]
    narrow = aligned[:7] + [65]
    assert over() == aligned
    for kw in (dict(A=C.c_void_p(BASE + 2)), dict(Wt=C.c_void_p(BASE + 2)), dict(A=C.c_void_p(BASE + 8)), dict(out=C.c_void_p(BASE + 2)), dict(ldc=322),
               dict(bias=C.c_void_p(BASE + 4)), dict(out_f32=1, out=C.c_void_p(BASE + 4)), dict(out_f32=1, out=C.c_void_p(BASE + 8))):
        assert over(**kw) == [EINVAL] * 8, kw
    assert over(out=C.c_void_p(BASE + 8)) == narrow and over(ldc=N + 4) == narrow
    assert over(res1=C.c_void_p(BASE + 8)) == narrow and over(res1=C.c_void_p(BASE), ld_res1=N + 4) == narrow
    assert over(A=C.c_void_p(BASE + 16), lda=K + 8) == aligned        # off the 128-byte line: the same kernel without its L2 prefetch
    # the streaming kernel at its smallest forced shape: taken when aligned, declined (a tiled kernel instead) for an out 8 bytes off
    assert queries(lib, desc(cfg=6, K=320, lda=320))[0] == 6 * 16 + 1
    assert queries(lib, desc(cfg=6, K=320, lda=320, A=C.c_void_p(BASE + 16), out=C.c_void_p(BASE + 8)))[0] == 1 * 16 + 1


LIMIT = 0xfffff000


@pytest.mark.parametrize("what,under,over", [
    # vk_gemm_pipe_fit, P_LIMIT: a 256-row tile of activation rows, and a 320-row tile of weight rows, stay below 4 GiB - 4 KiB of byte offsets
    ("256 lda 2 < P_LIMIT", dict(lda=8388592), dict(lda=8388600)),
    ("320 K 2 < P_LIMIT", dict(K=6710848, lda=6710848), dict(K=6710912, lda=6710912)),
    # epi_fast_everywhere: 32-bit byte offsets of the output / residual rows
    ("2 M ldc < 0xfffff000", dict(M=6710879), dict(M=6710880)),
    ("2 M ld_res1 < 0xfffff000", dict(res1=C.c_void_p(BASE), ld_res1=8259544), dict(res1=C.c_void_p(BASE), ld_res1=8259552)),
])
def test_extent_limits_of_the_pipelined_kernel(what, under, over, lib):
    """Just under each limit the forced variant 7 is taken; just over it the launch leaves variant 7 for a kernel with 64-bit addressing -- planned, not refused."""
    a, b = desc(cfg=7, **under), desc(cfg=7, **over)
    lo, hi = what.split(" < ")[0].split(), LIMIT
    ca, cb = agree(lib, a, False), agree(lib, b, False)
    print(f"OPERANDS cpu limit {what}: under -> {ca}, over -> {cb}")
    assert ca // 16 == 7, (what, ca)
    assert cb > 0 and cb // 16 != 7, (what, cb)
    # the two descriptors do straddle the limit
    val = {"256 lda 2": lambda d: 256 * d.lda * 2, "320 K 2": lambda d: 320 * d.K * 2, "2 M ldc": lambda d: 2 * d.M * d.ldc, "2 M ld_res1": lambda d: 2 * d.M * d.ld_res1}[" ".join(lo)]
    assert val(a) < hi <= val(b), (val(a), val(b))


def test_refusals_were_exercised():
    assert COUNTS["refused"] > 1000 and COUNTS["planned"] > 500, COUNTS
    print(f"OPERANDS cpu refusals={COUNTS['refused']} planned={COUNTS['planned']}")
