"""Per-kernel parity of the fp16-storage build (libvista_hip_f16.so) at the edge shapes of tests/test_kernels_gpu.py, in this process:
ops.storage(torch.float16) switches the enclosed ops.* calls to the fp16 library. Cases, float64 references and bounds: tests/_f16_cases.py (bound A:
derived from the number formats; bound B: measured on the MI355X + 25 %, profiles/f16_kernel_parity.txt); tests/test_f16_bounds_cpu.py proves that
the bounds separate a correct output from a broken one. The checks that do not depend on the storage type are written once, in
tests/_parity_bodies.py, and called here with this module's case table; what only the fp16 build has stays here. Every test prints its figures
(`F16PARITY ...`) before it asserts.

Every case runs on poisoned outputs inside guard bands (tests/_guard.py): the autouse storage fixture enters guarded(ops) around every test, so each
output, statistics slab, weight pack and workspace ops.py allocates is the interior of an arena whose guards and whose unwritten bytes are 0xFF
(NaN in fp16, bf16 and fp32 alike), the operands are arena copies, and the fixture's teardown verifies every guard byte and every input."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import _f16_cases as fc
from tests import _guard
from tests import _parity_bodies as pb

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
rnd = functools.partial(pb.rnd, fc)


@pytest.fixture(autouse=True)
def f16_storage():
    from vista_amd import build, ops
    if not os.path.exists(build.LIB_F16):
        pytest.fail("vista_amd/lib/libvista_hip_f16.so is missing: __graft_entry__.build() links both storage variants")
    saved = (ops.TILE_CFG, ops.SPLITK_WS_BYTES)
    try:
        with ops.storage(F16), _guard.guarded(ops):   # every allocation of ops.py an arena: poisoned outputs inside guard bands
            yield ops
            _guard.verify()                          # teardown: every guard byte intact, every embedded input unchanged
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
_PARAMS = [pytest.param(c, cfg, id=f"{c.name}-cfg{cfg}") for c in fc.CASES for cfg in c.cfgs]


@pytest.mark.parametrize("case,cfg", _PARAMS)
def test_case(case, cfg, f16_storage):
    """One case of tests/_f16_cases.py (GEMM-family cases: under every forced block-tile variant; a variant that does not take a problem falls
    back to the launcher's choice) against its float64 reference. Bound B (measured on the MI355X -> bound = + 25 %; each pair: _f16_cases.B_BOUNDS):
    ff_* 2.09e-4 .. 2.17e-4 -> 2.62e-4 .. 2.72e-4; attn_spatial_* (diffuse rows, first-tile base) 2.07e-4 .. 2.17e-4 -> 2.59e-4 .. 2.71e-4;
    attn_zero_base_gain12 3.84e-4 -> 4.80e-4, _gain400 4.65e-5 -> 5.81e-5 (most rows are one exact bf16 V value), attn_max_free_fallback_gain60
    1.03e-4 -> 1.29e-4, attn_spike_forces_rescale 5.35e-4 -> 6.68e-4; attn_temporal_* 3.88e-4 .. 5.58e-4 -> 4.85e-4 .. 6.97e-4."""
    pb.case_under_tile(f16_storage, fc, case, cfg)


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
    pb.conv_t3_halo_frames_are_bitwise_the_slice_of_the_whole_clip(f16_storage, fc)


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("name", ["splitk_dense_4032x1280x5120", "splitk_conv3x3_50x9x16x1280"])
def test_splitk_with_and_without_workspace(name, f16_storage):
    """Both runs within bound A / F32; the 16-bit results at most one fp16 ulp apart (another fp32 summation order; measured: the dense case
    agrees bit for bit, the conv case differs in 19915 of 9.2 M elements, each by one ulp or by the fp32 difference itself near zero); the fp32 form repeatable
    bit for bit and NOT equal to the plain kernel's -- which proves that the split path ran."""
    pb.splitk_with_and_without_workspace(f16_storage, fc, name)


# ------------------------------------------------------------------------------------------------ bitwise equalities between kernels
@pytest.mark.parametrize("kind", pb.DENSE_KINDS + pb.CONV_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", pb.BITWISE_SHAPES)
def test_pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(kind, n, H, W, Cc, f16_storage):
    """tile_cfg 7 (gemm_pipe.hip) == tile_cfg 4, outputs and row-sum slabs, inside the fp16 build; the q|k|v kind carries alt_cols_from."""
    pb.pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(f16_storage, fc, kind, n, H, W, Cc)


@pytest.mark.parametrize("kind", pb.DENSE_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", pb.BITWISE_SHAPES)
def test_two_per_cu_kernel_is_bitwise_the_pipelined_kernel(kind, n, H, W, Cc, f16_storage):
    pb.two_per_cu_kernel_is_bitwise_the_pipelined_kernel(f16_storage, fc, kind, n, H, W, Cc)


@pytest.mark.parametrize("kind", ["qkv_lnfold", "dense_K4N+res+stats", "conv3x3+emb+res", "conv_t3+blend"])
def test_tail_split_is_bitwise_the_single_launch(kind, f16_storage):
    pb.tail_split_is_bitwise_the_single_launch(f16_storage, fc, kind)


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
    i, _ = pb.inputs_and_ref(fc, case)
    fus, two = case.run(ops, _guard.embed(i))
    dist = ((fus.double() - two.double()).norm() / two.double().norm()).item()
    print(f"F16PARITY {case.name} fused-vs-two-kernel rel_l2={dist:.4g} bound=0.002")
    assert dist < 2e-3
    if mode == "res":
        ig = _guard.embed(i)
        pin = _guard.rehome_pack(ops.pack_geglu(ig.w1, ig.b1, ln=fc.Norm(ig.gamma, ig.beta) if ln else None))
        st = ops.rowstats(ig.x) if ln else None
        two, st2 = ops.linear(ops.linear(ig.x, pin, ln=st), ops.pack_linear(ig.w2, ig.b2), res1=ig.x, emit_stats=True)
        fus2, stf = ops.ff_fused(ig.x, pin, _guard.rehome_pack(ops.pack_ff_out(ig.w2, ig.b2)), ln=st, res1=ig.x, emit_stats=True)
        assert torch.equal(fus2, fus), "emitting the row sums changed the output"
        assert stf.parts == 2 and stf.t.shape == (2, M, 2)
        s2, sf = st2.t.sum(0), stf.t.sum(0)
        assert ((s2 - sf).abs().max() / s2.abs().max()).item() < 1e-3
        pb.check_stats(fc, stf, fus2)


# ------------------------------------------------------------------------------------------------ the streaming GEMM, forced
@pytest.mark.parametrize("kind", ["plain", "res+rowvec+stats", "qkv_lnfold", "qkv_lnfold+alt"])
def test_gemm_stream_forced(kind, f16_storage):
    """tile_cfg 6 at M = 32 * 300 + 7 against float64 (bound A) and bitwise against the tiled kernel. With alt_cols_from the streaming kernel
    refuses the launch, so the forced variant falls back to the tiled kernels: same bits as tile_cfg 4, V block in bf16."""
    pb.gemm_stream_forced(f16_storage, fc, kind)


# ------------------------------------------------------------------------------------------------ statistics outputs
@pytest.mark.parametrize("rows,Cc", [(257, 640), (64, 64)])
def test_rowstats_are_the_sums_of_the_input(rows, Cc, f16_storage):
    pb.rowstats_are_the_sums_of_the_input(f16_storage, fc, rows, Cc)


@pytest.mark.parametrize("cfg", fc.TILE_CFGS)
def test_emit_stats_are_the_sums_of_the_rounded_output(cfg, f16_storage):
    pb.emit_stats_are_the_sums_of_the_rounded_output(f16_storage, fc, cfg)


def test_conv_epilogue_groupnorm_statistics(f16_storage):
    pb.conv_epilogue_groupnorm_statistics(f16_storage, fc)


# ------------------------------------------------------------------------------------------------ norms: bitwise relation
@pytest.mark.parametrize("name", ["groupnorm_cat_3x144x640+320", "groupnorm_cat_2x100x64+128"])
def test_groupnorm_cat_is_bitwise_groupnorm_of_the_concat(name, f16_storage):
    pb.groupnorm_cat_is_bitwise_groupnorm_of_the_concat(f16_storage, fc, name)


# ------------------------------------------------------------------------------------------------ temporal attention: launch-geometry edges
def test_attn_temporal_one_key_is_bitwise_v(f16_storage):
    pb.attn_temporal_one_key_is_bitwise_v(f16_storage, fc)


def test_attn_temporal_narrow_store_is_bitwise_the_wide_store(f16_storage):
    pb.attn_temporal_narrow_store_is_bitwise_the_wide_store(f16_storage, fc)


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
