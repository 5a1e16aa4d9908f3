"""Per-kernel parity of the default bf16-storage build (libvista_hip.so) against float64 references of the very bf16 values the kernels are handed,
at format-derived bounds: the case table of tests/_bf16_cases.py (tests/_kernel_cases.py: make_cases(torch.bfloat16)) under every forced block tile,
and the bf16 twins of the hand-written tests of tests/test_f16_kernels_gpu.py that do not depend on the storage type. ops.storage(torch.bfloat16)
around every test, so the module also runs in a VISTA_ACT_DTYPE=fp16 process. Bound A: derived from the number format (u = 2^-8); bounds B and
LN: measured on the MI355X + 25 %, B capped at 1.5 x the output-rounding floor (profiles/bf16_kernel_parity.txt); tests/test_bf16_bounds_cpu.py
proves that the bounds separate a correct output from a truncated, bit-cut, K-dropped or double-rounded one -- which tests/test_kernels_gpu.py:
close() (1.6e-2 |ref| + 2e-2 rms) does not. The shared checks are written once, in tests/_parity_bodies.py, and called here with this module's case
table. Every test prints its figures (`BF16PARITY ...`) before it asserts.

Every case runs on poisoned outputs inside guard bands (tests/_guard.py): the autouse storage fixture enters guarded(ops) around every test, so each
output, statistics slab, weight pack and workspace ops.py allocates is the interior of an arena whose guards and whose unwritten bytes are 0xFF
(NaN in every format used here), the operands are arena copies, and the fixture's teardown verifies every guard byte and every input."""
import os

import pytest
import torch

from tests import _bf16_cases as fc
from tests import _guard
from tests import _parity_bodies as pb

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def bf16_storage():
    from vista_amd import build, ops
    if not os.path.exists(build.LIB):
        pytest.fail("vista_amd/lib/libvista_hip.so is missing: __graft_entry__.build() links both storage variants")
    saved = (ops.TILE_CFG, ops.SPLITK_WS_BYTES)
    try:
        with ops.storage(BF16), _guard.guarded(ops):   # every allocation of ops.py an arena: poisoned outputs inside guard bands
            yield ops
            _guard.verify()                           # teardown: every guard byte intact, every embedded input unchanged
    finally:
        ops.TILE_CFG, ops.SPLITK_WS_BYTES = saved


# ------------------------------------------------------------------------------------------------ the case table
_PARAMS = [pytest.param(c, cfg, id=f"{c.name}-cfg{cfg}") for c in fc.CASES for cfg in c.cfgs]


@pytest.mark.parametrize("case,cfg", _PARAMS)
def test_case(case, cfg, bf16_storage):
    """One case of tests/_bf16_cases.py (GEMM-family cases: under every forced block-tile variant of the case; a variant that does not take a
    problem falls back to the launcher's choice) against its float64 reference. Bounds B and LN: measured on the MI355X + 25 %, every pair in
    tests/_kernel_cases.py (B_BOUNDS_BF16, LN_BOUNDS_BF16) and in profiles/bf16_kernel_parity.txt."""
    pb.case_under_tile(bf16_storage, fc, case, cfg)


# ------------------------------------------------------------------------------------------------ halo frames
def test_conv_t3_halo_frames_are_bitwise_the_slice_of_the_whole_clip(bf16_storage):
    pb.conv_t3_halo_frames_are_bitwise_the_slice_of_the_whole_clip(bf16_storage, fc)


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("name", ["splitk_dense_4032x1280x5120", "splitk_conv3x3_50x9x16x1280"])
def test_splitk_with_and_without_workspace(name, bf16_storage):
    pb.splitk_with_and_without_workspace(bf16_storage, fc, name)


# ------------------------------------------------------------------------------------------------ bitwise equalities between kernels
@pytest.mark.parametrize("kind", pb.DENSE_KINDS + pb.CONV_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", pb.BITWISE_SHAPES)
def test_pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(kind, n, H, W, Cc, bf16_storage):
    pb.pipelined_kernel_is_bitwise_the_sixteen_wave_kernel(bf16_storage, fc, kind, n, H, W, Cc)


@pytest.mark.parametrize("kind", pb.DENSE_KINDS)
@pytest.mark.parametrize("n,H,W,Cc", pb.BITWISE_SHAPES)
def test_two_per_cu_kernel_is_bitwise_the_pipelined_kernel(kind, n, H, W, Cc, bf16_storage):
    pb.two_per_cu_kernel_is_bitwise_the_pipelined_kernel(bf16_storage, fc, kind, n, H, W, Cc)


@pytest.mark.parametrize("kind", ["qkv_lnfold", "dense_K4N+res+stats", "conv3x3+emb+res", "conv_t3+blend"])
def test_tail_split_is_bitwise_the_single_launch(kind, bf16_storage):
    pb.tail_split_is_bitwise_the_single_launch(bf16_storage, fc, kind)


# ------------------------------------------------------------------------------------------------ the streaming GEMM, forced
@pytest.mark.parametrize("kind", ["plain", "res+rowvec+stats", "qkv_lnfold"])
def test_gemm_stream_forced(kind, bf16_storage):
    pb.gemm_stream_forced(bf16_storage, fc, kind)


# ------------------------------------------------------------------------------------------------ statistics outputs
@pytest.mark.parametrize("rows,Cc", [(257, 640), (64, 64)])
def test_rowstats_are_the_sums_of_the_input(rows, Cc, bf16_storage):
    pb.rowstats_are_the_sums_of_the_input(bf16_storage, fc, rows, Cc)


@pytest.mark.parametrize("cfg", fc.TILE_CFGS)
def test_emit_stats_are_the_sums_of_the_rounded_output(cfg, bf16_storage):
    pb.emit_stats_are_the_sums_of_the_rounded_output(bf16_storage, fc, cfg)


def test_conv_epilogue_groupnorm_statistics(bf16_storage):
    pb.conv_epilogue_groupnorm_statistics(bf16_storage, fc)


# ------------------------------------------------------------------------------------------------ norms: bitwise relation
@pytest.mark.parametrize("name", ["groupnorm_cat_3x144x640+320", "groupnorm_cat_2x100x64+128"])
def test_groupnorm_cat_is_bitwise_groupnorm_of_the_concat(name, bf16_storage):
    pb.groupnorm_cat_is_bitwise_groupnorm_of_the_concat(bf16_storage, fc, name)


# ------------------------------------------------------------------------------------------------ temporal attention: launch-geometry edges
def test_attn_temporal_one_key_is_bitwise_v(bf16_storage):
    pb.attn_temporal_one_key_is_bitwise_v(bf16_storage, fc)


def test_attn_temporal_narrow_store_is_bitwise_the_wide_store(bf16_storage):
    pb.attn_temporal_narrow_store_is_bitwise_the_wide_store(bf16_storage, fc)


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
    ig = _guard.embed(i)
    pw = ops.pack_conv3x3(ig.w, ig.b)
    gn = ops.GnPartials() if route == "conv_epilogue_partials" else None
    y = pb.forced(ops, 7, lambda: ops.conv3x3(ig.x, pw, n, H, W, gn=gn)[0]).view(n, H * W, Cc)
    if gn is not None:
        assert ops.GN_EPI and gn.t is not None and gn.nchunks == H * W // 64, "the conv's epilogue did not emit its GroupNorm partials"
        got = ops.groupnorm(y, ig.gamma, ig.beta, 1e-5, False, gn=gn)
        assert gn.t is None
    else:
        got = ops.groupnorm_sharded(y, ig.gamma, ig.beta, 1e-5, False, 1, lambda sums: None, (Cc // 32) * H * W)
    ok, fig = fc.check(("A", BF16), got, fc.gn_route_ref(y.cpu(), i.gamma, i.beta))
    print(f"BF16PARITY groupnorm_large_mean_{route}[0] A cfg0 " + " ".join(f"{a}={b:.4g}" if isinstance(b, float) else f"{a}={b}" for a, b in fig.items()))
    assert ok, fig
