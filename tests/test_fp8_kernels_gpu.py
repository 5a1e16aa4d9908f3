"""Per-kernel parity of the fp8 path (BASELINE config 5: csrc/gemm_fp8.hip, the fp8 parts of norm.hip and gemm.hip, attn_spatial_fp8qk of
attention.hip) against float64 references of the very e4m3 values and scales the kernels are handed, at format-derived bounds: the case table of
tests/_fp8_cases.py, the dense fp8 GEMM cases under every forced block tile (0, 1, 3, 4; GEGLU 0, 1, 3). Bounds A, F32, Q, MX: derived from the
number formats; bound B (attention, bf16 output): measured on the MI355X + 25 %, capped at 1.5 x the output-rounding floor
(profiles/fp8_kernel_parity.txt); the fp32 outputs of linear_fp8 and the GEGLU MX codes: F32 plus the fp8 MFMA's own summation error, measured
on the instruction alone (tools/probes/fp8_mfma_sum_probe.py, profiles/fp8_mfma_sum_probe.txt) + 25 %. tests/test_fp8_bounds_cpu.py proves that every bound separates a correct output from a truncated, bit-cut,
K-dropped, double-rounded, wrongly scaled or wrongly quantised one -- which the tolerances of tests/test_fp8_gpu.py do not. That module stays: its
quantisation-error tests against the unquantised function ask a different question. Every figure is printed (`FP8PARITY ...`) before it is asserted.

No bitwise equality between forced tile variants is asserted: csrc/gemm_fp8.hip promises none (its 128x128, 256x256 and 256x320 tiles share the
K-loop order per output element, but nothing in the file states that as a contract).

Every case runs on poisoned outputs inside guard bands (tests/_guard.py): e4m3 codes, E8M0 and fp32 scales, bf16 outputs and row-sum slabs are arena
interiors filled with 0xFF (NaN in each of these formats) before the launch, the operands are arena copies, and both tests/_parity_bodies.py:
case_under_tile and this module's fixture verify every guard byte and every input after the run."""
import os

import pytest
import torch

from tests import _fp8_cases as fc
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


_PARAMS = [pytest.param(c, cfg, id=f"{c.name}-cfg{cfg}") for c in fc.CASES for cfg in c.cfgs]


@pytest.mark.parametrize("case,cfg", _PARAMS)
def test_case(case, cfg, bf16_storage):
    """One case of tests/_fp8_cases.py (dense fp8 GEMM cases: under every forced block-tile variant) against its float64 reference."""
    pb.case_under_tile(bf16_storage, fc, case, cfg)
