"""The default (bf16-storage) build's instantiation of the kernel parity case table (tests/_kernel_cases.py: cases, float64 references, bounds):
what tests/test_bf16_kernels_gpu.py runs under ops.storage(torch.bfloat16) and tests/test_bf16_bounds_cpu.py proves to bite."""
from tests._kernel_cases import *   # noqa: F401,F403  (the storage-independent helpers: G, r32, d, I, Norm, to_device, splice_last_tile, ...)
from tests._kernel_cases import B_BOUNDS_BF16, LN_BOUNDS_BF16, make_cases

T = make_cases(BF16)   # noqa: F405
CASES, BY_NAME, B_BOUNDS, LN_BOUNDS = T.CASES, T.BY_NAME, B_BOUNDS_BF16, LN_BOUNDS_BF16
check, check_any, check_ln_fold, check_te32 = T.check, T.check_any, T.check_ln_fold, T.check_te32
out_dtype, storage_cast, truncate_cast, bitcut_cast, close_tol = T.out_dtype, T.storage_cast, T.truncate_cast, T.bitcut_cast, T.close_tol
r16, v_bits, folded, ln_fold_ref, attn_ref = T.r16, T.v_bits, T.folded, T.ln_fold_ref, T.attn_ref
