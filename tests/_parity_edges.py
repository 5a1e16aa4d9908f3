"""Hand-written launch-geometry checks shared by the two kernel parity modules (tests/test_f16_kernels_gpu.py, tests/test_bf16_kernels_gpu.py):
each takes the ops module inside the caller's ops.storage(...) context and the storage type. Nothing here touches a GPU at import time."""
import ctypes as C
import math

import torch

from tests import _kernel_cases as kc

BF16 = torch.bfloat16


def _qkv(st, rows, heads, seed):
    """(rows, 3 * heads * 64) [q | k | v]: q, k values of the storage type, v bf16 values, as bits of the storage type."""
    g = kc.G(seed)
    c = heads * 64
    q, k = (torch.randn(rows, c, generator=g).to(st) for _ in range(2))
    v = torch.randn(rows, c, generator=g).to(BF16)
    return torch.cat([q, k, v.view(st)], 1).contiguous(), v


def temporal_one_key_is_bitwise_v(ops, st):
    """(B, T, S, heads) = (1, 1, 64, 2): one key, so P = 1 and the output is V itself, cast to the output type, bit for bit."""
    qkv, v = _qkv(st, 64, 2, 41)
    o = ops.attn_temporal(qkv.cuda(), 1, 1, 64, 2)
    assert o.dtype is st and torch.equal(o.cpu(), v.float().to(st)), f"{int((o.cpu() != v.float().to(st)).sum())} of {o.numel()} elements differ from V"


def temporal_narrow_store_is_bitwise_the_wide_store(ops, st, B=2, T=7, S=9, heads=3):
    """The kernel's 8-byte store path (output rows whose stride is not a multiple of 8 elements) is unreachable from ops.attn_temporal, whose
    output is contiguous: vk_attn_temporal_bf16 through ctypes with an output view of row stride heads * 64 + 4. Bitwise the wide-store result;
    the four pad columns of every row keep their sentinel."""
    c = heads * 64
    rows = B * T * S
    qkv = _qkv(st, rows, heads, 43)[0].cuda()
    wide = ops.attn_temporal(qkv, B, T, S, heads)
    sentinel = torch.tensor(-1234.0).to(st)
    pad = torch.full((rows, c + 4), sentinel.item(), dtype=st, device="cuda")
    assert pad.stride(0) % 8 == 4 and pad.stride(0) % 4 == 0
    ops.check(ops._lib.load().vk_attn_temporal_bf16(ops._p(qkv), ops._p(pad), B, T, S, heads, qkv.stride(0), c, 2 * c, pad.stride(0),
                                                     C.c_float(1.0 / math.sqrt(64)), ops._stream()), "vk_attn_temporal_bf16")
    torch.cuda.synchronize()
    assert torch.equal(pad[:, :c], wide), f"{int((pad[:, :c] != wide).sum())} of {wide.numel()} elements differ between the 8-byte and the 16-byte store path"
    assert (pad[:, c:] == sentinel.cuda()).all(), "the store wrote past the output columns"
