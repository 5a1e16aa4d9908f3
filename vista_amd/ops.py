"""Torch-tensor front end of the C-ABI kernels (include/vista_hip.h).

PyTorch is used for device memory (caching allocator), streams and views only; every arithmetic op below is a
hand-written gfx950 kernel in libvista_hip.so. Activations are token-major bf16: (n_img, S=H*W, C), C contiguous.
"""
import ctypes as C
import math
import os
import threading

import torch

from . import _lib
from ._lib import VkFp8Args, VkGemmDesc, check

AMODE_DENSE, AMODE_CONV3X3, AMODE_TEMPORAL3, AMODE_CONV3D, AMODE_UPCONV2X2 = 0, 1, 2, 3, 4
EPI_LINEAR, EPI_GEGLU, EPI_TRANS = 0, 1, 2
# The 16-bit storage type of activations and packed weights: bf16 unless the process runs the fp16 build (VISTA_ACT_DTYPE=fp16, _lib.ACT_DTYPE).
# `BF16` is the historical name used throughout this file for "the storage type"; ACT is the same object under an honest name.
ACT = torch.float16 if _lib.ACT_DTYPE == "fp16" else torch.bfloat16
BF16 = ACT
F32 = torch.float32


class storage:
    """Context manager: run the enclosed ops with another 16-bit storage type -- `with ops.storage(torch.bfloat16):` switches ops.ACT / ops.BF16 (every
    function of this file reads them at call time) and the library _lib.load() hands out, and restores both on exit. A no-op when the type is already
    current (any bf16 process). Used by the first-stage VAE and the conditioner, which store bf16 in every process (the reference runs them without
    autocast; fp16's exponent range is not safe there), so that an fp16 process (VISTA_ACT_DTYPE=fp16) can run the whole pipeline: denoiser in fp16,
    decode / encode / CLIP tower in bf16. Weight packs are built under the context that uses them (a module is only ever run under one type).
    Process-global, not thread-local: do not interleave two storage types from concurrent host threads."""

    def __init__(self, dtype):
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("ops.storage: torch.bfloat16 or torch.float16")
        self.dtype, self.name = dtype, ("fp16" if dtype is torch.float16 else "bf16")

    def __enter__(self):
        global ACT, BF16
        self.prev = (ACT, _lib.CURRENT)
        ACT = BF16 = self.dtype
        _lib.CURRENT = self.name
        return self

    def __exit__(self, *exc):
        global ACT, BF16
        ACT = BF16 = self.prev[0]
        _lib.CURRENT = self.prev[1]
        return False


def bf16_storage(fn):
    """Decorator for forwards that always store bf16 (first-stage VAE, conditioner): ops.storage(torch.bfloat16) around the call."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **k):
        if ACT is torch.bfloat16:
            return fn(*a, **k)
        with storage(torch.bfloat16):
            return fn(*a, **k)
    return wrapped


def _stream():
    # raw hipStream_t of torch's current stream on the current device; the C-level getters cost ~1 us against ~9 us for
    # torch.cuda.current_stream() (1500 launches per step go through here)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise _lib.VistaHipError(f"{name}: tensor is on {t.device}; vista_amd kernels run on the MI355X only (no CPU fallback)")


def _rows2d(t, name):
    """(…, C) tensor whose rows are uniformly strided -> (rows, ld)."""
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: last dim must be contiguous")
    t2 = t.reshape(-1, t.shape[-1]) if t.is_contiguous() else t
    if t2.dim() != 2:
        raise ValueError(f"{name}: pass a 2-D strided view")
    return t2, t2.stride(0)


def ceil_to(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------- operand contract
# What the kernels ask of every tensor they are handed (include/vista_hip.h states it beside each prototype; the C entry points refuse the same
# with VK_EINVAL): the storage dtype, the device, contiguous rows, a base address and a row stride that suit the widest access the kernels make,
# and an extent that covers every row and column the geometry arguments name. Checked here, before the launch, so that a wrong slice in model code
# is a ValueError that names the operand instead of a read or a write past a tensor. Refused, never cloned: a silent copy of a 600 MB activation
# would hide the bug (the `_aligned16` clones of the small front-door operands are another matter and stay).
# Cost: one pass over attributes torch already holds; every test is in the one `if` of the accepting path (measured against the parent commit on the
# eager and the graph-replay step: profiles/operand_contract.txt).
class OperandError(ValueError):
    """An operand outside its contract: refused before any launch."""


def _refuse(name, t, rule):
    if not t.is_cuda:
        raise _lib.VistaHipError(f"{name}: tensor is on {t.device}; vista_amd kernels run on the MI355X only (no CPU fallback)")
    raise OperandError(f"{name}: {rule} (got {tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}, address % 16 = {t.data_ptr() & 15})")


def _operand(t, name, dtype, dev, align, rows, cols, ld_mult=1, exact_cols=False):
    """t: a 2-D view with contiguous rows, of `dtype` on GPU `dev` (a device index: tensor.get_device(), -1 = not a GPU), base address a multiple of `align` bytes, row stride a multiple of `ld_mult`
    elements and >= its columns, >= rows x cols (exact_cols: exactly cols columns). Returns the row stride."""
    sh, st = t.shape, t.stride()
    if (t.dtype is dtype and len(sh) == 2 and st[1] == 1 and t.get_device() == dev and dev >= 0 and (t.data_ptr() & (align - 1)) == 0 and st[0] % ld_mult == 0
            and sh[0] >= rows and (sh[1] == cols if exact_cols else sh[1] >= cols) and (st[0] >= sh[1] or sh[0] == 1)):
        return st[0]
    if t.dtype is not dtype or not t.is_cuda:
        _refuse(name, t, f"dtype must be {dtype}")
    if t.get_device() != dev:
        _refuse(name, t, f"must be on cuda:{dev}, the device of the call's first operand")
    if len(sh) != 2 or st[1] != 1:
        _refuse(name, t, "must be a 2-D view with stride(-1) == 1")
    if t.data_ptr() & (align - 1):
        _refuse(name, t, f"base address must be a multiple of {align} bytes")
    if st[0] % ld_mult or (st[0] < sh[1] and sh[0] != 1):
        _refuse(name, t, f"row stride must be a multiple of {ld_mult} elements and cover the row")
    _refuse(name, t, f"needs at least {rows} rows and {'exactly' if exact_cols else 'at least'} {cols} columns")


def _token_rows(t, name, dtype, dev, align, rows, cols):
    """_operand for a token-major tensor that may be 3-D (n_img, S, ld-strided C): its rows, flattened, must be uniformly strided."""
    if t.dim() == 3 and t.stride(0) == t.shape[1] * t.stride(1):
        t = t.as_strided((t.shape[0] * t.shape[1], t.shape[2]), (t.stride(1), t.stride(2)), t.storage_offset())
    return _operand(t, name, dtype, dev, align, rows, cols)


def _affine(gamma, beta, Cc, dev):
    """gamma / beta of a norm over Cc channels: fp32, contiguous, exactly Cc long, on the input's device."""
    _dense(gamma, "gamma", F32, dev, 4, Cc)
    _dense(beta, "beta", F32, dev, 4, Cc)


def _dense(t, name, dtype, dev, align, numel):
    """t: contiguous, of `dtype` on `dev`, base address a multiple of `align` bytes, exactly `numel` elements (what the geometry arguments state)."""
    if t.dtype is dtype and t.get_device() == dev and dev >= 0 and (t.data_ptr() & (align - 1)) == 0 and t.numel() == numel and t.is_contiguous():
        return
    if t.dtype is not dtype or not t.is_cuda:
        _refuse(name, t, f"dtype must be {dtype}")
    if t.get_device() != dev:
        _refuse(name, t, f"must be on cuda:{dev}, the device of the call's first operand")
    if not t.is_contiguous():
        _refuse(name, t, "must be contiguous")
    if t.data_ptr() & (align - 1):
        _refuse(name, t, f"base address must be a multiple of {align} bytes")
    _refuse(name, t, f"must hold exactly {numel} elements, the extent the geometry arguments state")


# ---------------------------------------------------------------------------------------------- weight packing
class PackedWeight:
    """bf16 [ceil256(N)][K] weight (K contiguous) + f32 bias, laid out for vk_gemm_bf16. `colsum` (f32 [Np]) marks a weight with a
    LayerNorm folded in (pack_*_ln): wt = gamma (.) W, bias = W beta + b, colsum = row sums of the bf16-rounded wt."""

    __slots__ = ("wt", "bias", "N", "K", "geglu", "colsum", "ln_eps", "ffout", "classes")

    def __init__(self, wt, bias, N, K, geglu=False, colsum=None, ln_eps=0.0, ffout=False, classes=1):
        for name, t in (("wt", wt), ("bias", bias), ("colsum", colsum)):   # operand contract, once per pack: 16-byte LDS-DMA pieces / float4 loads
            if t is not None and (t.data_ptr() & 15 or not t.is_contiguous() or t.device != wt.device):
                _refuse(f"PackedWeight.{name}", t, "must be contiguous, 16-byte aligned and on the weight's device")
        self.wt, self.bias, self.N, self.K, self.geglu, self.colsum, self.ln_eps = wt, bias, N, K, geglu, colsum, ln_eps
        self.ffout = ffout  # laid out for vk_ff_fused_bf16's out-projection (pack_ff_out): not a vk_gemm_bf16 operand
        self.classes = classes  # 4: the class packs of a folded upsample convolution (pack_upconv2x2), one after another; only ops.upconv2x2 takes it


def _finish_pack(w2d, bias, device, geglu=False, ln=None):
    """ln = (gamma, beta, eps): fold `LayerNorm(x) @ W^T + b` into the GEMM (include/vista_hip.h, VkGemmDesc.ln_*):
    LN(x) W^T + b = rstd * (x W'^T - mean * s) + t with W' = gamma (.) W, s_n = sum_k bf16(W')[n][k], t = W beta + b."""
    N, K = w2d.shape
    Kp = ceil_to(K, 64)
    Np = max(ceil_to(N, 256), ceil_to(N, 320))  # readable by every block-tile variant (128/256/320-wide) without bounds checks
    colsum, eps = None, 0.0
    if ln is not None:
        gamma, beta, eps = ln
        if Kp != K:
            raise ValueError("LayerNorm fold needs K % 64 == 0")
        gamma, beta = gamma.detach().float().to(w2d.device), beta.detach().float().to(w2d.device)
        t = w2d @ beta
        bias = t if bias is None else bias.to(w2d.device) + t
        w2d = w2d * gamma[None, :]
    wt = torch.zeros((Np, Kp), dtype=BF16, device=device)
    wt[:N, :K] = w2d.to(device=device, dtype=BF16)
    if ln is not None:
        colsum = wt.float().sum(dim=1).contiguous()  # of the ROUNDED weights: the mean term then cancels exactly in the epilogue
    b = None
    if bias is not None:
        b = torch.zeros((Np,), dtype=F32, device=device)
        b[:N] = bias.to(device=device, dtype=F32)
    return PackedWeight(wt, b, ceil_to(N, 4), Kp, geglu, colsum, float(eps))  # N % 4 == 0 for the 4-column epilogue quads; the extra rows/bias are zero


def _ln_tuple(norm):
    """(gamma, beta, eps) of a LayerNorm parameter container."""
    return (norm.weight, norm.bias, norm.eps)


KPERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def pack_linear(weight, bias=None, device="cuda", ln=None):
    """nn.Linear.weight [N][K] (or a 1x1 conv weight [N][K][1][1]). ln: LayerNorm container applied to the input (folded)."""
    return _finish_pack(weight.detach().reshape(weight.shape[0], -1).float(), None if bias is None else bias.detach().float(), device,
                        ln=None if ln is None else _ln_tuple(ln))


def ff_out_layout(w):
    """[N][K] -> the out-projection operand of vk_ff_fused_bf16 (include/vista_hip.h): K permuted inside every 16-group to KPERM16 (the order in
    which a lane of the in-projection's 32x32 MFMA accumulator holds the hidden units), then chunk-major [K / 32][N][32] so that a 32-wide
    hidden chunk of all N rows is one contiguous 20 KB block (whole cache lines per LDS-DMA piece). Pure index shuffle (CPU-testable)."""
    N, K = w.shape
    if K % 32:
        raise ValueError("ff_out_layout needs K % 32 == 0")
    w = w.reshape(N, K // 16, 16)[:, :, list(KPERM16)].reshape(N, K // 32, 32)
    return w.permute(1, 0, 2).contiguous().reshape(K // 32 * N, 32)


def pack_ff_out(weight, bias=None, device="cuda"):
    """FeedForward.net[2] weight [N][K] for ops.ff_fused (bf16, ff_out_layout; bias f32)."""
    w = weight.detach().reshape(weight.shape[0], -1).float()
    N, K = w.shape
    b = None if bias is None else bias.detach().to(device=device, dtype=F32).contiguous()
    return PackedWeight(ff_out_layout(w).to(device=device, dtype=BF16), b, N, K, ffout=True)


def pack_rows_as_weight(t, N, K):
    """Treat an activation buffer whose first N rows are [N][K] bf16 (K contiguous) as the weight operand of a GEMM
    (q.k^T and P.v of the VAE decoder's AttnBlock). The caller guarantees the rows up to the next tile boundary are readable."""
    _need(t, BF16, "t")
    return PackedWeight(t, None, N, K)


def pack_linear_cat(weights, device="cuda", ln=None):
    """Several bias-free Linear weights sharing the input, concatenated along N (fused q|k or q|k|v projection)."""
    return _finish_pack(torch.cat([w.detach().float() for w in weights], 0), None, device, ln=None if ln is None else _ln_tuple(ln))


def geglu_perm(nout):
    """Row order of a packed GEGLU weight: every 32-row MFMA fragment holds [16 value rows | the 16 gate rows of the same output
    columns], so the GEMM epilogue forms value*gelu(gate) inside a lane for any block / wave tile shape."""
    if nout % 16:
        raise ValueError("GEGLU width must be a multiple of 16")
    idx = torch.arange(nout).reshape(-1, 16)
    return torch.stack([idx, idx + nout], 1).reshape(-1)  # [v-block0, g-block0, v-block1, g-block1, ...]


def pack_geglu(weight, bias, device="cuda", ln=None):
    """GEGLU.proj weight [2*Nout][K]: value rows then gate rows (attention.py:85-92), packed in `geglu_perm` order."""
    w = weight.detach().float()
    b = bias.detach().float()
    perm = geglu_perm(w.shape[0] // 2).to(w.device)
    return _finish_pack(w[perm], b[perm], device, geglu=True, ln=None if ln is None else _ln_tuple(ln))


def _slab_major(w):
    """[Cout][taps][Cin] (Cin % 64 == 0) -> [Cout][Cin/64][taps][64] flattened along K: the implicit-GEMM K-loop visits all taps of one
    64-channel slab on consecutive K-steps (the input rows a tile re-reads then sit in L2; csrc/gemm.hip header)."""
    cout, taps, cin = w.shape
    return w.reshape(cout, taps, cin // 64, 64).permute(0, 2, 1, 3).reshape(cout, taps * cin)


def pack_conv3x3(weight, bias=None, cin_pad=None, device="cuda"):
    """nn.Conv2d weight [Cout][Cin][3][3] -> [Cout][Cin(_pad)/64][ky][kx][64]."""
    w = weight.detach().float().permute(0, 2, 3, 1).contiguous()  # Cout, ky, kx, Cin
    cout, _, _, cin = w.shape
    cp = cin_pad or ceil_to(cin, 64)
    if cp != cin:
        w = torch.nn.functional.pad(w, (0, cp - cin))
    return _finish_pack(_slab_major(w.reshape(cout, 9, cp)), None if bias is None else bias.detach().float(), device)


UPCONV_ROWS = (((0,), (1, 2)), ((0, 1), (2,)))  # [parity a][dy] -> the taps ky of the 3x3 kernel that read source row i + a - 1 + dy


def fold_upconv2x2(weight):
    """conv3x3(pad 1) after a nearest x2 upsample as four 2x2 convolutions of the SOURCE image, one per output parity class (a, b): output pixel
    (2i + a, 2j + b) reads source pixels (i + a - 1 + dy, j + b - 1 + dx), dy, dx in {0, 1}, because tap ky of an output row of parity a reads
    source row (2i + a + ky - 1) >> 1 -- a = 0: i - 1, i, i; a = 1: i, i, i + 1 (UPCONV_ROWS), and likewise in x. Zero padding of the source
    reproduces the borders (upsampled row -1 / 2H is source row -1 / H). [Cout][Cin][3][3] -> [4][Cout][Cin][2][2] in the arithmetic of `weight`
    (fp32 in the packs, float64 in the tests), class index 2a + b; the taps are summed over ky first (in tap order), then over kx."""
    w = weight.detach()
    classes = []
    for a in (0, 1):
        rows = [sum(w[:, :, ky] for ky in UPCONV_ROWS[a][dy]) for dy in (0, 1)]          # [dy] -> [Cout][Cin][3 (kx)]
        for b in (0, 1):
            classes.append(torch.stack([torch.stack([sum(r[:, :, kx] for kx in UPCONV_ROWS[b][dx]) for dx in (0, 1)], -1) for r in rows], -2))
    return torch.stack(classes)


def pack_upconv2x2(weight, bias=None, device="cuda"):
    """The Upsample convolution (openaimodel.py:100-102) for ops.upconv2x2: the 3x3 weight [Cout][Cin][3][3] folded in fp32 from the module's master
    weights into the four class weights of fold_upconv2x2 (4/9 of the multiply-adds), rounded ONCE to the storage type, each class packed like a
    conv weight with four taps -- [Cout][Cin/64][dy][dx][64], rows zero-padded as every pack -- and the four packs stored one after another in a
    single allocation, class 2a + b at rows [(2a + b) * Np, (2a + b + 1) * Np); one bias vector."""
    w = fold_upconv2x2(weight.detach().float())                      # [4][Cout][Cin][2][2]
    _, cout, cin = w.shape[:3]
    if cin % 64:
        raise ValueError("pack_upconv2x2 needs Cin % 64 == 0")
    Np = max(ceil_to(cout, 256), ceil_to(cout, 320))
    wt = torch.zeros((4 * Np, 4 * cin), dtype=BF16, device=device)
    for c in range(4):
        wt[c * Np:c * Np + cout] = _slab_major(w[c].permute(0, 2, 3, 1).reshape(cout, 4, cin)).to(device=device, dtype=BF16)
    b = None
    if bias is not None:
        b = torch.zeros((Np,), dtype=F32, device=device)
        b[:cout] = bias.detach().to(device=device, dtype=F32)
    return PackedWeight(wt, b, ceil_to(cout, 4), 4 * cin, classes=4)


def unpack_upconv2x2(pw, cout):
    """The class weights of a pack_upconv2x2 pack, in its storage type: [4][Cout][Cin][2][2] (tests; the references of the folded form)."""
    Np, cin = pw.wt.shape[0] // 4, pw.K // 4
    return pw.wt.view(4, Np, cin // 64, 2, 2, 64)[:, :cout].permute(0, 1, 2, 5, 3, 4).reshape(4, cout, cin, 2, 2)


def pack_conv_t3(weight, bias=None, device="cuda", cin_pad=None):
    """nn.Conv3d weight [Cout][Cin][3][1][1] -> [Cout][Cin(_pad)/64][kt][64]."""
    w = weight.detach().float()[:, :, :, 0, 0].permute(0, 2, 1).contiguous()
    cout, _, cin = w.shape
    if cin_pad and cin_pad != cin:
        w = torch.nn.functional.pad(w, (0, cin_pad - cin))
        cin = cin_pad
    if cin % 64:
        raise ValueError("temporal conv needs Cin % 64 == 0")
    return _finish_pack(_slab_major(w), None if bias is None else bias.detach().float(), device)


# ---------------------------------------------------------------------------------------------- GEMM family
TILE_CFG = 0  # 0 = auto; tests force 1..7 to cover every block-tile variant (include/vista_hip.h, VkGemmDesc.tile_cfg)


SPLITK_WS_BYTES = int(os.environ.get("VISTA_SPLITK_WS_MB", "160")) << 20  # fp32 split-K workspace per (device, stream) (0 disables split-K)
class _SplitKTLS(threading.local):
    def __init__(self):
        self.ws = {}


_SPLITK_WS = _SplitKTLS()


class _GraphTLS(threading.local):
    """Per host thread: `depth` > 0 inside graph_workspace() (then _splitk_workspace hands out the graph workspace instead of a per-stream buffer);
    `ws` = {device: the ONE workspace of every hipGraph warm-up / capture of THIS thread on that device}. Thread-local like _SplitKTLS, so a worker
    thread's buffer goes with the thread (a module-level dict keyed by thread ident leaked 160 MiB per thread and let a new thread inherit
    a dead thread's buffer) -- unless a captured graph still needs it: sampling.FusedLoop keeps graph_workspace_tensor() in its graph-cache entry,
    because the graph's split-K launches have the pointer baked in. A graph may be replayed from any thread, one replay at a time."""

    def __init__(self):
        self.depth = 0
        self.slot = 0    # the workspace slot of the innermost graph_workspace()
        self.ws = {}     # device (slot 0) or (device, slot) -> workspace


_GRAPH_TLS = _GraphTLS()


class graph_workspace:
    """Context manager for hipGraph warm-up + capture (sampling.FusedLoop): every split-K GEMM enqueued inside uses ONE workspace per (thread,
    device, slot), allocated here -- OUTSIDE any capture, so it belongs to the ordinary caching allocator and not to a graph's private pool --
    instead of a fresh 160 MB buffer per (thread, stream). Graph replays run on the launch stream one after the other, so they may share it; eager
    work on other streams keeps its per-stream buffers. `slot` > 0: a workspace of its own for a graph that is replayed CONCURRENTLY with the
    slot-0 graphs on another stream (the two guidance halves of a step, FusedLoop(cfg_streams=True))."""

    def __init__(self, slot=0):
        self.slot = slot

    def __enter__(self):
        dev = torch._C._cuda_getDevice()
        key = dev if self.slot == 0 else (dev, self.slot)
        if SPLITK_WS_BYTES and key not in _GRAPH_TLS.ws:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ops.graph_workspace must be entered before the capture starts")
            _GRAPH_TLS.ws[key] = torch.empty(SPLITK_WS_BYTES // 4, dtype=F32, device=f"cuda:{dev}")
        _GRAPH_TLS.depth += 1
        self._outer, _GRAPH_TLS.slot = _GRAPH_TLS.slot, self.slot
        return self

    def __exit__(self, *exc):
        _GRAPH_TLS.depth -= 1
        _GRAPH_TLS.slot = self._outer
        return False


def _graph_ws_key():
    dev, slot = torch._C._cuda_getDevice(), _GRAPH_TLS.slot
    return dev if slot == 0 else (dev, slot)


def graph_workspace_tensor():
    """The calling thread's graph workspace on the current device (inside graph_workspace(slot): that slot's; None before the first
    graph_workspace()): a graph-cache entry holds a reference to it for as long as its graph lives."""
    return _GRAPH_TLS.ws.get(_graph_ws_key())


def _splitk_workspace(stream):
    """One workspace per (device, stream) of each host thread: launches on one stream are ordered, so they may share it; GEMMs in flight on
    different streams must not (include/vista_hip.h, VkGemmDesc.splitk_ws), and thread ranks (tests) share a stream but enqueue
    concurrently. Held in thread-local storage, so a worker thread's buffers are released when the thread exits. Inside
    graph_workspace() (hipGraph warm-up / capture) the thread's single graph workspace of the device is used instead."""
    if _GRAPH_TLS.depth > 0:
        return _GRAPH_TLS.ws[_graph_ws_key()]
    key = (torch._C._cuda_getDevice(), stream.value)
    ws = _SPLITK_WS.ws.get(key)
    if ws is None:
        ws = _SPLITK_WS.ws[key] = torch.empty(SPLITK_WS_BYTES // 4, dtype=F32, device=f"cuda:{key[0]}")
    return ws


class RowStats:
    """Per-row (sum, sum of squares) partials of an activation tensor, f32 [parts][M][2] (include/vista_hip.h, VkGemmDesc.ln_stats):
    written by the producing GEMM's epilogue (linear(..., emit_stats=True)) or by rowstats(); consumed by a GEMM with a folded LayerNorm."""

    __slots__ = ("t", "parts", "M")

    def __init__(self, t, parts, M):
        self.t, self.parts, self.M = t, parts, M


ROW_RANGE = None  # tests: (m_begin, m_end) -> the next GEMM calls compute only those output rows (VkGemmDesc.m_begin / m_end, ABI v5)

# GroupNorm statistics from the producing convolution's epilogue (VkGemmDesc.gnstat_out, ABI v6): 1 = a conv3x3 / conv_t3 call that is handed a
# GnPartials and whose launch can emit them (vk_gemm_gnstat_fit) does, and groupnorm(..., gn=...) then skips its statistics pass; 0 = the
# three-launch GroupNorm everywhere (A/B hook, VISTA_GN_EPI). A launch-affecting switch: part of the hipGraph cache key (sampling.py).
GN_EPI = int(os.environ.get("VISTA_GN_EPI", "1"))


class GnPartials:
    """Stage-1 GroupNorm partial sums of a tensor, written by the epilogue of the convolution that produced it: f32 [n_img * nchunks][64] =
    [32 group sums | 32 group sums of squares] per 64 consecutive rows (include/vista_hip.h, VkGemmDesc.gnstat_out). `t` stays None when the
    producer's launch could not emit them (split-K, a sixteen-wave tile, halo frames, rows per image not a multiple of 64 ...): the consumer
    then runs its own statistics pass -- same result up to the summation order. Consumed by ONE groupnorm call (the fold works in place)."""

    __slots__ = ("t", "nchunks", "rows", "C")

    def __init__(self):
        self.t, self.nchunks, self.rows, self.C = None, 0, 0, 0


def _prepare(desc):
    """What every vk_gemm_* call about `desc`, query or launch, must see alike: the forced tile variant, the row range and the split-K workspace
    (the launcher's decisions read all three). Returns the stream."""
    desc.tile_cfg = TILE_CFG
    if ROW_RANGE is not None:
        desc.m_begin, desc.m_end = ROW_RANGE
    stream = _stream()
    if SPLITK_WS_BYTES:
        ws = _splitk_workspace(stream)
        desc.splitk_ws, desc.splitk_ws_bytes = _p(ws), ws.numel() * 4
    return stream


def _ask_gn(d, gn, rows_per_image, device):
    """Before the launch: if this GEMM can emit the GroupNorm statistics of its output, give it the buffer."""
    if gn is None or not GN_EPI or ROW_RANGE is not None:   # (a row-range launch never emits)
        return
    d.gn_rows = int(rows_per_image)
    _prepare(d)
    slots = _lib.load().vk_gemm_gnstat_fit(C.byref(d))
    if slots < 0:
        raise _lib.VistaHipError(f"vk_gemm_gnstat_fit failed with code {slots}")
    if slots > 0:
        gn.t = torch.empty(slots * 64, dtype=F32, device=device)
        gn.nchunks, gn.rows, gn.C = int(rows_per_image) // 64, d.M, d.N
        d.gnstat_out = _p(gn.t)


def _gemm(desc, emit_stats=False, device=None):
    lib = _lib.load()
    stream = _prepare(desc)
    stats = None
    if emit_stats:
        parts = lib.vk_gemm_rowstat_parts(C.byref(desc))
        if parts <= 0:
            raise _lib.VistaHipError(f"vk_gemm_rowstat_parts failed with code {parts}")
        stats = RowStats(torch.empty((parts, desc.M, 2), dtype=F32, device=device), parts, desc.M)
        desc.rowstat_out = _p(stats.t)
    check(lib.vk_gemm_bf16(C.byref(desc), stream), "vk_gemm_bf16")
    return stats


def _fill_ln(d, pw, ln, M):
    """ln: RowStats of the GEMM's input rows; pw must carry a folded LayerNorm (and vice versa)."""
    if (ln is None) != (pw.colsum is None):
        raise ValueError("a weight packed with a folded LayerNorm needs the input's RowStats (ln=...), and only such a weight takes them")
    if ln is not None:
        if ln.M != M:
            raise ValueError(f"RowStats of {ln.M} rows passed to a GEMM over {M} rows")
        d.ln_stats, d.ln_parts, d.ln_colsum, d.ln_eps = _p(ln.t), ln.parts, _p(pw.colsum), pw.ln_eps


def _fill_epilogue(d, pw, out, M, rowvec, rows_per_vec, res1, res2, alpha, beta, rowvec2=None, ncols=None, out_dtype=None):
    """The epilogue operands of a GEMM over M rows into `out` (M x ncols; ncols: pw.N unless the caller says otherwise -- GEGLU, mx8_cols), each
    held to the operand contract: out 8-byte aligned (fp32: 16) with ldc % 4, residuals 8-byte aligned with ld % 4 and >= M x N, row vectors fp32,
    16-byte aligned, ldv % 4, >= ceil(M / rows_per_vec) x N. out_dtype: the fp8 GEGLU's MX output (e4m3 bytes, 16-byte aligned) instead of a 16-bit / fp32 one."""
    dev = pw.wt.get_device()
    d.Wt = _p(pw.wt)
    d.bias = _p(pw.bias)
    d.M, d.N, d.K = M, pw.N, pw.K
    if out is None:   # a plan query asked before the output exists (upconv2x2_fits): any 16-byte aligned device pointer, never written
        f32, d.out, d.ldc = False, d.Wt, pw.N
    else:
        f32 = out.dtype is F32
        d.ldc = _operand(out, "out", out_dtype or (F32 if f32 else BF16), dev, 16 if (f32 or out_dtype is not None) else 8, M, pw.N if ncols is None else ncols, 4,
                         exact_cols=True)
        d.out = _p(out)
    d.out_f32 = 1 if f32 else 0
    d.alpha, d.beta = float(alpha), float(beta)
    if rowvec is not None or rowvec2 is not None:
        if int(rows_per_vec) <= 0:
            raise ValueError("rowvec / rowvec2: rows_per_vec must be positive")
        nvec = (M + int(rows_per_vec) - 1) // int(rows_per_vec)
    if rowvec is not None:
        d.rowvec, d.ldv, d.rows_per_vec = _p(rowvec), _operand(rowvec, "rowvec", F32, dev, 16, nvec, pw.N, 4), int(rows_per_vec)
    if res1 is not None:
        r, ld = _rows2d(res1, "res1")
        d.res1, d.ld_res1 = _p(r), _operand(r, "res1", BF16, dev, 8, M, pw.N, 4)
    if res2 is not None:
        r, ld = _rows2d(res2, "res2")
        d.res2, d.ld_res2 = _p(r), _operand(r, "res2", BF16, dev, 8, M, pw.N, 4)
    if rowvec2 is not None:
        if res2 is None:
            raise ValueError("rowvec2 is added to res2 (out = alpha*(...) + beta*(res2 + rowvec2))")
        if rowvec is not None and rowvec.stride(0) != rowvec2.stride(0):
            raise ValueError("rowvec and rowvec2 share one row stride")
        d.rowvec2, d.ldv, d.rows_per_vec = _p(rowvec2), _operand(rowvec2, "rowvec2", F32, dev, 16, nvec, pw.N, 4), int(rows_per_vec)


def linear(x, pw, *, out=None, out_f32=False, rowvec=None, rows_per_vec=0, res1=None, res2=None, alpha=1.0, beta=0.0, rowvec2=None,
           x2=None, ln=None, emit_stats=False, act=None, mx8_cols=0, alt_cols_from=0):
    """out = alpha*(act(X @ W^T + bias + rowvec[row // rows_per_vec]) + res1) + beta*(res2 + rowvec2[row // rows_per_vec]); act: None | "gelu".
    x: (..., K) bf16. x2: second source of a channel concat, X = [x | x2] (never materialised). ln: RowStats of x's rows when pw has
    a LayerNorm folded in (X = LayerNorm(x)). emit_stats: also return the RowStats of the (bf16) output -> (out, stats)."""
    x2d, lda = _rows2d(x, "x")
    M = x2d.shape[0]
    k_in = x2d.shape[1]
    _operand(x2d, "x", BF16, pw.wt.get_device(), 16, M, k_in, 8)
    d = VkGemmDesc()
    if x2 is not None:
        b2d, ldb = _rows2d(x2, "x2")
        if b2d.shape[0] != M:
            raise ValueError("linear: x and x2 must have the same rows")
        _operand(b2d, "x2", BF16, pw.wt.get_device(), 16, M, b2d.shape[1], 8)
        d.A2, d.lda2, d.k_split = _p(b2d), ldb, k_in
        k_in += b2d.shape[1]
    if k_in != pw.K:
        raise ValueError(f"linear: K mismatch {k_in} vs {pw.K}")
    if pw.ffout:
        raise ValueError("linear: this weight is laid out for ff_fused (pack_ff_out), not for vk_gemm_bf16")
    if pw.geglu:
        nout = pw.N // 2
        if out is None:
            out = torch.empty((M, nout), dtype=BF16, device=x.device)
    elif out is None:
        out = torch.empty((M, pw.N - mx8_cols), dtype=F32 if out_f32 else BF16, device=x.device)
    d.A, d.lda = _p(x2d), lda
    d.amode = AMODE_DENSE
    d.epi = EPI_GEGLU if pw.geglu else EPI_LINEAR
    _fill_epilogue(d, pw, out, M, rowvec, rows_per_vec, res1, res2, alpha, beta, rowvec2, ncols=pw.N // 2 if pw.geglu else pw.N - mx8_cols)
    _fill_ln(d, pw, ln, M)
    mx = None
    if mx8_cols:
        # BASELINE config 5: the leading mx8_cols output columns leave as MX fp8 (e4m3 bytes + one E8M0 scale per row and 32 columns), the rest as
        # bf16 into `out` (M, N - mx8_cols): the q | k blocks of the fused q|k|v projection for the fp8 QK^T (include/vista_hip.h, mx8_*)
        if pw.geglu or emit_stats or mx8_cols % 320 or pw.N % 320 or out.shape[1] != pw.N - mx8_cols:
            raise ValueError("linear: mx8_cols needs a LINEAR weight, N and mx8_cols multiples of 320, no emit_stats")
        mx = (torch.empty((M, mx8_cols), dtype=torch.uint8, device=x.device), torch.empty((M, mx8_cols // 32), dtype=torch.uint8, device=x.device))
        d.mx8_out, d.mx8_scales, d.mx8_cols, d.ld_mx8, d.ld_mx8s = _p(mx[0]), _p(mx[1]), mx8_cols, mx8_cols, mx8_cols // 32
    if act is not None:
        if act != "gelu" or pw.geglu:
            raise ValueError("linear: act must be None or 'gelu' (exact-erf GELU in the LINEAR epilogue)")
        d.act = 1
    # fp16 build: output columns from alt_cols_from on leave as bf16 (the V block of a fused q|k|v projection: the attention kernels keep P.V in
    # bf16 in both builds, include/vista_hip.h). Ignored by the bf16 build, where every column is bf16 anyway.
    d.alt_cols_from = int(alt_cols_from)
    stats = _gemm(d, emit_stats, x.device)
    if mx is not None:
        return out, mx[0], mx[1]
    return (out, stats) if emit_stats else out


def linear_vt(x, pw, S, out=None, ln=None):
    """V^T projection for spatial attention: x (n_img*S, K) -> out (n_img, N, S) bf16 = (x @ W^T + bias)^T per image (EPI_TRANS)."""
    x2, lda = _rows2d(x, "x")
    M = x2.shape[0]
    _operand(x2, "x", BF16, pw.wt.get_device(), 16, M, pw.K, 8, exact_cols=True)
    if S <= 0 or M % S:
        raise ValueError(f"linear_vt: x has {M} rows, not a multiple of S = {S}")
    if out is None:
        out = torch.empty((M // S, pw.N, S), dtype=BF16, device=x.device)
    elif out.dtype != BF16 or not out.is_contiguous() or out.shape != (M // S, pw.N, S):
        raise ValueError("linear_vt: out must be contiguous bf16 (n_img, N, S)")
    _dense(out, "out", BF16, pw.wt.get_device(), 8, M * pw.N)
    d = VkGemmDesc()
    d.A, d.lda = _p(x2), lda
    d.amode, d.epi = AMODE_DENSE, EPI_TRANS
    d.bias = _p(pw.bias)
    d.Wt, d.M, d.N, d.K, d.out, d.ldc, d.S = _p(pw.wt), M, pw.N, pw.K, _p(out), S, S
    d.alpha = 1.0
    _fill_ln(d, pw, ln, M)
    _gemm(d)
    return out


def rowstats(x):
    """RowStats (one slab) of x (..., C) bf16 by a read-only pass: for tensors whose producer is not a GEMM epilogue on this rank."""
    x2, ldx = _rows2d(x, "x")
    M, Cc = x2.shape
    _operand(x2, "x", BF16, x.get_device(), 16, M, Cc, 8)
    st = torch.empty((1, M, 2), dtype=F32, device=x.device)
    check(_lib.load().vk_rowstats_bf16(_p(x2), _p(st), M, Cc, ldx, _stream()), "vk_rowstats_bf16")
    return RowStats(st, 1, M)


FF_FUSED_WIDTH, FF_FUSED_MAX_HIDDEN = 320, 1280
FF_FUSED_DBG_BUF = None
FF_FUSED_DBG = 0  # timing experiments only (tools/ff_fused_probe.py), honoured by a library built with -DFF_TIMING; the product build ignores it


def ff_fused_ok(pw_in, pw_out):
    """Shapes vk_ff_fused_bf16 covers: the level-0 FeedForward (width 320, hidden a multiple of 64 up to 1280)."""
    return (pw_in.geglu and pw_in.K == FF_FUSED_WIDTH and pw_out.N == FF_FUSED_WIDTH and pw_in.N == 2 * pw_out.K
            and pw_out.K % 64 == 0 and 128 <= pw_out.K <= FF_FUSED_MAX_HIDDEN)


def ff_fused(x, pw_in, pw_out, *, out=None, rowvec=None, rows_per_vec=0, res1=None, res2=None, alpha=1.0, beta=0.0, rowvec2=None, ln=None,
             emit_stats=False):
    """linear(linear(x, pw_in, ln=ln), pw_out', ...epilogue) in ONE kernel (vk_ff_fused_bf16): pw_in = pack_geglu(...), pw_out' =
    pack_ff_out(...). The hidden activation never leaves the CU. Returns out, or (out, RowStats) with emit_stats."""
    x2d, lda = _rows2d(x, "x")
    M = x2d.shape[0]
    _operand(x2d, "x", BF16, pw_in.wt.get_device(), 16, M, x2d.shape[1], 8)
    if not ff_fused_ok(pw_in, pw_out) or not pw_out.ffout or x2d.shape[1] != pw_in.K:
        raise ValueError("ff_fused: needs a packed GEGLU weight [2H][320] and a pack_ff_out weight [320][H], H % 64 == 0, 128 <= H <= 1280")
    if out is None:
        out = torch.empty((M, pw_out.N), dtype=BF16, device=x.device)
    g = VkGemmDesc()
    g.A, g.lda = _p(x2d), lda
    g.amode, g.epi = AMODE_DENSE, EPI_GEGLU
    g.Wt, g.bias, g.M, g.N, g.K = _p(pw_in.wt), _p(pw_in.bias), M, pw_in.N, pw_in.K
    g.out, g.ldc = _p(out), out.stride(0)   # (ignored by the kernel; validate() wants a non-NULL pointer)
    g.alpha = 1.0
    g.tile_cfg = FF_FUSED_DBG
    if FF_FUSED_DBG == 8 and FF_FUSED_DBG_BUF is not None:
        g.splitk_ws = _p(FF_FUSED_DBG_BUF)
    _fill_ln(g, pw_in, ln, M)
    d = VkGemmDesc()
    d.A, d.lda = _p(x2d), lda               # (ignored)
    d.amode, d.epi = AMODE_DENSE, EPI_LINEAR
    _fill_epilogue(d, pw_out, out, M, rowvec, rows_per_vec, res1, res2, alpha, beta, rowvec2)
    lib = _lib.load()
    stats = None
    if emit_stats:
        parts = lib.vk_ff_fused_rowstat_parts()
        stats = RowStats(torch.empty((parts, M, 2), dtype=F32, device=x.device), parts, M)
        d.rowstat_out = _p(stats.t)
    check(lib.vk_ff_fused_bf16(C.byref(g), C.byref(d), _stream()), "vk_ff_fused_bf16")
    return (out, stats) if emit_stats else out


def conv3x3(x, pw, n_img, H, W, *, stride=1, ups=1, out=None, out_f32=False, rowvec=None, res1=None, res2=None, alpha=1.0,
            beta=0.0, asym_pad=False, gn=None):
    """3x3 conv, pad 1, over token-major x (n_img, H*W, Cin); `ups`=2 applies a nearest x2 upsample to the source
    on the fly (Upsample.forward, openaimodel.py:100-102); stride 2 = Downsample (openaimodel.py:136)."""
    cin = x.shape[-1]
    _dense(x, "x", BF16, pw.wt.get_device(), 16, n_img * H * W * cin)
    if pw.K != 9 * cin:
        raise ValueError(f"conv3x3: weight K {pw.K} != 9*{cin}")
    He, We = H * ups, W * ups
    pad = 1 if asym_pad else 2  # asym_pad: F.pad(x, (0,1,0,1)) + conv pad 0 (VAE encoder Downsample, model.py:77-81)
    Hout = (He + pad - 3) // stride + 1
    Wout = (We + pad - 3) // stride + 1
    M = n_img * Hout * Wout
    if out is None:
        out = torch.empty((M, pw.N), dtype=F32 if out_f32 else BF16, device=x.device)
    d = VkGemmDesc()
    d.A, d.lda = _p(x), cin
    d.amode, d.epi = AMODE_CONV3X3, EPI_LINEAR
    d.H, d.Wd, d.Cin, d.Hout, d.Wout, d.stride, d.ups = H, W, cin, Hout, Wout, stride, ups
    d.asym_pad = 1 if asym_pad else 0
    _fill_epilogue(d, pw, out, M, rowvec, Hout * Wout, res1, res2, alpha, beta)
    _ask_gn(d, gn, Hout * Wout, x.device)   # gn: a GnPartials to fill with the GroupNorm statistics of `out` (the norm that follows this conv)
    _gemm(d)
    return (out.view(n_img, Hout * Wout, pw.N) if out.is_contiguous() else out), Hout, Wout


# Tile order of the folded upsample convolution (VkGemmDesc.tile_cfg bit 3): 0 = class-slowest, 1 = class-fastest (csrc/gemm_pipe.hip; both measured in
# profiles/upconv_fold.txt). Bitwise the same output either way.
UPCONV_CLASS_FASTEST = int(os.environ.get("VISTA_UPCONV_ORDER", "0")) != 0


def _upconv_desc(x, pw, n_img, H, W, rowvec, out):
    cin = x.shape[-1]
    d = VkGemmDesc()
    d.A, d.lda = _p(x), cin
    d.amode, d.epi = AMODE_UPCONV2X2, EPI_LINEAR
    d.H, d.Wd, d.Cin, d.Hout, d.Wout, d.stride, d.ups = H, W, cin, 2 * H, 2 * W, 1, 2
    _fill_epilogue(d, pw, out, n_img * 4 * H * W, rowvec, 4 * H * W, None, None, 1.0, 0.0)
    stream = _prepare(d)
    if UPCONV_CLASS_FASTEST:
        d.tile_cfg |= 8
    return d, stream


def upconv2x2_fits(x, pw, n_img, H, W, rowvec=None, out=None):
    """Does the library take the folded form of this upsample convolution (host arithmetic, no launch)? It does where the nine-tap form would run on
    the pipelined 256x320 kernel in one launch: Cout % 320 == 0 and enough rows to fill the chip; else the caller runs ops.conv3x3(..., ups=2)."""
    d, _ = _upconv_desc(x, pw, n_img, H, W, rowvec, out)   # (out None: the answer depends on alignment and extents only)
    return _lib.load().vk_gemm_tile_choice(C.byref(d)) > 0


def upconv2x2(x, pw, n_img, H, W, rowvec=None, out=None):
    """Upsample.forward (openaimodel.py:100-102: nearest x2, then conv3x3 pad 1) on a pack_upconv2x2 pack: four 2x2 class convolutions of the source,
    K = 4 Cin instead of 9 Cin, scattered to the output pixels of their parity. x (n_img, H*W, Cin) -> ((n_img, 4*H*W, Cout), 2H, 2W). Raises where the
    library declines the shape (upconv2x2_fits): there is no quiet change of algorithm here."""
    cin = x.shape[-1]
    _dense(x, "x", BF16, pw.wt.get_device(), 16, n_img * H * W * cin)
    if pw.classes != 4 or pw.K != 4 * cin:
        raise ValueError(f"upconv2x2: needs a pack_upconv2x2 weight with K = 4*{cin}")
    M = n_img * 4 * H * W
    if out is None:
        out = torch.empty((M, pw.N), dtype=BF16, device=x.device)
    d, stream = _upconv_desc(x, pw, n_img, H, W, rowvec, out)
    check(_lib.load().vk_gemm_bf16(C.byref(d), stream), "vk_gemm_bf16 (folded upsample convolution)")
    return (out.view(n_img, 4 * H * W, pw.N) if out.is_contiguous() else out), 2 * H, 2 * W


def conv_t3(x, pw, T, S, *, out=None, out_f32=False, rowvec=None, res1=None, res2=None, alpha=1.0, beta=0.0, halo_prev=None,
            halo_next=None, gn=None):
    """3x1x1 temporal conv, pad (1,0,0) (video_model.py:38-52) over x ((b t), S, C). halo_prev / halo_next: (clips, S, C) frames
    adjacent to the local frame range (frame-sharded multi-GPU); None = zero padding."""
    cin = x.shape[-1]
    if x.dim() != 3 or T <= 0 or x.shape[0] % T or x.shape[1] != S:
        raise ValueError(f"conv_t3: x must be ((b t), S, C) with (b t) a multiple of T = {T} and S = {S}, got {tuple(x.shape)}")
    _dense(x, "x", BF16, pw.wt.get_device(), 16, x.shape[0] * S * cin)
    if pw.K != 3 * cin:
        raise ValueError("conv_t3: weight K mismatch")
    M = x.shape[0] * x.shape[1]
    if out is None:
        out = torch.empty((M, pw.N), dtype=F32 if out_f32 else BF16, device=x.device)
    d = VkGemmDesc()
    d.A, d.lda = _p(x), cin
    d.amode, d.epi = AMODE_TEMPORAL3, EPI_LINEAR
    d.Cin, d.T, d.S = cin, T, S
    for name, h in (("halo_prev", halo_prev), ("halo_next", halo_next)):
        if h is not None:
            if h.shape != (x.shape[0] // T, S, cin):
                raise ValueError(f"{name}: expected contiguous (clips, S, C) = {(x.shape[0] // T, S, cin)}, got {tuple(h.shape)}")
            _dense(h, name, BF16, pw.wt.get_device(), 16, h.numel())
            setattr(d, name, _p(h))
    _fill_epilogue(d, pw, out, M, rowvec, S, res1, res2, alpha, beta)
    _ask_gn(d, gn, S, x.device)
    _gemm(d)
    return out.view(x.shape[0], S, pw.N)


def pack_conv3d(weight, bias=None, device="cuda", cin_pad=None):
    """nn.Conv3d weight [Cout][Cin][3][3][3] -> [Cout][Cin(_pad)/64][kt][ky][kx][64] (temporal VAE decoder)."""
    w = weight.detach().float().permute(0, 2, 3, 4, 1).contiguous()  # Cout, kt, ky, kx, Cin
    cout, _, _, _, cin = w.shape
    cp = cin_pad or ceil_to(cin, 64)
    if cp != cin:
        w = torch.nn.functional.pad(w, (0, cp - cin))
    return _finish_pack(_slab_major(w.reshape(cout, 27, cp)), None if bias is None else bias.detach().float(), device)


def conv3d(x, pw, T, H, W, *, out=None, out_f32=False, res1=None, res2=None, alpha=1.0, beta=0.0):
    """3x3x3 conv, pad 1, over x ((b t), H*W, Cin) with clips of T frames (AE3DConv.time_mix_conv and the decoder's time_stack)."""
    cin = x.shape[-1]
    if T <= 0 or x.shape[0] % T:
        raise ValueError(f"conv3d: x has {x.shape[0]} frames, not a multiple of T = {T}")
    _dense(x, "x", BF16, pw.wt.get_device(), 16, x.shape[0] * H * W * cin)
    if pw.K != 27 * cin:
        raise ValueError(f"conv3d: weight K {pw.K} != 27*{cin}")
    M = x.shape[0] * H * W
    if out is None:
        out = torch.empty((M, pw.N), dtype=F32 if out_f32 else BF16, device=x.device)
    d = VkGemmDesc()
    d.A, d.lda = _p(x), cin
    d.amode, d.epi = AMODE_CONV3D, EPI_LINEAR
    d.H, d.Wd, d.Cin, d.T = H, W, cin, T
    _fill_epilogue(d, pw, out, M, None, 0, res1, res2, alpha, beta)
    _gemm(d)
    return out.view(x.shape[0], H * W, -1) if out.dim() == 2 and out.is_contiguous() else out


# ---------------------------------------------------------------------------------------------- fp8 GEMM (BASELINE config 5)
FP8_MAX = 448.0  # OCP e4m3fn


class PackedWeightF8:
    """fp8 e4m3 [ceil-tile(N)][Kp] weight (Kp = ceil128(K), zero-filled) + f32 per-output-channel scale + f32 bias."""

    __slots__ = ("wt", "scale", "bias", "N", "K", "Kp", "geglu")

    def __init__(self, wt, scale, bias, N, K, Kp, geglu=False):
        self.wt, self.scale, self.bias, self.N, self.K, self.Kp, self.geglu = wt, scale, bias, N, K, Kp, geglu


def _finish_pack_fp8(w2d, bias, device, geglu=False):
    N, K = w2d.shape
    if K % 16:
        raise ValueError("fp8 GEMM needs K % 16 == 0")
    Kp = ceil_to(K, 128)
    Np = max(ceil_to(N, 256), ceil_to(N, 320))
    amax = w2d.abs().amax(dim=1).clamp_min(1e-12)
    sc = (amax / FP8_MAX).float()
    q = (w2d / sc[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    wt = torch.zeros((Np, Kp), dtype=torch.uint8, device=device)
    wt[:N, :K] = q.view(torch.uint8).to(device)
    scale = torch.ones((Np,), dtype=F32, device=device)
    scale[:N] = sc.to(device)
    b = None
    if bias is not None:
        b = torch.zeros((Np,), dtype=F32, device=device)
        b[:N] = bias.to(device=device, dtype=F32)
    return PackedWeightF8(wt, scale, b, ceil_to(N, 4), K, Kp, geglu)


def pack_linear_fp8(weight, bias=None, device="cuda"):
    """nn.Linear weight [N][K] -> per-output-channel-scaled fp8 (host-side, once per weight load)."""
    return _finish_pack_fp8(weight.detach().reshape(weight.shape[0], -1).float().cpu(), None if bias is None else bias.detach().float().cpu(), device)


def pack_conv3x3_fp8(weight, bias=None, device="cuda"):
    """nn.Conv2d weight [Cout][Cin][3][3] (Cin % 64 == 0) -> e4m3 [Cout][Cin/64][ky][kx][64], one scale per output channel."""
    w = weight.detach().float().cpu().permute(0, 2, 3, 1).contiguous()
    cout, _, _, cin = w.shape
    if cin % 64:
        raise ValueError("fp8 conv3x3 needs Cin % 64 == 0")
    return _finish_pack_fp8(_slab_major(w.reshape(cout, 9, cin)), None if bias is None else bias.detach().float().cpu(), device)


def pack_conv_t3_fp8(weight, bias=None, device="cuda"):
    """nn.Conv3d weight [Cout][Cin][3][1][1] (Cin % 64 == 0) -> e4m3 [Cout][Cin/64][kt][64], one scale per output channel."""
    w = weight.detach().float().cpu()[:, :, :, 0, 0].permute(0, 2, 1).contiguous()
    if w.shape[2] % 64:
        raise ValueError("fp8 temporal conv needs Cin % 64 == 0")
    return _finish_pack_fp8(_slab_major(w), None if bias is None else bias.detach().float().cpu(), device)


def pack_geglu_fp8(weight, bias, device="cuda"):
    """GEGLU.proj in the value/gate-interleaved row order of pack_geglu, quantised per packed row."""
    w = weight.detach().float().cpu()
    b = bias.detach().float().cpu()
    perm = geglu_perm(w.shape[0] // 2)
    return _finish_pack_fp8(w[perm], b[perm], device, geglu=True)


def quantize_rows_fp8(x):
    """x (..., K) bf16 (rows may be strided) -> (q uint8 (M, K) holding e4m3 bytes, scale f32 (M,)) with x ~= q * scale[:, None]."""
    _need(x, BF16, "x")
    x2, ldx = _rows2d(x, "x")
    M, K = x2.shape
    q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    scale = torch.empty((M,), dtype=F32, device=x.device)
    check(_lib.load().vk_quantize_rows_fp8(_p(x2), _p(q), _p(scale), M, K, ldx, K, _stream()), "vk_quantize_rows_fp8")
    return q, scale


def groupnorm_fp8(x, gamma, beta, eps, silu, frames_per_group=1, x2=None):
    """GroupNorm(32)[+SiLU] with e4m3 output and one scale per image group: x (n_img, S, C) bf16 [x2: second tensor of a channel concat]
    -> (y8 uint8 (n_img, S, C[+C2]), scale f32 (n_img / frames_per_group,)), GN(x) ~= y8 * scale[image group]. The scale is an upper bound
    from the statistics pass (include/vista_hip.h: vk_groupnorm_silu_fp8), not a measured maximum."""
    _need(x, BF16, "x")
    if not x.is_contiguous() or (x2 is not None and (not x2.is_contiguous() or x2.shape[:2] != x.shape[:2])):
        raise ValueError("groupnorm_fp8: contiguous (n_img, S, C) inputs with equal n_img, S required")
    n_img, S, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[2]
    ng = n_img // frames_per_group
    y = torch.empty((n_img, S, c1 + c2), dtype=torch.uint8, device=x.device)
    scale = torch.empty((ng,), dtype=F32, device=x.device)
    ws = torch.empty(ng * 64 + n_img * ((S + 31) // 32) * 65, dtype=F32, device=x.device)
    check(_lib.load().vk_groupnorm_silu_fp8(_p(x), _p(x2), _p(y), _p(scale), _p(gamma), _p(beta), _p(ws), n_img, S, c1, c2, frames_per_group,
                                            float(eps), 1 if silu else 0, _stream()), "vk_groupnorm_silu_fp8")
    return y, scale


def _conv_fp8(d, x8, scale, rows_per_scale, pw, M, rowvec, rows_per_vec, res1, res2, alpha, beta):
    out = torch.empty((M, pw.N), dtype=BF16, device=x8.device)
    _fill_epilogue(d, pw, out, M, rowvec, rows_per_vec, res1, res2, alpha, beta)
    d.K = pw.Kp
    d.tile_cfg = 0
    a = VkFp8Args()
    a.a_scale, a.w_scale, a.k_real, a.a_scale_rows = _p(scale), _p(pw.scale), pw.K, rows_per_scale
    check(_lib.load().vk_gemm_fp8_mx(C.byref(d), C.byref(a), _stream()), "vk_gemm_fp8_mx")
    return out


def conv3x3_fp8(x8, scale, pw, n_img, H, W, *, frames_per_scale=1, rowvec=None, res1=None, res2=None, alpha=1.0, beta=0.0):
    """3x3 conv, stride 1, pad 1, over the e4m3 output of groupnorm_fp8 (x8 (n_img, H*W, Cin) uint8, scale one per `frames_per_scale`
    images) with fp8 weights (pack_conv3x3_fp8) -> (n_img, H*W, Cout) bf16; epilogue options as conv3x3."""
    if x8.dtype != torch.uint8 or not x8.is_contiguous() or x8.shape[:2] != (n_img, H * W):
        raise TypeError("conv3x3_fp8: x8 must be a contiguous (n_img, H*W, Cin) uint8 tensor")
    cin = x8.shape[-1]
    if pw.K != 9 * cin:
        raise ValueError(f"conv3x3_fp8: weight K {pw.K} != 9*{cin}")
    M = n_img * H * W
    d = VkGemmDesc()
    d.A, d.lda = _p(x8), cin
    d.amode, d.epi = AMODE_CONV3X3, EPI_LINEAR
    d.H, d.Wd, d.Cin, d.Hout, d.Wout, d.stride, d.ups = H, W, cin, H, W, 1, 1
    return _conv_fp8(d, x8, scale, frames_per_scale * H * W, pw, M, rowvec, H * W, res1, res2, alpha, beta).view(n_img, H * W, pw.N)


def conv_t3_fp8(x8, scale, pw, T, S, *, rowvec=None, res1=None, res2=None, alpha=1.0, beta=0.0):
    """3x1x1 temporal conv, pad (1,0,0), over the e4m3 output of groupnorm_fp8(frames_per_group=T): x8 ((b t), S, Cin) uint8, scale (b,)."""
    if x8.dtype != torch.uint8 or not x8.is_contiguous() or x8.shape[1] != S or x8.shape[0] % T:
        raise TypeError("conv_t3_fp8: x8 must be a contiguous ((b t), S, Cin) uint8 tensor")
    cin = x8.shape[-1]
    if pw.K != 3 * cin:
        raise ValueError("conv_t3_fp8: weight K mismatch")
    M = x8.shape[0] * S
    d = VkGemmDesc()
    d.A, d.lda = _p(x8), cin
    d.amode, d.epi = AMODE_TEMPORAL3, EPI_LINEAR
    d.Cin, d.T, d.S = cin, T, S
    return _conv_fp8(d, x8, scale, T * S, pw, M, rowvec, S, res1, res2, alpha, beta).view(x8.shape[0], S, pw.N)


def layernorm_quant_fp8(x, norm):
    """LayerNorm fused with per-row e4m3 quantisation (one pass): x (..., C) bf16 -> (q uint8 (M, C), scale f32 (M,)) with LN(x) ~= q * scale[:, None]."""
    _need(x, BF16, "x")
    if not x.is_contiguous():
        raise ValueError("layernorm_quant_fp8: x must be contiguous")
    Cc = x.shape[-1]
    M = x.numel() // Cc
    q = torch.empty((M, Cc), dtype=torch.uint8, device=x.device)
    scale = torch.empty((M,), dtype=F32, device=x.device)
    check(_lib.load().vk_layernorm_quant_fp8(_p(x), _p(q), _p(scale), _p(norm.weight), _p(norm.bias), M, Cc, float(norm.eps), _stream()),
          "vk_layernorm_quant_fp8")
    return q, scale


def linear_fp8(xq, a_scale, pw, *, out=None, out_f32=False, rowvec=None, rows_per_vec=0, res1=None, res2=None, alpha=1.0, beta=0.0,
               rowvec2=None, a_mx=None, mx_out=False, emit_stats=False):
    """out = alpha*((xq*scales) @ (Wq*w_scale)^T + bias + rowvec + res1) + beta*(res2 + rowvec2), fp8 x fp8 -> f32 accumulate.
    Activation scales: `a_scale` f32 (M,) per row, OR `a_mx` uint8 (M, K/32) E8M0 block scales (MX; a_scale None).
    mx_out (GEGLU weights only): return (h8 uint8 (M, nout), hs uint8 (M, nout/32)) -- the gated output quantised to MX fp8 in the epilogue.
    emit_stats: also return the RowStats of the (bf16) output."""
    if xq.dtype != torch.uint8 or xq.dim() != 2 or xq.stride(1) != 1:
        raise TypeError("linear_fp8: xq must be a (M, K) uint8 tensor of e4m3 bytes")
    M, K = xq.shape
    if K != pw.K:
        raise ValueError(f"linear_fp8: K mismatch {K} vs {pw.K}")
    if (a_scale is None) == (a_mx is None):
        raise ValueError("linear_fp8: exactly one of a_scale (per row) / a_mx (MX block scales)")
    nout = pw.N // 2 if pw.geglu else pw.N
    hs = None
    if mx_out:
        if not pw.geglu or nout % 32:
            raise ValueError("mx_out: GEGLU weights with an output width that is a multiple of 32")
        out = torch.empty((M, nout), dtype=torch.uint8, device=xq.device)
        hs = torch.empty((M, nout // 32), dtype=torch.uint8, device=xq.device)
    elif out is None:
        out = torch.empty((M, nout), dtype=F32 if (out_f32 and not pw.geglu) else BF16, device=xq.device)
    d = VkGemmDesc()
    d.A, d.lda = _p(xq), xq.stride(0)
    d.amode = AMODE_DENSE
    d.epi = EPI_GEGLU if pw.geglu else EPI_LINEAR
    _fill_epilogue(d, pw, out, M, rowvec, rows_per_vec, res1, res2, alpha, beta, rowvec2, ncols=nout, out_dtype=torch.uint8 if out.dtype is torch.uint8 else None)
    d.K = pw.Kp
    d.tile_cfg = TILE_CFG & 7
    lib = _lib.load()
    stats = None
    if emit_stats:
        parts = lib.vk_gemm_fp8_rowstat_parts(C.byref(d))
        if parts <= 0:
            raise _lib.VistaHipError(f"vk_gemm_fp8_rowstat_parts failed with code {parts}")
        stats = RowStats(torch.empty((parts, M, 2), dtype=F32, device=xq.device), parts, M)
        d.rowstat_out = _p(stats.t)
    a = VkFp8Args()
    a.a_scale, a.w_scale, a.k_real = _p(a_scale), _p(pw.scale), K
    if a_mx is not None:
        if a_mx.dtype != torch.uint8 or a_mx.dim() != 2 or a_mx.shape[0] != M or a_mx.shape[1] < K // 32 or a_mx.stride(1) != 1 or a_mx.stride(0) % 4:
            raise ValueError("a_mx: uint8 (M, >= K/32) E8M0 block scales, row stride a multiple of 4 (the kernel reads one dword per 128 K-bytes)")
        a.a_mx, a.ld_mx = _p(a_mx), a_mx.stride(0)
    if mx_out:
        a.mx_out, a.ld_mx_out = _p(hs), hs.stride(0)
    check(lib.vk_gemm_fp8_mx(C.byref(d), C.byref(a), _stream()), "vk_gemm_fp8_mx")
    if mx_out:
        return out, hs
    return (out, stats) if emit_stats else out


# ---------------------------------------------------------------------------------------------- attention
PROFILE_ATTN = None  # bench.py sets this to a list: (S, n_img*heads, start_event, end_event) per launch, on the launch stream


LOG2E = 1.4426950408889634


def attn_spatial(q, k, vt, n_img, heads, S, scale=None, v_rows=False, q_log2=False):
    """q, k: 2-D strided views (n_img*S, heads*64) bf16. vt: (n_img, heads*64, S) = V transposed (linear_vt), or with v_rows=True a
    2-D strided view (n_img*S, heads*64) like q and k -- the v column block of ONE fused q|k|v GEMM. Returns (n_img*S, heads*64).
    q_log2 (with v_rows): q already carries softmax_scale * log2(e) (folded into the query weights at pack time), so q.k is the base-2
    exponent itself and the kernel's zero-base path needs no scale / base fma (vk_attn_spatial_qkv_log2_bf16); `scale` is not used."""
    M, c = n_img * S, heads * 64
    _operand(q, "q", BF16, q.get_device(), 16, M, c, 8, exact_cols=True)
    _operand(k, "k", BF16, q.get_device(), 16, M, c, 8, exact_cols=True)
    if v_rows:
        _operand(vt, "v", BF16, q.get_device(), 16, M, c, 8, exact_cols=True)
    else:
        if vt.shape != (n_img, c, S):
            _refuse("vt", vt, f"must be (n_img, heads*64, S) = {(n_img, c, S)}")
        _dense(vt, "vt", BF16, q.get_device(), 16, M * c)
    if S % 8:
        raise ValueError(f"attn_spatial: S = {S} must be a multiple of 8")
    o = torch.empty((M, c), dtype=BF16, device=q.device)
    lib = _lib.load()
    ev = None
    if PROFILE_ATTN is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    sc = float(scale if scale is not None else 1.0 / math.sqrt(64))
    if v_rows:
        if q_log2:
            check(lib.vk_attn_spatial_qkv_log2_bf16(_p(q), _p(k), _p(vt), _p(o), n_img, heads, S, q.stride(0), k.stride(0), vt.stride(0), o.stride(0),
                                                    _stream()), "vk_attn_spatial_qkv_log2_bf16")
        else:
            check(lib.vk_attn_spatial_qkv_bf16(_p(q), _p(k), _p(vt), _p(o), n_img, heads, S, q.stride(0), k.stride(0), vt.stride(0), o.stride(0), sc,
                                               _stream()), "vk_attn_spatial_qkv_bf16")
    else:
        if ACT is not torch.bfloat16:
            raise _lib.VistaHipError("attn_spatial with a V^T tensor: bf16 build only (in the fp16 build V must come from a q|k|v projection launched "
                                     "with alt_cols_from, i.e. as bf16 rows)")
        check(lib.vk_attn_spatial_bf16(_p(q), _p(k), _p(vt), _p(o), n_img, heads, S, q.stride(0), k.stride(0), o.stride(0), sc, _stream()),
              "vk_attn_spatial_bf16")
    if ev is not None:
        ev[1].record()
        PROFILE_ATTN.append((S, n_img * heads, ev[0], ev[1]))
    return o


def attn_spatial_fp8qk(q8, k8, qs, ks, v, n_img, heads, S, scale=None, mx_out=False):
    """BASELINE config 5: spatial self-attention with the score product in fp8. q8 / k8: (n_img*S, heads*64) uint8 views of e4m3 bytes (rows
    may be strided: the q | k blocks of linear(..., mx8_cols=2C)); qs / ks: (n_img*S, 2*heads) uint8 views of their E8M0 block scales; v:
    (n_img*S, heads*64) bf16 rows. Returns bf16 (n_img*S, heads*64), or with mx_out=True (o8 uint8 (M, C), o_scales uint8 (M, C/32)).
    scale=0.0: q already carries softmax_scale * log2(e) (the pre-scaled query of attn_spatial(..., q_log2=True))."""
    _need(v, BF16, "v")
    for name, t in (("q8", q8), ("k8", k8), ("qs", qs), ("ks", ks)):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda:
            raise TypeError(f"attn_spatial_fp8qk: {name} must be a 2-D uint8 device view with contiguous rows")
    M, c = n_img * S, heads * 64
    if q8.shape != (M, c) or k8.shape != (M, c) or qs.shape != (M, 2 * heads) or ks.shape != (M, 2 * heads) or v.shape != (M, c) or v.stride(1) != 1:
        raise ValueError("attn_spatial_fp8qk: shape mismatch")
    o = o8 = osc = None
    if mx_out:
        o8 = torch.empty((M, c), dtype=torch.uint8, device=v.device)
        osc = torch.empty((M, ceil_to(2 * heads, 4)), dtype=torch.uint8, device=v.device)  # row stride % 4 for the consumer GEMM; the kernel sets the pad bytes to 2^0
    else:
        o = torch.empty((M, c), dtype=BF16, device=v.device)
    ev = None
    if PROFILE_ATTN is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    check(_lib.load().vk_attn_spatial_fp8qk(_p(q8), _p(k8), _p(qs), _p(ks), _p(v), _p(o), _p(o8), _p(osc), n_img, heads, S, q8.stride(0), k8.stride(0),
                                            qs.stride(0), ks.stride(0), v.stride(0), c, c, ceil_to(2 * heads, 4),
                                            float(scale if scale is not None else 1.0 / math.sqrt(64)), _stream()), "vk_attn_spatial_fp8qk")
    if ev is not None:
        ev[1].record()
        PROFILE_ATTN.append((S, n_img * heads, ev[0], ev[1]))
    return (o8, osc) if mx_out else o


def attn_small(qkv, n_img, heads, S, D, scale=None):
    """qkv: (n_img*S, 3*heads*D) bf16 row-major [q | k | v]; softmax(q k^T * scale) v per (image, head), D in {64, 80, 128}
    (the OpenCLIP image tower's nn.MultiheadAttention). Returns (n_img*S, heads*D)."""
    c = heads * D
    _operand(qkv, "qkv", BF16, qkv.get_device(), 16, n_img * S, 3 * c, 8, exact_cols=True)
    if qkv.shape[0] != n_img * S:
        _refuse("qkv", qkv, f"must be (n_img*S, 3*heads*D) = {(n_img * S, 3 * c)}")
    o = torch.empty((n_img * S, c), dtype=BF16, device=qkv.device)
    check(_lib.load().vk_attn_small_bf16(_p(qkv), _p(o), n_img, heads, S, D, qkv.stride(0), c, 2 * c, o.stride(0),
                                         float(scale if scale is not None else 1.0 / math.sqrt(D)), _stream()), "vk_attn_small_bf16")
    return o


def antialias_blur_params(in_size, out_size):
    """(sigma, kernel size) of kornia-0.6.9 `resize(..., antialias=True)` along one axis (kornia/geometry/transform/affwarp.py: the
    blur only exists when downscaling; sigma = max((factor - 1) / 2, 0.001), ks = int(max(4 sigma, 3)) made odd). No blur: (1.0, 1)."""
    factor = in_size / out_size
    sigma = max((factor - 1.0) / 2.0, 0.001)
    ks = int(max(2.0 * 2 * sigma, 3))
    if ks % 2 == 0:
        ks += 1
    return sigma, ks


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess_patches(img, out_hw=224, patch=14, kpad=None, antialias=True, mean=CLIP_MEAN, std=CLIP_STD):
    """img (n, 3, H, W) f32 in [-1, 1] -> (n * (1 + g*g), Kp) bf16, g = out_hw / patch: row 0 of every image zero (class-token slot), row
    1 + py*g + px = patch (py, px) of the resized / normalised image flattened [c][ky][kx], zero-padded to Kp = ceil64(3*patch^2).
    FrozenOpenCLIPImageEmbedder.preprocess (modules.py:304-315) fused with the patch convolution's im2col."""
    _need(img, F32, "img")
    img = img.contiguous()
    n, c, H, W = img.shape
    if c != 3:
        raise ValueError("clip_preprocess_patches: 3-channel images")
    g = out_hw // patch
    kp = kpad or ceil_to(3 * patch * patch, 64)
    out = torch.zeros((n * (1 + g * g), kp), dtype=BF16, device=img.device)
    down = antialias and max(H / out_hw, W / out_hw) > 1  # kornia blurs BOTH axes as soon as either one is downscaled
    (sy, ky), (sx, kx) = (antialias_blur_params(H, out_hw), antialias_blur_params(W, out_hw)) if down else ((1.0, 1), (1.0, 1))
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(_lib.load().vk_clip_preprocess_patches(_p(img), _p(out), n, H, W, out_hw, patch, kp, sy, sx, ky, kx, m3, s3, _stream()),
          "vk_clip_preprocess_patches")
    return out


def attn_temporal(qkv, B, T, S, heads, scale=None):
    """qkv: ((b t) s, 3*heads*64) bf16 row-major [q | k | v]. Returns ((b t) s, heads*64)."""
    c = heads * 64
    _operand(qkv, "qkv", BF16, qkv.get_device(), 16, B * T * S, 3 * c, 8, exact_cols=True)
    if qkv.shape[0] != B * T * S:
        _refuse("qkv", qkv, f"must be ((b t) s, 3*heads*64) = {(B * T * S, 3 * c)}")
    o = torch.empty((B * T * S, c), dtype=BF16, device=qkv.device)
    lib = _lib.load()
    check(lib.vk_attn_temporal_bf16(_p(qkv), _p(o), B, T, S, heads, qkv.stride(0), c, 2 * c, o.stride(0),
                                    float(scale if scale is not None else 1.0 / math.sqrt(64)), _stream()), "vk_attn_temporal_bf16")
    return o


# ---------------------------------------------------------------------------------------------- norms
def softmax_rows(x, out=None):
    """x (rows, cols) fp32 (row stride may exceed cols) -> bf16 softmax over the last dim (VAE decoder AttnBlock)."""
    if x.dim() != 2:
        _refuse("x", x, "must be 2-D")
    rows, cols = x.shape
    _operand(x, "x", F32, x.get_device(), 16, rows, cols, 4)
    if out is None:
        out = torch.empty((rows, cols), dtype=BF16, device=x.device)
    else:
        _operand(out, "out", BF16, x.get_device(), 8, rows, cols, 4, exact_cols=True)
    check(_lib.load().vk_softmax_rows_f32_bf16(_p(x), _p(out), rows, cols, x.stride(0), out.stride(0), _stream()), "vk_softmax_rows_f32_bf16")
    return out


def _gn_partials_ok(gn, n_img, S, Cc):
    """The producer's partials describe exactly this tensor (and have not been consumed yet)."""
    if gn is None or gn.t is None:
        return False
    if gn.rows != n_img * S or gn.C != Cc or gn.nchunks * 64 != S:
        raise ValueError(f"GnPartials of a ({gn.rows} rows, {gn.C} channels, {gn.nchunks * 64} rows per image) tensor passed to a GroupNorm over ({n_img}, {S}, {Cc})")
    return True


def groupnorm(x, gamma, beta, eps, silu, frames_per_group=1, out=None, gn=None):
    """x (n_img, S, C) bf16 contiguous. gn: the GnPartials the producer of x filled (conv3x3 / conv_t3 (..., gn=...)): fold + apply, no
    statistics pass over x."""
    if x.dim() != 3:
        _refuse("x", x, "must be (n_img, S, C)")
    n_img, S, Cc = x.shape
    _dense(x, "x", BF16, x.get_device(), 16, n_img * S * Cc)
    _affine(gamma, beta, Cc, x.get_device())
    if out is None:
        out = torch.empty_like(x)
    else:
        _dense(out, "out", BF16, x.get_device(), 16, n_img * S * Cc)
    if _gn_partials_ok(gn, n_img, S, Cc):
        lib = _lib.load()
        count = float(Cc // 32) * float(S) * float(frames_per_group)
        if frames_per_group * gn.nchunks <= lib.vk_groupnorm_fold_max():   # ABI v7: the apply workgroups fold the slots themselves (no finalize launch)
            check(lib.vk_groupnorm_apply_partials_bf16(_p(x), _p(out), _p(gamma), _p(beta), _p(gn.t), n_img, S, Cc, gn.nchunks, frames_per_group, count,
                                                       float(eps), 1 if silu else 0, _stream()), "vk_groupnorm_apply_partials_bf16")
            gn.t = None   # consumed
            return out
        sums = torch.empty((n_img // frames_per_group) * 64, dtype=F32, device=x.device)
        check(lib.vk_groupnorm_finalize_partials(_p(gn.t), _p(sums), n_img, gn.nchunks, frames_per_group, _stream()), "vk_groupnorm_finalize_partials")
        gn.t = None   # consumed
        check(lib.vk_groupnorm_apply_bf16(_p(x), _p(out), _p(gamma), _p(beta), _p(sums), n_img, S, Cc, frames_per_group, count, float(eps),
                                          1 if silu else 0, _stream()), "vk_groupnorm_apply_bf16")
        return out
    ws = torch.empty(((n_img // frames_per_group) + n_img * ((S + 31) // 32)) * 64, dtype=F32, device=x.device)
    lib = _lib.load()
    check(lib.vk_groupnorm_silu_bf16(_p(x), _p(out), _p(gamma), _p(beta), _p(ws), n_img, S, Cc, frames_per_group, float(eps),
                                     1 if silu else 0, _stream()), "vk_groupnorm_silu_bf16")
    return out


def groupnorm_cat(a, b, gamma, beta, eps, silu, frames_per_group=1):
    """GroupNorm(32)[+SiLU] of the channel concat [a | b] ((n_img, S, C1) and (n_img, S, C2) bf16) -> (n_img, S, C1+C2), without
    materialising the concat (the skip `torch.cat` of the UNet's output blocks, video_model.py:493)."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[:2] != b.shape[:2]:
        raise ValueError("groupnorm_cat: contiguous (n_img, S, C) inputs with equal n_img, S required")
    n_img, S, c1 = a.shape
    c2 = b.shape[2]
    _dense(a, "a", BF16, a.get_device(), 16, n_img * S * c1)
    _dense(b, "b", BF16, a.get_device(), 16, n_img * S * c2)
    _affine(gamma, beta, c1 + c2, a.get_device())
    out = torch.empty((n_img, S, c1 + c2), dtype=BF16, device=a.device)
    ws = torch.empty(((n_img // frames_per_group) + n_img * ((S + 31) // 32)) * 64, dtype=F32, device=a.device)
    check(_lib.load().vk_groupnorm_silu_cat_bf16(_p(a), _p(b), _p(out), _p(gamma), _p(beta), _p(ws), n_img, S, c1, c2, frames_per_group,
                                                 float(eps), 1 if silu else 0, _stream()), "vk_groupnorm_silu_cat_bf16")
    return out


def groupnorm_sharded(x, gamma, beta, eps, silu, frames_per_group, allreduce, global_count, gn=None):
    """GroupNorm whose statistics also span other ranks' shards of the same images (pixel-sharded temporal ResBlock):
    local fixed-order sums -> `allreduce(sums)` (in place, SUM over ranks) -> apply with the GLOBAL element count.
    gn: the producer's GnPartials of x (as groupnorm)."""
    if x.dim() != 3:
        _refuse("x", x, "must be (n_img, S, C)")
    n_img, S, Cc = x.shape
    _dense(x, "x", BF16, x.get_device(), 16, n_img * S * Cc)
    _affine(gamma, beta, Cc, x.get_device())
    out = torch.empty_like(x)
    ng = n_img // frames_per_group
    sums = torch.empty(ng * 64, dtype=F32, device=x.device)
    lib = _lib.load()
    if _gn_partials_ok(gn, n_img, S, Cc):
        check(lib.vk_groupnorm_finalize_partials(_p(gn.t), _p(sums), n_img, gn.nchunks, frames_per_group, _stream()), "vk_groupnorm_finalize_partials")
        gn.t = None
    else:
        part = torch.empty(n_img * ((S + 31) // 32) * 64, dtype=F32, device=x.device)
        check(lib.vk_groupnorm_stats_bf16(_p(x), _p(sums), _p(part), n_img, S, Cc, frames_per_group, _stream()), "vk_groupnorm_stats_bf16")
    allreduce(sums)
    check(lib.vk_groupnorm_apply_bf16(_p(x), _p(out), _p(gamma), _p(beta), _p(sums), n_img, S, Cc, frames_per_group, float(global_count),
                                      float(eps), 1 if silu else 0, _stream()), "vk_groupnorm_apply_bf16")
    return out


def layernorm(x, gamma, beta, eps=1e-5, addvec=None, rows_per_vec=0, want_sum=False):
    """x (..., C) bf16 contiguous -> LN(x + addvec[row // rows_per_vec]); optionally also returns the sum."""
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    _dense(x, "x", BF16, x.get_device(), 16, rows * Cc)
    _affine(gamma, beta, Cc, x.get_device())
    if addvec is not None:
        if int(rows_per_vec) <= 0:
            raise ValueError("layernorm: addvec needs rows_per_vec > 0")
        _operand(addvec, "addvec", F32, x.get_device(), 4, (rows + int(rows_per_vec) - 1) // int(rows_per_vec), Cc)
    y = torch.empty_like(x)
    s = torch.empty_like(x) if (want_sum and addvec is not None) else None
    lib = _lib.load()
    check(lib.vk_layernorm_bf16(_p(x), _p(y), _p(s), _p(gamma), _p(beta), _p(addvec), rows, Cc, int(rows_per_vec),
                                addvec.stride(0) if addvec is not None else 0, float(eps), _stream()), "vk_layernorm_bf16")
    return (y, s) if want_sum else y


# ---------------------------------------------------------------------------------------------- elementwise
def concat_channels(a, b):
    c1, c2 = a.shape[-1], b.shape[-1]
    rows = a.numel() // c1
    if a.shape[:-1] != b.shape[:-1]:
        raise ValueError("concat_channels: a and b must agree in every dim but the last")
    _dense(a, "a", BF16, a.get_device(), 16, rows * c1)
    _dense(b, "b", BF16, a.get_device(), 16, rows * c2)
    out = torch.empty(a.shape[:-1] + (c1 + c2,), dtype=BF16, device=a.device)
    check(_lib.load().vk_concat_channels_bf16(_p(a), _p(b), _p(out), rows, c1, c2, _stream()), "vk_concat_channels_bf16")
    return out


def nchw_to_tokens(x, cpad):
    n, c, h, w = x.shape
    x = x.contiguous()
    _dense(x, "x", F32, x.get_device(), 4, n * c * h * w)
    out = torch.empty((n, h * w, cpad), dtype=BF16, device=x.device)
    check(_lib.load().vk_nchw_to_tokens_bf16(_p(x), _p(out), n, c, h * w, cpad, _stream()), "vk_nchw_to_tokens_bf16")
    return out


def tokens_to_nchw(x, n_img, Cc, H, W):
    _token_rows(x, "x", F32, x.get_device(), 4, n_img * H * W, Cc)
    out = torch.empty((n_img, Cc, H, W), dtype=F32, device=x.device)
    check(_lib.load().vk_tokens_to_nchw_f32(_p(x), _p(out), n_img, Cc, H * W, x.stride(-2), _stream()), "vk_tokens_to_nchw_f32")
    return out


def timestep_embedding(t, dim, max_period=10000.0, out_f32=False):
    t = t.contiguous()
    _dense(t, "t", F32, t.get_device(), 4, t.shape[0])
    out = torch.empty((t.shape[0], dim), dtype=F32 if out_f32 else BF16, device=t.device)
    lib = _lib.load()
    fn = lib.vk_timestep_embedding_f32 if out_f32 else lib.vk_timestep_embedding_bf16
    check(fn(_p(t), _p(out), t.shape[0], dim, float(max_period), _stream()), "vk_timestep_embedding")
    return out


def emb_combine(a, b, c, mask):
    """emb = a*mask + b*(1-mask) + c ; returns (emb f32, silu(emb) bf16)."""
    n, dim = b.shape
    for name, t in (("a", a), ("b", b), ("c", c)):
        if t is not None:
            _dense(t, name, F32, b.get_device(), 4, n * dim)
    if mask is not None:
        _dense(mask, "mask", F32, b.get_device(), 4, n)
    emb = torch.empty((n, dim), dtype=F32, device=b.device)
    se = torch.empty((n, dim), dtype=BF16, device=b.device)
    check(_lib.load().vk_emb_combine(_p(a), _p(b), _p(c), _p(mask), _p(emb), _p(se), n, dim, _stream()), "vk_emb_combine")
    return emb, se


def silu_to_bf16(x):
    _need(x, F32, "x")
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(_lib.load().vk_silu_f32_to_bf16(_p(x), _p(y), x.numel(), _stream()), "vk_silu_f32_to_bf16")
    return y


def cast_to_bf16(x):
    _need(x, F32, "x")
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(_lib.load().vk_cast_f32_to_bf16(_p(x), _p(y), x.numel(), _stream()), "vk_cast_f32_to_bf16")
    return y


# ---- sampler-side ----
def sampler_prepare(x, cond_frame, mask, concat_uc, concat_c, cpad, c_in, replace):
    T, ch, H, W = x.shape
    if ch != 4:
        _refuse("x", x, "must be (T, 4, H, W)")
    for name, t in (("x", x), ("cond_frame", cond_frame), ("concat_uc", concat_uc), ("concat_c", concat_c)):
        if t is not None:
            _dense(t, name, F32, x.get_device(), 4, T * 4 * H * W)
    if mask is not None:
        _dense(mask, "mask", F32, x.get_device(), 4, T)
    net_in = torch.empty((2 * T, H * W, cpad), dtype=BF16, device=x.device)
    check(_lib.load().vk_sampler_prepare(_p(x), _p(cond_frame), _p(mask), _p(concat_uc), _p(concat_c), _p(net_in), T, H * W, cpad,
                                         float(c_in), 1 if replace else 0, _stream()), "vk_sampler_prepare")
    return net_in


def sampler_update(x, net_out, scale, c_out, c_skip, sigma, sigma_next):
    T, ch, H, W = x.shape
    if ch != 4:
        _refuse("x", x, "must be (T, 4, H, W)")
    _dense(x, "x", F32, x.get_device(), 4, T * 4 * H * W)
    _token_rows(net_out, "net_out", F32, x.get_device(), 4, 2 * T * H * W, 4)
    _dense(scale, "scale", F32, x.get_device(), 4, T)
    check(_lib.load().vk_sampler_update(_p(x), _p(net_out), _p(scale), T, H * W, net_out.stride(-2), float(c_out), float(c_skip),
                                        float(sigma), float(sigma_next), _stream()), "vk_sampler_update")
    return x


def sampler_update_2m(x, net_out, scale, hist, c_out, c_skip, a, b, c, first):
    """The fused DPM-Solver++(2M) step (vk_sampler_update_2m): x = fmaf(c, hist, fmaf(b, g, a*x)) and hist = g, both in place. `first`: hist is
    written but not read. (a, b, c): one triple of sampling.dpmpp2m_coefficients."""
    T, ch, H, W = x.shape
    if ch != 4:
        _refuse("x", x, "must be (T, 4, H, W)")
    _dense(x, "x", F32, x.get_device(), 4, T * 4 * H * W)
    _token_rows(net_out, "net_out", F32, x.get_device(), 4, 2 * T * H * W, 4)
    _dense(scale, "scale", F32, x.get_device(), 4, T)
    if tuple(hist.shape) != tuple(x.shape):
        _refuse("hist", hist, f"must have x's shape {tuple(x.shape)}")
    _dense(hist, "hist", F32, x.get_device(), 4, T * 4 * H * W)
    if hist.data_ptr() == x.data_ptr():
        _refuse("hist", hist, "must not be x: the step reads x and writes both")
    check(_lib.load().vk_sampler_update_2m(_p(x), _p(net_out), _p(scale), _p(hist), T, H * W, net_out.stride(-2), float(c_out), float(c_skip),
                                           float(a), float(b), float(c), 1 if first else 0, _stream()), "vk_sampler_update_2m")
    return x


def dpmpp2m_step(x, den, den_old, a, b, c, out=None):
    """out = fmaf(c, den_old, fmaf(b, den, a*x)) (vk_dpmpp2m_step); den_old None: fmaf(b, den, a*x). A new tensor unless out= is given (out may be x)."""
    dev, n = x.get_device(), x.numel()
    _dense(x, "x", F32, dev, 4, n)
    for name, t in (("den", den), ("den_old", den_old)):
        if t is not None:
            if tuple(t.shape) != tuple(x.shape):
                _refuse(name, t, f"must have x's shape {tuple(x.shape)}")
            _dense(t, name, F32, dev, 4, n)
    if out is None:
        out = torch.empty(x.shape, dtype=F32, device=x.device)
    else:
        if tuple(out.shape) != tuple(x.shape):
            _refuse("out", out, f"must have x's shape {tuple(x.shape)}")
        _dense(out, "out", F32, dev, 4, n)
    check(_lib.load().vk_dpmpp2m_step(_p(x), _p(den), _p(den_old), _p(out), float(a), float(b), float(c), n, _stream()), "vk_dpmpp2m_step")
    return out


def _c(*ts):
    return [t.contiguous() for t in ts]


def denoiser_combine(net, x, c_out, c_skip):
    net, x, c_out, c_skip = _c(net, x, c_out, c_skip)
    out = torch.empty_like(x)
    n = x.shape[0]
    check(_lib.load().vk_denoiser_combine(_p(net), _p(x), _p(c_out), _p(c_skip), _p(out), n, x.numel() // n, _stream()),
          "vk_denoiser_combine")
    return out


def cfg_combine(x2, scale):
    x2, scale = _c(x2, scale)
    T = x2.shape[0] // 2
    out = torch.empty((T,) + tuple(x2.shape[1:]), dtype=F32, device=x2.device)
    check(_lib.load().vk_cfg_combine(_p(x2), _p(scale), _p(out), T, out.numel() // T, _stream()), "vk_cfg_combine")
    return out


def euler_step(x, den, sigma, sigma_next):
    x, den, sigma, sigma_next = _c(x, den, sigma, sigma_next)
    out = torch.empty_like(x)
    n = x.shape[0]
    check(_lib.load().vk_euler_step(_p(x), _p(den), _p(sigma), _p(sigma_next), _p(out), n, x.numel() // n, _stream()), "vk_euler_step")
    return out


def mask_replace(x, cond, mask):
    x, cond, mask = _c(x, cond, mask)
    out = torch.empty_like(x)
    n = x.shape[0]
    check(_lib.load().vk_mask_replace(_p(x), _p(cond), _p(mask), _p(out), n, x.numel() // n, _stream()), "vk_mask_replace")
    return out


def gaussian_sample(moments, noise=None, scale=1.0):
    """moments (n, 2C, h, w) f32 -> (n, C, h, w): (mean + exp(0.5*clamp(logvar)) * noise) * scale; noise None = mode."""
    _need(moments, F32, "moments")
    moments = moments.contiguous()
    n, c2, h, w = moments.shape
    if noise is not None:
        _need(noise, F32, "noise")
        noise = noise.contiguous()
        if noise.shape != (n, c2 // 2, h, w):
            raise ValueError("gaussian_sample: noise must be (n, C, h, w)")
    out = torch.empty((n, c2 // 2, h, w), dtype=F32, device=moments.device)
    check(_lib.load().vk_gaussian_sample(_p(moments), _p(noise), _p(out), n, c2 // 2, h * w, float(scale), _stream()), "vk_gaussian_sample")
    return out


def ensemble_variance_sum(x):
    """x (E, ...) f32 -> python float: sum over elements of the unbiased variance across the E ensemble members."""
    _need(x, F32, "x")
    x = x.contiguous()
    E = x.shape[0]
    n = x.numel() // E
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = torch.empty(512, dtype=torch.float64, device=x.device)
    check(_lib.load().vk_ensemble_variance_sum(_p(x), _p(out), _p(ws), E, n, _stream()), "vk_ensemble_variance_sum")
    return float(out.item())


def scale_rows(x, s):
    x, s = _c(x, s)
    out = torch.empty_like(x)
    n = x.shape[0]
    check(_lib.load().vk_scale_rows(_p(x), _p(s), _p(out), n, x.numel() // n, _stream()), "vk_scale_rows")
    return out


# ---- image I/O of the sampling front door (csrc/image_io.hip, ABI v8) ----
_IMAGE_TABLES = {}   # (device, crop_w, crop_h, width, height) -> device copies of the Lanczos tables; "lut": the 256 output values


def _image_tables(device, crop_w, crop_h, width, height):
    from . import image_io
    key = (str(device), crop_w, crop_h, width, height)
    t = _IMAGE_TABLES.get(key)
    if t is None:
        bx, cx, kx = image_io.lanczos_tables(crop_w, width)
        by, cy, ky = image_io.lanczos_tables(crop_h, height)
        up = lambda a: torch.from_numpy(a.copy()).to(device)  # noqa: E731
        if len(_IMAGE_TABLES) >= 16:
            _IMAGE_TABLES.clear()
        t = _IMAGE_TABLES[key] = (up(bx), up(cx), kx, up(by), up(cy), ky, up(image_io.unit_range_table()))
    return t


def load_img_batch(frames_u8, height, width, box=None):
    """`load_img` (sample.py:174-201) for a stack of decoded frames: frames_u8 (n, h, w, 3) uint8 RGB on the GPU -> (n, 3, height, width) fp32 in
    [-1, 1]. The centre crop (image_io.crop_box, or `box` = (left, top, crop_w, crop_h)) is applied through source offsets; the resize is Pillow's
    8-bit LANCZOS, byte for byte (vk_lanczos_resize_u8), and the output values are ToTensor's k/255 followed by x * 2.0 - 1.0, bit for bit."""
    from . import image_io
    _need(frames_u8, torch.uint8, "frames_u8")
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8[None]
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f"load_img_batch: expected (n, h, w, 3) uint8 RGB frames, got {tuple(frames_u8.shape)}")
    frames_u8 = frames_u8.contiguous()
    n, sh, sw, _ = frames_u8.shape
    left, top, cw, ch = image_io.crop_box(sw, sh, height, width) if box is None else box
    dev = frames_u8.device
    if cw <= 0 or ch <= 0:   # (the tables of an empty box do not exist: the entry point is asked all the same, and answers VK_EINVAL)
        bx = cx = by = cy = lut = torch.zeros(4, dtype=torch.int32, device=dev)
        kx = ky = 1
    else:
        bx, cx, kx, by, cy, ky, lut = _image_tables(dev, cw, ch, width, height)
    tmp = torch.empty((n, max(ch, 1), width, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 3, height, width), dtype=F32, device=dev)
    check(_lib.load().vk_lanczos_resize_u8(_p(frames_u8), _p(tmp), _p(out), _p(bx), _p(cx), kx, _p(by), _p(cy), ky, _p(lut), n, sh, sw,
                                           left, top, ch, cw, height, width, _stream()), "vk_lanczos_resize_u8")
    return out


def frames_to_u8(x, real=False, grid=False):
    """The float -> uint8 conversion of `perform_save_locally` (sample_utils.py:96-137) on the GPU: x (n, 3, H, W) fp32 -> (n, H, W, 3) uint8, or
    with grid=True ONE (rows, cols, 3) uint8 canvas laid out like torchvision.utils.make_grid(x, nrow=int(n ** 0.5)) (padding 2, pad value 0;
    image_io.grid_geometry). real=False: uint8(255 * x) for samples in [0, 1]; real=True: uint8(255 * (x + 1) / 2) for inputs in [-1, 1] -- numpy's
    float32 arithmetic and truncating cast, bit for bit. torchvision is not installed where this package is tested: the layout follows make_grid's
    published source (a single image comes back without a border), parity with a live make_grid is not pinned by a test."""
    from . import image_io
    _need(x, F32, "x")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"frames_to_u8: expected (n, 3, H, W) fp32 frames, got {tuple(x.shape)}")
    x = x.contiguous()
    n, _, H, W = x.shape
    if grid:
        xmaps, _, rows, cols, pad = image_io.grid_geometry(n, H, W)
        out = torch.empty((rows, cols, 3) if pad else (H, W, 3), dtype=torch.uint8, device=x.device)
    else:
        xmaps, pad = 1, 0
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=x.device)
    check(_lib.load().vk_frames_to_u8(_p(x), _p(out), n, H, W, xmaps, pad, 1 if real else 0, _stream()), "vk_frames_to_u8")
    return out


# ---- reward estimation front door (csrc/reward.hip) ----
FRAME_STATS_BLOCKS = 16   # VK_FRAME_STATS_BLOCKS of include/vista_hip.h: partial sums per frame in the workspace


def _aligned16(t):
    """A dense tensor whose first element sits on a 16-byte boundary (a dense view into another tensor's storage may not)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def ensemble_frame_stats(x, want_map=True):
    """x (E, T, C, h, w) f32, the stacked members of a reward ensemble -> (frame_sum (T,) float64 tensor, map (T, h, w) float32 or None):
    the unbiased ensemble variance summed over every frame's elements (fixed order, fp64) and averaged over its channels per pixel
    (vk_ensemble_frame_stats; same per-element arithmetic as ensemble_variance_sum). Nothing is synchronised: both results stay on the GPU."""
    _need(x, F32, "x")
    if x.dim() != 5:
        raise ValueError(f"ensemble_frame_stats: expected (E, T, C, h, w) latents, got {tuple(x.shape)}")
    x = _aligned16(x)
    E, T, Cn, h, w = x.shape
    frame_sum = torch.empty(max(T, 1), dtype=torch.float64, device=x.device)[:T]
    ws = torch.empty(max(T, 1) * FRAME_STATS_BLOCKS, dtype=torch.float64, device=x.device)
    fmap = torch.empty((T, h, w), dtype=F32, device=x.device) if want_map else None
    check(_lib.load().vk_ensemble_frame_stats(_p(x), _p(frame_sum), _p(fmap), _p(ws), E, T, Cn, h * w, _stream()), "vk_ensemble_frame_stats")
    return frame_sum, fmap


def candidate_frame_stats(x, t0, want_map=False):
    """x (K, E, T, C, h, w) f32, the stacked members of K candidates' ensembles; frames [t0, T) are scored -> (frame_sum (K, T - t0) float64,
    total (K,) float64, best 0-dim int32, map (K, T - t0, h, w) float32 or None): ensemble_frame_stats of every candidate's scored frames, bit
    for bit, every candidate's frame sums added in frame order, and the index of the smallest total (ties to the lowest index, NaN never,
    -1 if all are NaN) -- vk_candidate_frame_stats. Nothing is synchronised: all results stay on the GPU."""
    _need(x, F32, "x")
    if x.dim() != 6:
        raise ValueError(f"candidate_frame_stats: expected (K, E, T, C, h, w) latents, got {tuple(x.shape)}")
    if not isinstance(t0, int) or isinstance(t0, bool):
        raise TypeError(f"candidate_frame_stats: t0 must be an int, got {t0!r}")
    x = _aligned16(x)
    K, E, T, Cn, h, w = x.shape
    Ts = T - t0 if 0 <= t0 < T else 0   # (0: a t0 the entry refuses; the buffers below still hold one row)
    rows = max(K * Ts, 1)
    frame_sum = torch.empty(rows, dtype=torch.float64, device=x.device)[:K * Ts].view(K, Ts)
    total = torch.empty(max(K, 1), dtype=torch.float64, device=x.device)[:K]
    best = torch.empty((), dtype=torch.int32, device=x.device)
    ws = torch.empty(rows * FRAME_STATS_BLOCKS, dtype=torch.float64, device=x.device)
    fmap = torch.empty((K, Ts, h, w), dtype=F32, device=x.device) if want_map else None
    check(_lib.load().vk_candidate_frame_stats(_p(x), _p(frame_sum), _p(total), _p(best), _p(fmap), _p(ws), K, E, T, t0, Cn, h * w, _stream()),
          "vk_candidate_frame_stats")
    return frame_sum, total, best, fmap


def heat_overlay_u8(frames, fmap, vmax, alpha=0.6):
    """frames (n, 3, H, W) f32 in [-1, 1] and fmap (n, H / cell, W / cell) f32 >= 0 -> (n, H, W, 3) uint8: every frame blended towards the heat
    colour (255, 32, 0) with weight alpha * min(1, fmap / vmax) of its cell (vk_heat_overlay_u8; a zero map gives frames_to_u8(real=True)'s
    bytes). 1 / vmax is formed here in float32; cell = H / fmap.shape[1] must be the same whole number along both axes."""
    import numpy as np
    _need(frames, F32, "frames")
    _need(fmap, F32, "fmap")
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"heat_overlay_u8: expected (n, 3, H, W) fp32 frames, got {tuple(frames.shape)}")
    n, _, H, W = frames.shape
    if fmap.dim() != 3 or fmap.shape[0] != n or fmap.shape[1] <= 0 or fmap.shape[2] <= 0:
        raise ValueError(f"heat_overlay_u8: expected a (n, H / cell, W / cell) map for {n} frames, got {tuple(fmap.shape)}")
    cell = H // fmap.shape[1]
    if cell <= 0 or cell * fmap.shape[1] != H or cell * fmap.shape[2] != W:
        raise ValueError(f"heat_overlay_u8: a {tuple(fmap.shape[1:])} map does not tile {H} x {W} frames with square cells")
    if not float(vmax) > 0.0:
        raise ValueError(f"heat_overlay_u8: vmax must be positive, got {vmax}")
    inv_vmax = float(np.float32(1) / np.float32(vmax))
    frames, fmap = _aligned16(frames), fmap.contiguous()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=frames.device)
    check(_lib.load().vk_heat_overlay_u8(_p(frames), _p(fmap), _p(out), n, H, W, cell, inv_vmax, float(alpha), _stream()), "vk_heat_overlay_u8")
    return out


# ---- evaluation front door (csrc/fidelity.hip) ----
FIDELITY_TAPS, FIDELITY_TILE_H, FIDELITY_TILE_W = 11, 16, 32   # VK_FIDELITY_* of include/vista_hip.h


def frame_fidelity_u8(a, b):
    """a, b (n, H, W, 3) uint8, dense, on the GPU (the bytes frames_to_u8 writes) -> (sse (n, 3) int64, ssim_sum (n, 3) float64): per frame and
    channel the exact sum of squared differences and the sum of the SSIM index over the (H - 10) * (W - 10) valid window positions
    (vk_frame_fidelity_u8; window: fidelity.WINDOW_F32, fixed-order fp64 reduction). Nothing is synchronised: both results stay on the GPU."""
    from . import fidelity
    _need(a, torch.uint8, "a")
    _need(b, torch.uint8, "b")
    if a.dim() != 4 or a.shape[3] != 3 or a.shape != b.shape:
        raise ValueError(f"frame_fidelity_u8: expected two (n, H, W, 3) uint8 stacks of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"frame_fidelity_u8: a is on {a.device}, b is on {b.device}")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("frame_fidelity_u8: a and b must be dense (contiguous) stacks")
    n, H, W, _ = a.shape
    if W % 4 == 0:   # the kernel loads 4 bytes per lane there (a dense view into another tensor's storage may start anywhere)
        a = a if a.data_ptr() % 4 == 0 else a.clone()
        b = b if b.data_ptr() % 4 == 0 else b.clone()
    lib = _lib.load()
    per_frame = lib.vk_frame_fidelity_ws_bytes(H, W)
    check(min(per_frame, 0), "vk_frame_fidelity_ws_bytes")
    sse = torch.empty((max(n, 1), 3), dtype=torch.int64, device=a.device)[:n]
    ssim_sum = torch.empty((max(n, 1), 3), dtype=torch.float64, device=a.device)[:n]
    ws = torch.empty(max(n, 1) * per_frame // 8, dtype=torch.float64, device=a.device)
    check(lib.vk_frame_fidelity_u8(_p(a), _p(b), _p(sse), _p(ssim_sum), _p(ws), fidelity.window_ptr(), n, H, W, _stream()),
          "vk_frame_fidelity_u8")
    return sse, ssim_sum


# ---- motion scores (csrc/flow.hip) ----
FLOW_BLOCK, FLOW_LEVELS, FLOW_COARSE_RANGE, FLOW_REFINE_RANGE = 8, 3, 7, 2   # VK_FLOW_* of include/vista_hip.h
FLOW_MAX_FRAMES, FLOW_MAX_SIDE = 65535, 65536
FLOW_TILE = FLOW_BLOCK << (FLOW_LEVELS - 1)   # 32: the level-0 side of a level-2 block; H and W are multiples of it


def flow_check_shape(what, n, H, W):
    """The one refusal, by name, of a stack the flow kernels do not take (vista_amd/motion.py and evaluate ask it too, before any launch)."""
    if H < FLOW_TILE or W < FLOW_TILE or H % FLOW_TILE or W % FLOW_TILE:
        raise ValueError(f"{what}: {H} x {W} frames: the block-matching flow takes heights and widths that are multiples of {FLOW_TILE} "
                         f"({FLOW_BLOCK}-px blocks on {FLOW_LEVELS} pyramid levels)")
    if n > FLOW_MAX_FRAMES or H > FLOW_MAX_SIDE or W > FLOW_MAX_SIDE or n * H * W * 21 // 16 > 0x7fffffff:
        raise ValueError(f"{what}: {n} frames of {H} x {W}: at most {FLOW_MAX_FRAMES} frames, sides of {FLOW_MAX_SIDE} and a pyramid of "
                         "2^31 - 1 bytes a call")


def flow_luma_pyramid_u8(frames_u8):
    """frames_u8 (n, H, W, 3) uint8, dense, on the GPU, n >= 1, H and W multiples of 32 -> the three luma levels of every frame in one flat
    uint8 tensor: level 0 (n, H, W), then level 1 (n, H/2, W/2), then level 2 (n, H/4, W/4) (vk_flow_luma_pyramid_u8; flow_pyramid_levels
    gives the views). Nothing is synchronised."""
    _need(frames_u8, torch.uint8, "frames_u8")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        raise ValueError(f"flow_luma_pyramid_u8: expected an (n, H, W, 3) uint8 stack of at least one frame, got {tuple(frames_u8.shape)}")
    if not frames_u8.is_contiguous():
        raise ValueError("flow_luma_pyramid_u8: frames_u8 must be a dense (contiguous) stack")
    n, H, W, _ = frames_u8.shape
    flow_check_shape("flow_luma_pyramid_u8", n, H, W)
    frames_u8 = frames_u8 if frames_u8.data_ptr() % 4 == 0 else frames_u8.clone()   # (a dense view into another tensor's storage may start anywhere)
    pyr = torch.empty(n * H * W * 21 // 16, dtype=torch.uint8, device=frames_u8.device)
    check(_lib.load().vk_flow_luma_pyramid_u8(_p(frames_u8), _p(pyr), n, H, W, _stream()), "vk_flow_luma_pyramid_u8")
    return pyr


def flow_pyramid_levels(pyr, n, H, W):
    """The three levels of flow_luma_pyramid_u8's tensor as (n, H, W), (n, H/2, W/2) and (n, H/4, W/4) views."""
    a, b = n * H * W, n * H * W // 4
    return pyr[:a].view(n, H, W), pyr[a:a + b].view(n, H // 2, W // 2), pyr[a + b:].view(n, H // 4, W // 4)


def block_flow_u8(pyr, n, H, W):
    """pyr: flow_luma_pyramid_u8 of n >= 2 frames of (H, W) -> (flow (n - 1, H/8, W/8, 2) int16, sad (n - 1, H/8, W/8, 2) uint16): per pair of
    consecutive frames and 8 x 8 block the vector (vy, vx) in pixels -- content at (y, x) of frame i is found at (y + vy, x + vx) of frame
    i + 1 --, its SAD and the block's SAD at zero displacement (vk_block_flow_u8). Nothing is synchronised."""
    _need(pyr, torch.uint8, "pyr")
    n, H, W = int(n), int(H), int(W)
    if n < 2:
        raise ValueError(f"block_flow_u8: {n} frames hold no pair of consecutive frames")
    flow_check_shape("block_flow_u8", n, H, W)
    if pyr.dim() != 1 or pyr.numel() != n * H * W * 21 // 16 or not pyr.is_contiguous():
        raise ValueError(f"block_flow_u8: pyr must be the flat, dense tensor flow_luma_pyramid_u8 returns for {n} frames of {H} x {W} "
                         f"({n * H * W * 21 // 16} bytes), got {tuple(pyr.shape)}")
    pyr = pyr if pyr.data_ptr() % 4 == 0 else pyr.clone()
    flow = torch.empty((n - 1, H // FLOW_BLOCK, W // FLOW_BLOCK, 2), dtype=torch.int16, device=pyr.device)
    sad = torch.empty((n - 1, H // FLOW_BLOCK, W // FLOW_BLOCK, 2), dtype=torch.uint16, device=pyr.device)
    check(_lib.load().vk_block_flow_u8(_p(pyr), _p(flow), _p(sad), n, H, W, _stream()), "vk_block_flow_u8")
    return flow, sad


def flow_pair_sums(flow, sad, flow_ref=None):
    """flow (pairs, gy, gx, 2) int16 and sad (pairs, gy, gx, 2) uint16 of block_flow_u8, flow_ref: a second field of flow's shape or None ->
    (pairs, 5) int64 on the GPU: per pair the blocks with a non-zero vector, sum |v|^2, sum SAD, sum SAD at zero, sum |v - v_ref|^2 (0 without
    flow_ref) (vk_flow_pair_sums). Nothing is synchronised."""
    _need(flow, torch.int16, "flow")
    _need(sad, torch.uint16, "sad")
    if flow.dim() != 4 or flow.shape[3] != 2 or sad.shape != flow.shape or flow.shape[0] < 1 or flow.shape[1] * flow.shape[2] < 1:
        raise ValueError(f"flow_pair_sums: expected flow and sad of one shape (pairs, gy, gx, 2), got {tuple(flow.shape)} and {tuple(sad.shape)}")
    if flow_ref is not None:
        _need(flow_ref, torch.int16, "flow_ref")
        if flow_ref.shape != flow.shape:
            raise ValueError(f"flow_pair_sums: flow is {tuple(flow.shape)}, flow_ref {tuple(flow_ref.shape)}: the two fields must have one shape")
    for name, t in (("flow", flow), ("sad", sad), ("flow_ref", flow_ref)):
        if t is not None and t.device != flow.device:
            raise ValueError(f"flow_pair_sums: flow is on {flow.device}, {name} is on {t.device}")
        if t is not None and not t.is_contiguous():
            raise ValueError(f"flow_pair_sums: {name} must be dense (contiguous)")
    aligned = lambda t: t if t is None or t.data_ptr() % 4 == 0 else t.clone()   # noqa: E731
    flow, sad, flow_ref = aligned(flow), aligned(sad), aligned(flow_ref)
    pairs, blocks = flow.shape[0], flow.shape[1] * flow.shape[2]
    out = torch.empty((pairs, 5), dtype=torch.int64, device=flow.device)
    check(_lib.load().vk_flow_pair_sums(_p(flow), _p(sad), _p(flow_ref), _p(out), pairs, blocks, _stream()), "vk_flow_pair_sums")
    return out


# ---- CLIP-space scores (csrc/perceptual.hip) ----
EMBED_MAX_ROWS, EMBED_MAX_DIM, EMBED_MMD_TILE = 1 << 20, 1 << 16, 64   # VK_EMBED_* of include/vista_hip.h


def clip_preprocess_patches_u8(frames_u8, out_hw=224, patch=14, kpad=None, antialias=True, mean=CLIP_MEAN, std=CLIP_STD):
    """frames_u8 (n, H, W, 3) uint8, dense, on the GPU (the bytes frames_to_u8 writes) -> what clip_preprocess_patches returns for
    `frames_u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0` (an IEEE fp32 division), bit for bit, without the fp32 frames: the bytes are
    converted once, in LDS (vk_clip_preprocess_patches_u8). Any width and any base address are taken. Nothing is synchronised."""
    _need(frames_u8, torch.uint8, "frames_u8")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        _refuse("frames_u8", frames_u8, "must be (n, H, W, 3), n >= 1")
    if not frames_u8.is_contiguous():
        _refuse("frames_u8", frames_u8, "must be a dense (contiguous) stack")
    n, H, W, _ = frames_u8.shape
    g = out_hw // patch
    kp = kpad or ceil_to(3 * patch * patch, 64)
    out = torch.zeros((n * (1 + g * g), kp), dtype=BF16, device=frames_u8.device)
    down = antialias and max(H / out_hw, W / out_hw) > 1  # kornia blurs BOTH axes as soon as either one is downscaled
    (sy, ky), (sx, kx) = (antialias_blur_params(H, out_hw), antialias_blur_params(W, out_hw)) if down else ((1.0, 1), (1.0, 1))
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(_lib.load().vk_clip_preprocess_patches_u8(_p(frames_u8), _p(out), n, H, W, out_hw, patch, kp, sy, sx, ky, kx, m3, s3, _stream()),
          "vk_clip_preprocess_patches_u8")
    return out


def _embedding(t, name, cols=None):
    _need(t, F32, name)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (cols is not None and t.shape[1] != cols):
        _refuse(name, t, "must be (rows, d) with rows, d >= 1" + ("" if cols is None else f" and d = {cols}"))
    if not t.is_contiguous():
        _refuse(name, t, "must be dense (contiguous)")
    if t.shape[0] > EMBED_MAX_ROWS or t.shape[1] > EMBED_MAX_DIM:
        _refuse(name, t, f"at most {EMBED_MAX_ROWS} rows of at most {EMBED_MAX_DIM} columns")


def embed_row_stats(a, b):
    """a, b (n, d) fp32, dense, on the GPU -> (n, 3) float64 on the GPU: per row a.b, a.a, b.b, products of fp32 values summed in fp64 in one
    fixed order (vk_embed_row_stats). `a is b` gives three equal bit patterns per row. Nothing is synchronised."""
    _embedding(a, "a")
    _embedding(b, "b", cols=a.shape[1])
    if a.shape != b.shape or a.device != b.device:
        _refuse("b", b, f"must pair up with a {tuple(a.shape)} on {a.device}")
    out = torch.empty((a.shape[0], 3), dtype=torch.float64, device=a.device)
    check(_lib.load().vk_embed_row_stats(_p(a), _p(b), _p(out), a.shape[0], a.shape[1], _stream()), "vk_embed_row_stats")
    return out


def embed_mmd_sums(x, y, sigma):
    """x (m, d), y (n, d) fp32, dense, on the GPU -> 3 float64 on the GPU: the sums of 1 - k over the pairs i < j of x^, over the pairs of y^,
    and over every (x^_i, y^_j); u^ = u / |u|, k(u, v) = exp(-|u - v|^2 / (2 sigma^2)) (vk_embed_mmd_sums: fp32 differences, expm1, fp64
    sums in a fixed order). Nothing is synchronised."""
    _embedding(x, "x")
    _embedding(y, "y", cols=x.shape[1])
    if x.device != y.device:
        _refuse("y", y, f"must be on {x.device}")
    if not (isinstance(sigma, (int, float)) and 0 < sigma < math.inf):
        raise ValueError(f"embed_mmd_sums: sigma must be a positive finite number, got {sigma!r}")
    (m, d), n = x.shape, y.shape[0]
    lib = _lib.load()
    ws_bytes = lib.vk_embed_mmd_ws_bytes(m, n, d)
    check(min(ws_bytes, 0), "vk_embed_mmd_ws_bytes")
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    check(lib.vk_embed_mmd_sums(_p(x), _p(y), _p(out), _p(ws), m, n, d, float(sigma), _stream()), "vk_embed_mmd_sums")
    return out


# ---- exchange packing of the frame-sharded step (csrc/reshard.hip, ABI v9) ----
def row_boxes(boxes):
    """A list of (src_row, dst_row, src_stride_b, src_stride_t, dst_stride_b, dst_stride_t, nb, nt, ns) tuples -> the VkRowBoxes the library
    reads. n is the list's length whatever it is (the library refuses 0 and more than VK_RESHARD_MAX_BOXES); boxes past the struct's capacity
    are not stored."""
    rb = _lib.VkRowBoxes()
    rb.n = len(boxes)
    for i, b in enumerate(boxes[:_lib.VK_RESHARD_MAX_BOXES]):
        if len(b) != 9:
            raise ValueError(f"row_boxes: box {i} has {len(b)} entries, expected 9 (src_row, dst_row, four strides, nb, nt, ns)")
        rb.box[i] = _lib.VkRowBox(*[int(v) for v in b], 0)
    return rb


def copy_row_boxes(src, dst, boxes):
    """vk_copy_row_boxes: copy the strided row boxes of a plan from src (src_rows, C) into dst (dst_rows, C) in one launch, on the current stream.
    src and dst are 2-D views of one dtype and one row width with dense rows; `boxes` is a list of 9-tuples (row_boxes) or a prebuilt
    VkRowBoxes. The destination rows of a plan must not overlap. Rows dst is not told to write keep their contents."""
    if src.dim() != 2 or dst.dim() != 2:
        raise ValueError(f"copy_row_boxes: expected 2-D (rows, C) views, got {tuple(src.shape)} and {tuple(dst.shape)}")
    if src.dtype != dst.dtype:
        raise ValueError(f"copy_row_boxes: src is {src.dtype}, dst is {dst.dtype}")
    if src.shape[1] != dst.shape[1]:
        raise ValueError(f"copy_row_boxes: row widths differ: src {src.shape[1]}, dst {dst.shape[1]}")
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("copy_row_boxes: src and dst must have dense rows (contiguous 2-D views)")
    if not (src.is_cuda and dst.is_cuda):
        raise _lib.VistaHipError("copy_row_boxes: tensors must live on the GPU (vista_amd has no CPU / eager fallback)")
    rb = boxes if isinstance(boxes, _lib.VkRowBoxes) else row_boxes(boxes)
    check(_lib.load().vk_copy_row_boxes(_p(src), _p(dst), C.byref(rb), src.shape[0], dst.shape[0], src.shape[1] * src.element_size(),
                                        _stream()), "vk_copy_row_boxes")
    return dst


# ---- drive front door (csrc/overlay.hip) ----
OVERLAY_MAX_SETS, OVERLAY_MAX_STROKES, OVERLAY_MAX_SEGMENTS = 8, 32, 64   # VK_OVERLAY_MAX_* of include/vista_hip.h


def stroke_counts(sets):
    """(sets, strokes, segments) a list of stroke sets occupies in a plan."""
    return len(sets), sum(len(s) for s in sets), sum(len(stroke[3]) for s in sets for stroke in s)


def stroke_plan(sets):
    """A list of stroke sets -> the VkStrokePlan the library reads. A set is a list of strokes (colour (3 floats in [0, 255]), alpha, r, segments),
    a segment (ax, ay, bx, by) in pixel coordinates, a disc a segment with a == b. inv_len2 = 1 / |b - a|^2 is formed here in float32, one
    rounding per operation (0 for a disc). The counts are stored whatever they are (the library refuses what exceeds VK_OVERLAY_MAX_*);
    entries past the struct's capacity are not stored."""
    import numpy as np
    f = np.float32
    plan = _lib.VkStrokePlan()
    plan.n_sets, plan.n_strokes, plan.n_segments = stroke_counts(sets)
    k = g = 0
    for i, strokes in enumerate(sets):
        if i < OVERLAY_MAX_SETS:
            plan.set[i] = _lib.VkStrokeSet(k, len(strokes))
        for colour, alpha, r, segments in strokes:
            if k < OVERLAY_MAX_STROKES:
                plan.stroke[k] = _lib.VkStroke((C.c_float * 3)(*[float(c) for c in colour]), float(alpha), float(r), g, len(segments))
            k += 1
            for ax, ay, bx, by in segments:
                if g < OVERLAY_MAX_SEGMENTS:
                    dx, dy = f(bx) - f(ax), f(by) - f(ay)
                    l2 = dx * dx + dy * dy
                    plan.seg[g] = _lib.VkStrokeSegment(float(ax), float(ay), float(bx), float(by), 0.0 if l2 == 0 else float(f(1) / l2))
                g += 1
    return plan


def stroke_overlay(frames, sets, set_of_frame, out=None):
    """vk_stroke_overlay_u8: frames (n, H, W, 3) uint8, dense, on the GPU -> the frames with anti-aliased strokes drawn in; frame i takes
    sets[set_of_frame[i]], a value outside [0, len(sets)) (-1) copies it. `sets` is a list of stroke sets (stroke_plan) or a prebuilt VkStrokePlan,
    `set_of_frame` a sequence of ints or an int32 tensor on the frames' device. `out` may be `frames` itself (in place); by default a new
    tensor. The bytes equal the numpy float32 evaluation of the header's definition (tests/_overlay_ref.py)."""
    _need(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"stroke_overlay: expected (n, H, W, 3) uint8 frames, got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("stroke_overlay: frames must be a dense (contiguous) stack")
    n, H, W, _ = frames.shape
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError("stroke_overlay: out must be a dense uint8 stack of the frames' shape on the frames' device")
    if not torch.is_tensor(set_of_frame):
        set_of_frame = torch.tensor([int(v) for v in set_of_frame], dtype=torch.int32, device=frames.device)
    _need(set_of_frame, torch.int32, "set_of_frame")
    if set_of_frame.dim() != 1 or set_of_frame.shape[0] != n or set_of_frame.device != frames.device or not set_of_frame.is_contiguous():
        raise ValueError(f"stroke_overlay: set_of_frame must hold one int32 per frame ({n}) on the frames' device")
    plan = sets if isinstance(sets, _lib.VkStrokePlan) else stroke_plan(sets)
    check(_lib.load().vk_stroke_overlay_u8(_p(frames), _p(out), _p(set_of_frame), C.byref(plan), n, H, W, _stream()), "vk_stroke_overlay_u8")
    return out


# ---- denoising-loss front door (csrc/loss.hip) ----
LOSS_STATS_BLOCKS, LOSS_MAX_CHANNELS = 16, 64   # VK_LOSS_STATS_BLOCKS, VK_LOSS_MAX_CHANNELS of include/vista_hip.h


def _latents4(t, name):
    _need(t, F32, name)
    if t.dim() != 4 or not t.is_contiguous():
        raise ValueError(f"{name}: expected dense (n, C, h, w) fp32 latents, got {tuple(t.shape)} with strides {tuple(t.stride())}")


def _per_image(t, name, like, numel):
    if t is None:
        return
    _dense(t, name, F32, like.get_device(), 4, numel)


def loss_noise_input(x, noise, sigma, mask=None, offset=None, level=0.0, out=None):
    """x, noise (n, C, h, w) f32, sigma (n,), mask (n,) or None, offset (n, C) or None -> x + (noise + level * offset) * ((1 - mask) * sigma),
    bit for bit torch's fp32 expression on the CPU (vk_loss_noise_input). Operands are taken where they lie (16-byte lanes where they allow it);
    nothing is synchronised."""
    _latents4(x, "x")
    _latents4(noise, "noise")
    if noise.shape != x.shape or noise.device != x.device:
        raise ValueError(f"loss_noise_input: noise {tuple(noise.shape)} on {noise.device} does not match x {tuple(x.shape)} on {x.device}")
    n, Cn, h, w = x.shape
    _per_image(sigma, "sigma", x, n)
    _per_image(mask, "mask", x, n)
    _per_image(offset, "offset", x, n * Cn)
    if out is None:
        out = torch.empty_like(x)
    else:
        _latents4(out, "out")
        if out.shape != x.shape or out.device != x.device:
            raise ValueError("loss_noise_input: out must have x's shape and device")
    check(_lib.load().vk_loss_noise_input(_p(x), _p(noise), _p(sigma), _p(mask), _p(offset), float(level), _p(out), n, Cn, h * w, _stream()),
          "vk_loss_noise_input")
    return out


def fourier_highpass_fits(H, W):
    """Can vk_fourier_highpass hold an H x W plane (include/vista_hip.h: 16 H W + 16 (H + W) <= 160 KiB)? Pure arithmetic: no library, no GPU."""
    return H >= 1 and W >= 1 and 16 * H * W + 16 * (H + W) <= 160 * 1024


def fourier_highpass(a, keep, scale, b=None, cond_mask=None):
    """a (n, C, H, W) f32 -> the reference's fourier_filter of every plane of d = a (b None), a - b, or (a * (1 - m) + b * m) - b with
    m = cond_mask[image] (vk_fourier_highpass). keep (H, W) uint8 on the GPU: 1 where the UNSHIFTED frequency is kept, 0 where it is multiplied
    by `scale`. Nothing is synchronised."""
    _latents4(a, "a")
    n, Cn, H, W = a.shape
    if b is not None:
        _latents4(b, "b")
        if b.shape != a.shape or b.device != a.device:
            raise ValueError(f"fourier_highpass: b {tuple(b.shape)} on {b.device} does not match a {tuple(a.shape)} on {a.device}")
    if cond_mask is not None and b is None:
        raise ValueError("fourier_highpass: cond_mask blends a with b; give b")
    _per_image(cond_mask, "cond_mask", a, n)
    _dense(keep, "keep", torch.uint8, a.get_device(), 1, H * W)
    if not fourier_highpass_fits(H, W):
        raise OperandError(f"fourier_highpass: a {H} x {W} plane does not fit the workgroup's LDS (16 H W + 16 (H + W) <= 160 KiB; 72 x 128 does)")
    y = torch.empty_like(a)
    check(_lib.load().vk_fourier_highpass(_p(a), _p(b), _p(cond_mask), _p(keep), float(scale), _p(y), n * Cn, Cn, H, W, _stream()),
          "vk_fourier_highpass")
    return y


def loss_stats(out, target, num_frames, cond_mask=None, hf=None, l1=False):
    """out, target (B * T, C, h, w) f32, T = num_frames -> sums (B * T, 3) float64 on the GPU: per frame S0 = sum e, S1 = sum e * aux_w,
    S2 = sum |hf|^p (vk_loss_stats; include/vista_hip.h states e, aux_w and the order of the sums). Two launches; nothing is synchronised."""
    _latents4(out, "out")
    _latents4(target, "target")
    if target.shape != out.shape or target.device != out.device:
        raise ValueError(f"loss_stats: target {tuple(target.shape)} on {target.device} does not match out {tuple(out.shape)} on {out.device}")
    n, Cn, h, w = out.shape
    if not isinstance(num_frames, int) or num_frames < 1 or n % num_frames:
        raise ValueError(f"loss_stats: {n} images are no whole number of clips of {num_frames} frames")
    if hf is not None:
        _latents4(hf, "hf")
        if hf.shape != out.shape or hf.device != out.device:
            raise ValueError("loss_stats: hf must have out's shape and device")
    _per_image(cond_mask, "cond_mask", out, n)
    B = n // num_frames
    sums = torch.empty((max(n, 1), 3), dtype=torch.float64, device=out.device)[:n]
    ws = torch.empty(B * Cn * LOSS_STATS_BLOCKS, dtype=torch.float64, device=out.device) if num_frames > 1 else None   # (T == 1: launch 1 is skipped)
    check(_lib.load().vk_loss_stats(_p(out), _p(target), _p(cond_mask), _p(hf), _p(sums), _p(ws), B, num_frames, Cn, h * w, int(bool(l1)), _stream()),
          "vk_loss_stats")
    return sums


# ---- Motion-JPEG video output (csrc/jpeg.hip) ----
JPEG_MAX_EXTENT, JPEG_MAX_COUNT = 65535, 2 ** 31 - 1   # the extent limits include/vista_hip.h states beside the three prototypes


def _jpeg_operand(t, name, dtype, ndim, last, align):
    """An operand of the JPEG entry points: a dense `ndim`-D tensor of `dtype` on a GPU whose last extent is `last`, base address a multiple of
    `align` bytes. Refused by name, never cloned."""
    if not torch.is_tensor(t):
        raise OperandError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.dtype is dtype and t.is_cuda and t.dim() == ndim and t.shape[-1] == last and t.is_contiguous() and (t.data_ptr() & (align - 1)) == 0:
        return
    rule = (f"dtype must be {dtype}" if t.dtype is not dtype else "must be on the GPU (no CPU fallback)" if not t.is_cuda
            else f"must be {ndim}-D with a last extent of {last}" if t.dim() != ndim or t.shape[-1] != last
            else "must be dense (contiguous)" if not t.is_contiguous() else f"base address must be a multiple of {align} bytes")
    raise OperandError(f"{name}: {rule} (got {tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}, address % 16 = {t.data_ptr() & 15})")


def jpeg_quant(quality):
    """The VkJpegQuant of a quality: libjpeg's scaling of the Annex K tables (video.jpeg_tables), in zigzag order."""
    from . import video
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise OperandError(f"quality: a JPEG quality is an integer from 1 to 100, got {quality!r}")
    luma, chroma = video.jpeg_tables(quality)["quant"]
    q = _lib.VkJpegQuant()
    q.quality = quality
    for k, nat in enumerate(video.ZIGZAG):
        q.luma[k], q.chroma[k] = luma[nat], chroma[nat]
    return q


def jpeg_dct_quant(frames, quality):
    """frames (n, H, W, 3) uint8, dense, on the GPU (what frames_to_u8, heat_overlay_u8 and stroke_overlay write) -> coef (n, 6 * mcu_h * mcu_w, 64)
    int16: the quantised DCT coefficients of a 4:2:0 baseline JPEG at `quality`, zigzag order, blocks in scan order (vk_jpeg_dct_quant_u8).
    Nothing is synchronised."""
    _jpeg_operand(frames, "frames", torch.uint8, 4, 3, 1)
    n, H, W, _ = frames.shape
    if not (n >= 1 and 1 <= H <= JPEG_MAX_EXTENT and 1 <= W <= JPEG_MAX_EXTENT):
        raise OperandError(f"frames: n >= 1 and 1 <= H, W <= {JPEG_MAX_EXTENT}, got {tuple(frames.shape)}")
    q = jpeg_quant(quality)
    mcu_h, mcu_w = (H + 15) // 16, (W + 15) // 16
    if 6 * n * mcu_h * mcu_w > JPEG_MAX_COUNT or 3 * n * H * W > JPEG_MAX_COUNT:
        raise OperandError(f"frames: {tuple(frames.shape)} is {6 * n * mcu_h * mcu_w} blocks and {3 * n * H * W} bytes; both must stay below 2^31 "
                           "(encode fewer frames per call)")
    coef = torch.empty((n, 6 * mcu_h * mcu_w, 64), dtype=torch.int16, device=frames.device)
    check(_lib.load().vk_jpeg_dct_quant_u8(_p(frames), _p(coef), C.byref(q), n, H, W, _stream()), "vk_jpeg_dct_quant_u8")
    return coef


def jpeg_entropy(coef, mcu_h, mcu_w):
    """coef (n, 6 * mcu_h * mcu_w, 64) int16 from jpeg_dct_quant -> (scan, offsets): `scan` a uint8 GPU tensor that holds every frame's
    entropy-coded scan back to back, `offsets` the n * mcu_h + 1 exclusive byte offsets of the restart intervals as a CPU int64 tensor (frame i is
    scan[offsets[i * mcu_h] : offsets[(i + 1) * mcu_h]]). vk_jpeg_interval_sizes, a cumulative sum, ONE transfer of the offsets to the host (the
    only synchronisation: the output's size is data), vk_jpeg_entropy_write."""
    _jpeg_operand(coef, "coef", torch.int16, 3, 64, 16)
    for name, v in (("mcu_h", mcu_h), ("mcu_w", mcu_w)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 4096:
            raise OperandError(f"{name}: a whole number of MCUs from 1 to 4096, got {v!r}")
    n, blocks, _ = coef.shape
    if n < 1 or blocks != 6 * mcu_h * mcu_w or n * blocks > JPEG_MAX_COUNT:
        raise OperandError(f"coef: {tuple(coef.shape)} does not hold n >= 1 frames of 6 * {mcu_h} * {mcu_w} = {6 * mcu_h * mcu_w} blocks "
                           "(and at most 2^31 - 1 blocks in all)")
    lib = _lib.load()
    sizes = torch.empty(n * mcu_h, dtype=torch.int32, device=coef.device)
    check(lib.vk_jpeg_interval_sizes(_p(coef), _p(sizes), n, mcu_h, mcu_w, n * blocks, _stream()), "vk_jpeg_interval_sizes")
    offsets = torch.zeros(n * mcu_h + 1, dtype=torch.int64, device=coef.device)
    offsets[1:] = torch.cumsum(sizes, 0, dtype=torch.int64)
    host = offsets.cpu()
    total = int(host[-1])
    if not 1 <= total <= JPEG_MAX_COUNT:
        raise OperandError(f"coef: the scans take {total} bytes; the output must stay below 2^31 (encode fewer frames per call)")
    scan = torch.empty(total, dtype=torch.uint8, device=coef.device)
    check(lib.vk_jpeg_entropy_write(_p(coef), _p(offsets), _p(scan), total, n, mcu_h, mcu_w, n * blocks, _stream()), "vk_jpeg_entropy_write")
    return scan, host


# ---- PNG output (csrc/png.hip) ----
PNG_MAX_EXTENT, PNG_MAX_SEGMENT_BYTES, PNG_PLAN_WORDS = 65535, 1 << 24, 420   # the limits include/vista_hip.h states beside the three prototypes


def png_filter(frames):
    """frames (n, H, W, 3) uint8, dense, on the GPU -> rows (n, H, 1 + 3 W) uint8: per row the PNG filter type libpng's heuristic picks (the smallest
    sum of |byte as int8| over None, Sub, Up, Average, Paeth; the lowest type on a tie) and the filtered bytes (vk_png_filter_u8). Nothing is
    synchronised."""
    _jpeg_operand(frames, "frames", torch.uint8, 4, 3, 1)
    n, H, W, _ = frames.shape
    if not (n >= 1 and 1 <= H <= PNG_MAX_EXTENT and 1 <= W <= PNG_MAX_EXTENT):
        raise OperandError(f"frames: n >= 1 and 1 <= H, W <= {PNG_MAX_EXTENT}, got {tuple(frames.shape)}")
    if n * H * (1 + 3 * W) > JPEG_MAX_COUNT:
        raise OperandError(f"frames: {tuple(frames.shape)} gives {n * H * (1 + 3 * W)} bytes of rows; they must stay below 2^31 (encode fewer frames "
                           "per call)")
    rows = torch.empty((n, H, 1 + 3 * W), dtype=torch.uint8, device=frames.device)
    check(_lib.load().vk_png_filter_u8(_p(frames), _p(rows), n, H, W, _stream()), "vk_png_filter_u8")
    return rows


def png_deflate(rows, seg_rows=16):
    """rows (n, H, row_bytes) uint8, dense, on the GPU (any row_bytes) -> (stream, offsets, adler): `stream` a uint8 GPU tensor that holds every
    frame's raw deflate data back to back, one dynamic-Huffman block per segment of `seg_rows` rows; `offsets` the n * segs + 1 exclusive byte
    offsets of the segments as a CPU int64 tensor (segs = ceil(H / seg_rows); frame i is stream[offsets[i * segs] : offsets[(i + 1) * segs]]);
    `adler` (n * segs, 2) int64 on the CPU, the Adler-32 sums (s1, s2) of each segment's bytes alone. vk_png_deflate_plan builds the trees on the
    GPU; a cumulative sum and ONE transfer of the offsets to the host (the only synchronisation between the kernels: the output's size is data);
    vk_png_deflate_write."""
    _jpeg_operand(rows, "rows", torch.uint8, 3, rows.shape[-1] if torch.is_tensor(rows) and rows.dim() else 0, 1)
    if isinstance(seg_rows, bool) or not isinstance(seg_rows, int) or not 1 <= seg_rows <= JPEG_MAX_COUNT:
        raise OperandError(f"seg_rows: a whole number of rows per segment, at least 1, got {seg_rows!r}")
    n, H, row_bytes = rows.shape
    if n < 1 or H < 1 or row_bytes < 1 or n * H * row_bytes > JPEG_MAX_COUNT:
        raise OperandError(f"rows: {tuple(rows.shape)} must hold n, H, row_bytes >= 1 and at most 2^31 - 1 bytes (encode fewer frames per call)")
    if min(seg_rows, H) * row_bytes > PNG_MAX_SEGMENT_BYTES:
        raise OperandError(f"rows: a segment of {min(seg_rows, H)} rows of {row_bytes} bytes is {min(seg_rows, H) * row_bytes} bytes; at most "
                           f"{PNG_MAX_SEGMENT_BYTES} (lower seg_rows)")
    segs = (H + seg_rows - 1) // seg_rows
    lib, dev = _lib.load(), rows.device
    sizes = torch.empty(n * segs, dtype=torch.int32, device=dev)
    adler = torch.empty((n * segs, 2), dtype=torch.int32, device=dev)
    plan = torch.empty((n * segs, PNG_PLAN_WORDS), dtype=torch.int32, device=dev)
    check(lib.vk_png_deflate_plan(_p(rows), _p(sizes), _p(adler), _p(plan), n, H, row_bytes, seg_rows, n * segs, _stream()), "vk_png_deflate_plan")
    offsets = torch.zeros(n * segs + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(sizes, 0, dtype=torch.int64)
    host = offsets.cpu()
    total = int(host[-1])
    if not 1 <= total <= JPEG_MAX_COUNT:
        raise OperandError(f"rows: the streams take {total} bytes; the output must stay below 2^31 (encode fewer frames per call)")
    stream = torch.empty(total, dtype=torch.uint8, device=dev)
    check(lib.vk_png_deflate_write(_p(rows), _p(plan), _p(offsets), _p(stream), total, n, H, row_bytes, seg_rows, n * segs, _stream()),
          "vk_png_deflate_write")
    return stream, host, adler.cpu().to(torch.int64)
