"""Guard bands and poisoned outputs for the kernel tests: every tensor a kernel is handed sits inside an arena of known bytes.

    with guarded(ops) as g:          # ops.torch is a proxy for the duration; restored in `finally`
        i = embed(inputs)            # every tensor of a case's inputs copied into an arena on the GPU (replaces to_device)
        outs = case.run(ops, i)      # every torch.empty / empty_like / zeros / ones of ops.py is the interior of an arena
        ...judge outs...
        verify()                     # synchronise; every guard byte still 0xFF; every embedded input bitwise what was put in

An arena is one flat uint8 allocation [front guard | tensor | back guard]. Guards are filled with byte 0xFF, and so is the interior of an
`empty` / `empty_like` tensor (`zeros` and `ones` keep their value). 0xFF repeated is NaN in bf16, fp16, fp32, fp64, e4m3 and E8M0
(tests/test_extent_cpu.py), so the one byte makes
  an output element the kernel never stores   a NaN in the result (no stale block of the caching allocator can stand in for the store),
  a load past the end of an operand           a NaN wherever it reaches the result,
  a store past the end of a tensor            a changed guard byte, which verify() names by tensor, side and offset.
A guard is max(4 KiB, 320 rows of the tensor's last dimension) rounded up to 256 B and capped at 8 MiB: 320 rows / columns is the tallest / widest
tile any kernel variant owns. The front guard is a multiple of 256 B, so the tensor keeps the allocator's alignment (the 16-byte paths are chosen
as without guards); the back guard starts at the first byte after the tensor. All guard memory is allocated memory: a wrong kernel damages a
guard, never an unmapped page.

Skewed and strided arenas (the operand contract of include/vista_hip.h has a misaligned side and a padded-row side of every switch): put / embed /
scratch / empty take `skew`, bytes between the aligned start and the tensor's first byte, and `ld`, the row stride in elements (rows = all dims
but the last, flattened; ld >= the last dim). The arena is then [front guard | skew | row 0 | gap | row 1 | gap ... | last row | back guard]: the
skew bytes and the gaps between rows are poison and verify() checks them as guard memory -- a store whose address was rounded down lands in the
skew, a store of a whole ld-wide row in a gap. The tensor is a view of exactly the rows: data_ptr() % 256 == skew % 256, stride(-2) == ld.

No conftest, no hook in ops.py: the proxy forwards every attribute to torch except the factories through which ops.py creates kernel-visible
memory. What ops.py creates another way (the `colsum` of a LayerNorm fold, the operand of pack_ff_out) is re-homed by rehome_pack(), which the
cases call on such packs. The per-stream split-K workspace ops.py caches is dropped when a context is entered and left, so each context allocates
its own, guarded, and none outlives its context. Nothing here imports vista_amd or touches a GPU at import time."""
import contextlib

import torch

POISON = 0xFF
GUARD_MIN, GUARD_ROWS, GUARD_ALIGN, GUARD_MAX = 4096, 320, 256, 8 << 20
FACTORIES = ("empty", "empty_like", "zeros", "ones", "full")
TOTALS = {"arenas": 0, "largest_guard": 0, "contexts": 0}   # over the process, for the record (profiles/extent_guard.txt)
_ACTIVE = None


def guard_bytes(shape, itemsize):
    row = (shape[-1] if len(shape) else 1) * itemsize
    g = max(GUARD_MIN, GUARD_ROWS * row)
    return min((g + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN, GUARD_MAX)


class Arena:
    """[front guard | tensor | back guard] in one uint8 allocation. role: "empty" (poisoned interior), "zeros", "ones", "full" (outputs and
    workspaces: guards checked), "input" (guards checked and the interior compared with `saved`), "scratch" (a copy the kernel may write)."""

    def __init__(self, shape, dtype, device, role, label, skew=0, ld=None):
        self.shape, self.dtype, self.role, self.label = tuple(shape), dtype, role, label
        item = self.item = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in self.shape:
            n *= s
        self.cols = self.shape[-1] if self.shape else 1
        self.rows = n // self.cols if self.cols else 0
        self.skew, self.ld = int(skew), (self.cols if ld is None else int(ld))
        if self.skew < 0 or self.skew % item or self.ld < self.cols or (self.ld != self.cols and len(self.shape) < 2):
            raise ValueError(f"arena of {self.shape} {dtype}: skew {skew} must be a non-negative multiple of the element size, ld {ld} >= the last dim")
        self.strided = self.ld != self.cols and self.rows > 1
        # the bytes from the tensor's first to its last: dense, or `rows` rows that start ld elements apart
        self.nbytes = ((self.rows - 1) * self.ld + self.cols) * item if self.strided else n * item
        self.guard = guard_bytes(self.shape, item)
        self.start = self.guard + self.skew
        self.base = torch.empty(self.start + self.nbytes + self.guard, dtype=torch.uint8, device=device)
        self.base.fill_(POISON)
        self.saved = None

    def interior(self):
        """The tensor's own bytes: flat (dense), or (rows, row bytes) without the gaps (strided)."""
        if self.strided:
            return self.base.as_strided((self.rows, self.cols * self.item), (self.ld * self.item, 1), self.start)
        return self.base[self.start:self.start + self.nbytes]

    def tensor(self):
        if self.strided:
            strides, acc = [1], self.ld
            for s in reversed(self.shape[1:-1]):
                strides.insert(0, acc)
                acc *= s
            strides.insert(0, acc)
            flat = self.base[self.start:self.start + self.nbytes].view(self.dtype)
            return flat.as_strided(self.shape, strides, flat.storage_offset())   # (as_strided counts from the storage's start)
        return self.interior().view(self.dtype).view(self.shape)

    def sides(self):
        """Every run of guard bytes: (name, bytes, position of byte k of it in words). The front guard includes the skew."""
        out = [("front", self.base[:self.start]), ("back", self.base[self.start + self.nbytes:])]
        if self.strided:
            out.append(("gap", self.base.as_strided((self.rows - 1, (self.ld - self.cols) * self.item), (self.ld * self.item, 1),
                                                    self.start + self.cols * self.item)))
        return tuple(out)

    def where(self, side, k):
        if side == "front":
            return f"{self.start - k} bytes before its first byte"
        if side == "back":
            return f"{k} bytes past its last byte"
        per = (self.ld - self.cols) * self.item
        return f"{k % per} bytes past the end of row {k // per}"

    def __repr__(self):
        return f"{self.label} {self.shape} {self.dtype}"


class _TorchProxy:
    """Stands in for the module global `torch` of vista_amd/ops.py: the factories allocate arenas, everything else is torch's."""

    def __init__(self, session):
        self._session = session

    def __getattr__(self, name):
        return getattr(torch, name)


def _factory(name):
    def make(self, *args, **kw):
        return self._session._make(name, args, kw)
    make.__name__ = name
    return make


for _name in FACTORIES:
    setattr(_TorchProxy, _name, _factory(_name))


class Session:
    def __init__(self, ops):
        self.ops, self.arenas, self._storages, self._counted = ops, [], {}, 0
        self.proxy = _TorchProxy(self)

    # ---- allocation ----
    def _new(self, shape, dtype, device, role, label, skew=0, ld=None):
        a = Arena(shape, dtype, device, role, label, skew, ld)
        self.arenas.append(a)
        self._storages[a.base.untyped_storage().data_ptr()] = a
        return a

    def _make(self, name, args, kw):
        """The shape, dtype and layout torch's own factory would give (asked of the meta device), as the interior of a new arena."""
        meta = getattr(torch, name)(*args, **{**kw, "device": "meta"})
        if not meta.is_contiguous():
            raise NotImplementedError(f"guarded torch.{name}: a non-contiguous result {tuple(meta.shape)} / {meta.stride()} has no arena form")
        device = kw.get("device")
        if device is None:
            device = args[0].device if name.endswith("_like") else "cpu"
        a = self._new(meta.shape, meta.dtype, device, name.replace("_like", ""), f"torch.{name}")
        t = a.tensor()
        if name == "zeros":
            t.zero_()
        elif name == "ones":
            t.fill_(1)
        elif name == "full":
            t.fill_(args[1] if len(args) > 1 else kw["fill_value"])
        return t

    def put(self, t, device="cuda", writable=False, label="input", skew=0, ld=None):
        """A copy of t (values, shape and dtype; dense, or skewed / strided: module docstring) inside an arena on `device`. Unless writable,
        verify() holds it bitwise unchanged."""
        a = self._new(t.shape, t.dtype, device, "scratch" if writable else "input", label, skew, ld)
        out = a.tensor()
        out.copy_(t)
        if not writable:
            a.saved = a.interior().clone()
        return out

    def empty(self, shape, dtype, device="cuda", skew=0, ld=None, label="out"):
        """A poisoned output at a chosen alignment and row stride: what ops.py's own torch.empty cannot be asked for."""
        return self._new(shape, dtype, device, "empty", label, skew, ld).tensor()

    def owns(self, t):
        return t.untyped_storage().data_ptr() in self._storages

    # ---- verification ----
    def verify(self):
        if any(a.base.is_cuda for a in self.arenas):
            torch.cuda.synchronize()
        fails = []
        for a in self.arenas:
            for side, g in a.sides():
                bad = (g != POISON).reshape(-1)
                if bool(bad.any()):
                    k = int(bad.nonzero()[0])
                    fails.append(f"{a}: {side} guard damaged, first damaged byte {a.where(side, k)} ({int(bad.sum())} of {bad.numel()} guard bytes changed)")
            if a.saved is not None and not torch.equal(a.interior(), a.saved):
                k = int((a.interior() != a.saved).reshape(-1).nonzero()[0])   # (strided: counted over the rows' own bytes, gaps left out)
                fails.append(f"{a}: the kernel modified an input it does not own, first at byte {k}")
        new = self.arenas[self._counted:]
        self._counted = len(self.arenas)
        TOTALS["arenas"] += len(new)
        TOTALS["largest_guard"] = max([TOTALS["largest_guard"]] + [a.guard for a in new])
        print(f"EXTENTGUARD arenas={len(self.arenas)} new={len(new)} largest_guard={max([a.guard for a in self.arenas] or [0])} damaged={len(fails)}")
        assert not fails, "guard verification:\n  " + "\n  ".join(fails[:8])


def _drop_cached_workspaces(ops):
    ws = getattr(getattr(ops, "_SPLITK_WS", None), "ws", None)
    if ws:
        ws.clear()


@contextlib.contextmanager
def guarded(ops):
    """Rebinds ops.torch to the proxy for the duration (restored in `finally`). Re-entrant: an inner `with` joins the outer context. Refuses to
    be entered while a stream is capturing (a graph's private pool is no place for arenas, and verify() synchronises)."""
    global _ACTIVE
    if _ACTIVE is not None:
        if _ACTIVE.ops is not ops:
            raise RuntimeError("guarded(): already active for another module")
        yield _ACTIVE
        return
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("guarded() must not be entered while a stream is capturing")
    session = Session(ops)
    saved = ops.torch
    _drop_cached_workspaces(ops)
    ops.torch = session.proxy
    _ACTIVE = session
    TOTALS["contexts"] += 1
    try:
        yield session
    finally:
        ops.torch = saved
        _ACTIVE = None
        _drop_cached_workspaces(ops)


@contextlib.contextmanager
def plain(ops):
    """Inside guarded(ops): the enclosed ops.* calls allocate as outside it (for a second run whose bits the guarded run must equal)."""
    proxy, ops.torch = ops.torch, torch
    try:
        yield
    finally:
        ops.torch = proxy


def active():
    return _ACTIVE


def _need_active(what):
    if _ACTIVE is None:
        raise RuntimeError(f"{what} outside guarded(ops)")
    return _ACTIVE


def embed(inputs, device="cuda", layout=None):
    """to_device with arenas: every tensor of a case's inputs copied into an arena of its own on `device`; views made later stay views of it.
    layout: operand name -> (skew bytes, ld elements or None) for the operands that are to sit off the allocator's alignment / in padded rows."""
    s = _need_active("embed()")
    lay = lambda k: dict(zip(("skew", "ld"), (layout or {}).get(k, (0, None))))   # noqa: E731
    return inputs.__class__({k: (s.put(v, device, label=f"input {k}", **lay(k)) if torch.is_tensor(v) else v) for k, v in inputs.items()})


def put(t, device="cuda", label="input", skew=0, ld=None):
    """One tensor into an arena on `device`, held unchanged by verify(); outside a guarded context: t.to(device) (no skew / ld there)."""
    if _ACTIVE is None and (skew or ld is not None):
        raise RuntimeError("put(skew= / ld=) outside guarded(ops)")
    return _ACTIVE.put(t, device, label=label, skew=skew, ld=ld) if _ACTIVE is not None else t.to(device)


def scratch(t, label="scratch", skew=0, ld=None):
    """A copy of t that the entry point under test is DECLARED to write (vk_sampler_prepare with `replace`, vk_sampler_update's x, the `partial`
    of vk_groupnorm_finalize_partials, out == in of the stroke overlay): guards checked, contents not held. Outside a context: t.clone()."""
    if _ACTIVE is None and (skew or ld is not None):
        raise RuntimeError("scratch(skew= / ld=) outside guarded(ops)")
    return _ACTIVE.put(t, t.device, writable=True, label=label, skew=skew, ld=ld) if _ACTIVE is not None else t.clone()


def empty(shape, dtype, device="cuda", skew=0, ld=None, label="out"):
    """A poisoned output tensor at `skew` bytes past the aligned start with rows `ld` elements apart, for an ops.* call's out= argument."""
    return _need_active("empty()").empty(shape, dtype, device, skew, ld, label)


def rehome_pack(pw):
    """A weight pack whose operands did not all come from the factories (pack_ff_out's operand and bias, the colsum of a LayerNorm fold):
    every tensor of it that lies outside the arenas is copied into one, in place. Packs are read-only to every kernel, so verify() holds them
    unchanged. Outside a guarded context: the pack as it is."""
    if _ACTIVE is None:
        return pw
    for name in ("wt", "bias", "colsum", "scale"):
        t = getattr(pw, name, None)
        if torch.is_tensor(t) and not _ACTIVE.owns(t):
            setattr(pw, name, _ACTIVE.put(t, t.device, label=f"pack.{name}"))
    return pw


def verify():
    _need_active("verify()").verify()
