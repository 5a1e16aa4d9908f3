"""Proof, on the CPU, that the guard harness of tests/_guard.py separates right from wrong (the pattern of tests/test_bf16_bounds_cpu.py): plain-torch
stand-ins for a kernel -- out = bf16(1.5 x + 0.25) on a (300, 4) bf16 operand, allocated as ops.py allocates, through its module global `torch`
-- are driven through the very body the GPU modules use (tests/_parity_bodies.py: case_under_tile -> guarded, embed, judge with bound A, verify).
The correct stand-in passes; one that leaves an element unwritten, stores outside its output, loads past its operand into the result or writes an
operand it does not own fails, for that reason, and a damaged guard names the right tensor. A stand-in reaches the bytes around a tensor the way
a kernel does: by address (as_strided on the arena's storage).

Skewed and strided arenas (tests/_guard.py: skew, ld): the same stand-in on an operand 8 bytes past the aligned start in rows of COLS + 2 elements and
an output 8 bytes past it in rows of COLS + 4 passes; one that rounds its first store's address down to 16 bytes is caught in the front skew, one
that stores whole ld-wide rows in a row gap, and a load of a padded operand's gap reaches the result as NaN."""
import re

import pytest
import torch

from tests import _bf16_cases as fc
from tests import _guard
from tests import _parity_bodies as pb

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
ROWS, COLS = 300, 4


@pytest.fixture
def ops():
    from vista_amd import ops
    assert ops.torch is torch
    yield ops
    assert ops.torch is torch, "guarded() left its proxy in ops.torch"


def _past(t, rows):
    """t (ROWS, COLS) seen `rows` further rows past its end: the address arithmetic of a kernel whose row bound is off."""
    return t.as_strided((ROWS + rows, COLS), (COLS, 1), t.storage_offset())


def _byte(t, offset):
    """One byte at `offset` bytes from t's first byte (negative: before it)."""
    flat = torch.empty(0, dtype=U8).set_(t.untyped_storage())
    return flat[t.storage_offset() * t.element_size() + offset:][:1]


SKEW, LD_OUT, LD_IN = 8, COLS + 4, COLS + 2
LAYOUT_KINDS = ("correct_skewed_and_strided", "rounds_its_store_address_down_to_16_bytes", "stores_a_full_ld_wide_row", "loads_a_full_ld_wide_row")


def _standin(kind):
    laid_out = kind in LAYOUT_KINDS

    def run(ops, i):
        aux = ops.torch.empty((7, 64), dtype=F32, device=i.x.device)      # a second, untouched allocation: never the one a failure names
        if laid_out:
            out = _guard.empty((ROWS, COLS), BF16, i.x.device, skew=SKEW, ld=LD_OUT)
            assert out.data_ptr() % 16 == SKEW and out.stride() == (LD_OUT, 1) and i.x.data_ptr() % 16 == SKEW and i.x.stride() == (LD_IN, 1)
        else:
            out = ops.torch.empty((ROWS, COLS), dtype=BF16, device=i.x.device)
        aux.fill_(0.0)
        y = (i.x.float() * 1.5 + 0.25).to(BF16)
        if kind == "rounds_its_store_address_down_to_16_bytes":            # row 0's 8-byte store at (address & ~15): the 8 bytes before the tensor
            out.copy_(y)
            out.as_strided((COLS,), (1,), out.storage_offset() - SKEW // 2).copy_(y[0])
            return [out]
        if kind == "stores_a_full_ld_wide_row":                            # row 5 stored LD_OUT elements wide: its gap is written
            out.copy_(y)
            out.as_strided((LD_OUT,), (1,), out.storage_offset() + 5 * LD_OUT).fill_(0.5)
            out[5] = y[5]
            return [out]
        if kind == "loads_a_full_ld_wide_row":                             # the last column's load one element further: the operand's gap
            wide = i.x.as_strided((ROWS, COLS + 1), (LD_IN, 1), i.x.storage_offset())
            out.copy_((wide[:, 1:].float() * 1.5 + 0.25).to(BF16))
            out[:, :-1] = y[:, :-1]
            return [out]
        if kind == "skips_last_row":
            out[:-1] = y[:-1]
        elif kind == "skips_one_element":
            keep = torch.ones(ROWS * COLS, dtype=torch.bool)
            keep[ROWS * COLS // 2 + 1] = False
            out.view(-1)[keep] = y.view(-1)[keep]
        elif kind == "reads_one_row_past_the_input":
            out.copy_((_past(i.x, 1)[1:].float() * 1.5 + 0.25).to(BF16))
            out[:-1] = y[:-1]                                            # only the last row's load is off by one row
        else:
            out.copy_(y)
        if kind == "writes_one_element_past_the_end":
            _past(out, 1)[ROWS, 0] = 1.0
        elif kind == "writes_one_row_past_the_end":
            _past(out, 1)[ROWS] = 1.0
        elif kind == "writes_one_element_before_the_start":
            _byte(out, -2).fill_(0)
            _byte(out, -1).fill_(0)
        elif kind == "writes_the_last_byte_of_the_back_guard":
            _byte(out, ROWS * COLS * 2 + _guard.guard_bytes((ROWS, COLS), 2) - 1).fill_(0)
        elif kind == "modifies_an_input":
            i.x[17, 2] = 3.0
        return [out]

    def build():
        return fc.I(x=fc.r16(fc.G(77), ROWS, COLS))
    return fc.Case(f"extent_standin_{kind}", build, lambda i: [fc.d(i.x) * 1.5 + 0.25], run, [("A", BF16)], layout={"x": (SKEW, LD_IN)} if laid_out else None)


def _drive(ops, kind):
    pb.case_under_tile(ops, fc, _standin(kind), 0, device="cpu")


OUT = f"torch.empty ({ROWS}, {COLS}) torch.bfloat16"


def test_a_correct_standin_passes(ops):
    before = _guard.TOTALS["arenas"]
    _drive(ops, "correct")
    assert _guard.TOTALS["arenas"] - before == 3   # the operand, the untouched allocation, the output


@pytest.mark.parametrize("kind", ["skips_last_row", "skips_one_element"])
def test_an_unwritten_element_fails(kind, ops):
    with pytest.raises(AssertionError, match="nonfinite"):
        _drive(ops, kind)


@pytest.mark.parametrize("kind,side,where", [
    ("writes_one_element_past_the_end", "back", "0 bytes past its last byte \\(2 of"),
    ("writes_one_row_past_the_end", "back", f"0 bytes past its last byte \\({2 * COLS} of"),
    ("writes_one_element_before_the_start", "front", "2 bytes before its first byte \\(2 of"),
    ("writes_the_last_byte_of_the_back_guard", "back", f"{_guard.guard_bytes((ROWS, COLS), 2) - 1} bytes past its last byte \\(1 of"),
])
def test_a_store_outside_the_output_fails_and_names_it(kind, side, where, ops):
    with pytest.raises(AssertionError) as e:
        _drive(ops, kind)
    msg = str(e.value)
    lines = [ln for ln in msg.splitlines() if "guard damaged" in ln]
    assert len(lines) == 1, msg                              # one tensor, one side: neither the operand nor the other allocation
    assert lines[0].strip().startswith(f"{OUT}: {side} guard damaged") and re.search(where, lines[0]), lines[0]


def test_a_correct_standin_on_skewed_and_strided_operands_passes(ops):
    _drive(ops, "correct_skewed_and_strided")


@pytest.mark.parametrize("kind,side,where", [
    ("rounds_its_store_address_down_to_16_bytes", "front", f"{SKEW} bytes before its first byte \\({SKEW} of"),
    ("stores_a_full_ld_wide_row", "gap", f"0 bytes past the end of row 5 \\({2 * (LD_OUT - COLS)} of"),
])
def test_a_store_into_the_skew_or_a_row_gap_fails_and_names_it(kind, side, where, ops):
    with pytest.raises(AssertionError) as e:
        _drive(ops, kind)
    lines = [ln for ln in str(e.value).splitlines() if "guard damaged" in ln]
    assert len(lines) == 1, str(e.value)
    assert lines[0].strip().startswith(f"out ({ROWS}, {COLS}) torch.bfloat16: {side} guard damaged") and re.search(where, lines[0]), lines[0]


def test_a_load_of_a_row_gap_reaches_the_result_as_nan(ops):
    with pytest.raises(AssertionError, match="nonfinite"):
        _drive(ops, "loads_a_full_ld_wide_row")


def test_a_load_past_the_input_reaches_the_result_as_nan(ops):
    with pytest.raises(AssertionError, match="nonfinite"):
        _drive(ops, "reads_one_row_past_the_input")


def test_a_modified_input_fails(ops):
    with pytest.raises(AssertionError, match=r"input x \(300, 4\) torch.bfloat16: the kernel modified an input it does not own, first at byte " + str((17 * COLS + 2) * 2)):
        _drive(ops, "modifies_an_input")


def test_a_declared_scratch_copy_may_be_written_but_not_overrun(ops):
    with _guard.guarded(ops):
        x = _guard.put(torch.zeros(5, 3), device="cpu")
        s = _guard.scratch(x)
        s += 1.0
        _guard.verify()
        s.as_strided((1,), (1,), s.storage_offset() + 15)[0] = 1.0
        with pytest.raises(AssertionError, match=r"scratch \(5, 3\) torch.float32: back guard damaged"):
            _guard.verify()


class _Recycling:
    """What the caching allocator does to back-to-back variants of one case: `empty` hands out the block the previous call of that size freed,
    contents and all."""

    def __init__(self):
        self.blocks = {}

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        key = (tuple(shape), dtype)
        if key not in self.blocks:
            self.blocks[key] = torch.empty(shape, dtype=dtype, device=device)
        return self.blocks[key]


def test_the_hole_a_recycled_block_hides_a_skipped_store_without_poison(ops):
    """The suite's earlier flow (run on plain allocations, judge): after a correct variant, a variant that skips its last row passes on what its
    predecessor left in the recycled block. Through case_under_tile as it is now the same stand-in fails (test_an_unwritten_element_fails)."""
    good, bad = _standin("correct"), _standin("skips_last_row")
    i, refs = pb.inputs_and_ref(fc, good)
    ops.torch = _Recycling()
    try:
        pb.judge(fc, good, good.run(ops, i), refs, "plain")
        pb.judge(fc, bad, bad.run(ops, i), refs, "plain")      # passes: the hole
    finally:
        ops.torch = torch
    with pytest.raises(AssertionError, match="nonfinite"):
        _drive(ops, "skips_last_row")


# ------------------------------------------------------------------------------------------------ the arena itself
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.float8_e4m3fn, torch.float8_e8m0fnu])
def test_byte_ff_repeated_is_nan(dtype):
    t = torch.full((64,), _guard.POISON, dtype=U8).view(dtype)
    assert t.float().isnan().all()


@pytest.mark.parametrize("shape,dtype,guard", [((300, 4), BF16, 4096), ((7, 5120), BF16, 320 * 10240), ((3, 1001), U8, 320 * 1001 + 192),
                                               ((), torch.int32, 4096), ((1 << 20,), F32, 8 << 20), ((0,), torch.float64, 4096)])
def test_arena_geometry(shape, dtype, guard, ops):
    """Guards of max(4 KiB, 320 rows) rounded up to 256 B and capped at 8 MiB; the interior 256-byte aligned relative to the arena's start, the
    back guard from the first byte after it; an `empty` interior all 0xFF, `zeros` / `ones` / `full` their value."""
    with _guard.guarded(ops) as g:
        e, z, o = (getattr(ops.torch, f)(shape, dtype=dtype) for f in ("empty", "zeros", "ones"))
        f = ops.torch.full(shape, 3, dtype=dtype)
        like = ops.torch.empty_like(e)
        assert [a.guard for a in g.arenas] == [guard] * 5 and guard % 256 == 0
        for a, t in zip(g.arenas, (e, z, o, f, like)):
            assert t.shape == torch.Size(shape) and t.dtype is dtype and t.is_contiguous()
            assert t.storage_offset() * t.element_size() == a.guard and a.base.numel() == 2 * a.guard + t.numel() * t.element_size()
            assert t.untyped_storage().data_ptr() == a.base.data_ptr()
            assert all(bool((s == _guard.POISON).all()) for _, s in a.sides())
        assert bool((g.arenas[0].interior() == _guard.POISON).all()) and bool((g.arenas[4].interior() == _guard.POISON).all())
        assert not z.any() and bool((o == 1).all()) and bool((f == 3).all())
        _guard.verify()


def test_the_proxy_forwards_everything_else_and_is_restored_after_an_exception(ops):
    with pytest.raises(ZeroDivisionError):
        with _guard.guarded(ops) as g:
            assert ops.torch is g.proxy and ops.torch.float16 is torch.float16 and ops.torch.cat is torch.cat and ops.torch.nn is torch.nn
            with _guard.guarded(ops) as inner:    # re-entrant: the inner context joins the outer one
                assert inner is g
            assert ops.torch is g.proxy
            1 / 0
    assert ops.torch is torch and _guard.active() is None
    with pytest.raises(RuntimeError):
        _guard.verify()
    with pytest.raises(RuntimeError):
        _guard.embed(fc.I(x=torch.zeros(2)))


def test_a_context_drops_the_cached_splitk_workspaces(ops):
    ops._SPLITK_WS.ws[("cpu", 0)] = torch.zeros(4)
    try:
        with _guard.guarded(ops):
            assert not ops._SPLITK_WS.ws           # (a workspace from before would carry no guards)
            ops._SPLITK_WS.ws[("cpu", 0)] = ops.torch.empty(4, dtype=F32)
        assert not ops._SPLITK_WS.ws               # (and an arena must not outlive the context that verifies it)
    finally:
        ops._SPLITK_WS.ws.clear()


def test_refuses_to_be_entered_during_stream_capture(ops, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        with _guard.guarded(ops):
            pass
    assert ops.torch is torch


def test_rehome_pack_moves_what_the_factories_did_not_allocate(ops):
    """The colsum of a LayerNorm fold and pack_ff_out's operand are not built by the factories: rehome_pack copies them into arenas, bit for bit."""
    g = fc.G(3)
    w, b = fc.r32(g, 8, 64), fc.r32(g, 8)
    with _guard.guarded(ops) as s:
        pw = ops.pack_linear(w, b, device="cpu", ln=fc.Norm(fc.r32(g, 64, shift=1.0), fc.r32(g, 64)))
        assert s.owns(pw.wt) and s.owns(pw.bias) and not s.owns(pw.colsum)
        colsum = pw.colsum.clone()
        assert _guard.rehome_pack(pw) is pw and s.owns(pw.colsum) and torch.equal(pw.colsum, colsum)
        po = ops.pack_ff_out(fc.r32(g, 320, 128), fc.r32(g, 320), device="cpu")
        assert not s.owns(po.wt) and not s.owns(po.bias)
        wt = po.wt.clone()
        _guard.rehome_pack(po)
        assert s.owns(po.wt) and s.owns(po.bias) and torch.equal(po.wt, wt) and po.wt.dtype is wt.dtype
        _guard.verify()
