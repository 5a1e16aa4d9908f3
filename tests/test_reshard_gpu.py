"""vk_copy_row_boxes (csrc/reshard.hip) and the exchange packing of FrameShard built on it, on the MI355X. Every check is bitwise: the kernel
copies rows, so it is compared with torch's gather / scatter of the same rows and with the torch path of parallel.py (HIP_RESHARD off)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = 0x5A


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _torch_copy(src, dst, boxes):
    from tests._reshard_ref import expand_boxes
    s, d = expand_boxes(boxes)
    want = dst.clone()
    want[d.to(dst.device)] = src[s.to(src.device)]
    return want


def _random_rows(rows, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (rows, C * torch.empty(0, dtype=dtype).element_size()), generator=g, dtype=torch.uint8).cuda().view(dtype)


def _check(src, dst_rows, boxes):
    from vista_amd import ops
    dst = torch.full((dst_rows, src.shape[1]), 0, dtype=src.dtype, device="cuda")
    _bits(dst).fill_(SENTINEL)
    want = _torch_copy(src, dst, boxes)
    got = ops.copy_row_boxes(src, dst, boxes)
    assert got is dst and torch.equal(_bits(dst), _bits(want))
    return dst


# (src_row, dst_row, src_stride_b, src_stride_t, dst_stride_b, dst_stride_t, nb, nt, ns): a (2, 3, 5) box out of a (2, 4, 7) array into a dense one
BOX = (7 + 1, 3, 28, 7, 15, 5, 2, 3, 5)


@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 8), (torch.bfloat16, 320), (torch.bfloat16, 1280), (torch.float32, 4), (torch.float32, 40),
                                     (torch.float16, 64)], ids=["16B", "640B", "2560B", "f32_16B", "f32_160B", "f16_128B"])
def test_copy_row_boxes_equals_torch_bitwise(dtype, C):
    src = _random_rows(61, C, dtype, seed=C)
    dst = _check(src, 40, [BOX])                           # dst has 40 rows, the box writes rows 3 .. 32: the rest keeps the sentinel
    assert (_bits(dst[:3]) == SENTINEL).all() and (_bits(dst[33:]) == SENTINEL).all()
    _check(src, 61, [(60, 0, -1, 0, 1, 0, 61, 1, 1)])      # ns = 1, a negative stride: the rows in reverse order
    _check(src, 9, [(5, 2, 0, 0, 3, 1, 2, 3, 1)])          # stride 0 on the source: one row broadcast to six


def test_copy_row_boxes_many_boxes_empty_boxes_and_more_than_one_block():
    from vista_amd import ops
    src = _random_rows(4096, 320, torch.bfloat16, seed=1)  # 2.6 MB: 160 blocks of 256 threads x 4 units
    boxes = [(128 * k + (k % 5), 100 * (31 - k), 40, 10, 50, 10, 2, 5, 7 + (k % 3)) for k in range(32)]   # 32 boxes, destinations in reverse order
    _check(src, 3200, boxes)
    some = list(boxes)
    for k in (0, 7, 8, 31):                                 # empty boxes first, in the middle, last
        some[k] = (0, 0, 0, 0, 0, 0, 0, 0, 0)
    some[3] = (10 ** 12, -5, 1, 1, 1, 1, 4, 0, 4)           # an empty box is skipped whatever its rows say
    dst = _check(src, 3200, some)
    assert (_bits(dst[100 * 31:100 * 31 + 100]) == SENTINEL).all()
    dst = _check(src, 16, [(0, 0, 0, 0, 0, 0, 0, 0, 0)] * 3)   # nothing but empty boxes: VK_OK, no launch
    assert (_bits(dst) == SENTINEL).all()
    big = _random_rows(20000, 1280, torch.bfloat16, seed=2)    # 51 MB: more units than the capped grid has threads x 4 (grid-stride loop)
    _check(big, 20000, [(0, 10000, 2, 1, 2, 1, 5000, 2, 1), (10000, 0, 1000, 0, 1000, 0, 10, 1, 1000)])
    with pytest.raises(ValueError):
        ops.copy_row_boxes(src, src.float(), [BOX])
    with pytest.raises(ValueError):
        ops.copy_row_boxes(src, src[:, :8].contiguous(), [BOX])
    with pytest.raises(ValueError):
        ops.copy_row_boxes(src[:, :8], src[:, :8].contiguous(), [BOX])      # rows that are not dense


def test_copy_row_boxes_refusals_leave_dst_intact():
    from vista_amd import _lib, ops
    src = _random_rows(61, 8, torch.bfloat16, seed=3)
    dst = torch.empty((40, 8), dtype=torch.bfloat16, device="cuda")
    _bits(dst).fill_(SENTINEL)

    def refused(s, d, boxes):
        with pytest.raises(_lib.VistaHipError, match="-22"):
            ops.copy_row_boxes(s, d, boxes)
        torch.cuda.synchronize()
        assert (_bits(d) == SENTINEL).all() and (_bits(dst) == SENTINEL).all()     # the tensor that was passed, and the one it may be a view of
    refused(src[:, :4].contiguous(), dst[:, :4].contiguous(), [(0, 0, 0, 0, 0, 0, 1, 1, 1)])          # row_bytes = 8 (a sentinel-filled copy of dst)
    flat = torch.zeros(62 * 8, dtype=torch.bfloat16, device="cuda")
    refused(flat[4:4 + 61 * 8].view(61, 8), dst, [BOX])                                                 # src 8 bytes off a 16-byte boundary
    refused(src, dst.view(-1)[4:4 + 39 * 8].view(39, 8), [(0, 0, 0, 0, 0, 0, 1, 1, 1)])                 # dst misaligned
    refused(src, dst, [])                                                                               # n = 0
    refused(src, dst, [(0, k, 0, 0, 0, 0, 1, 1, 1) for k in range(33)])                                 # n = 33
    for neg in ((0, 0, 1, 1, 1, 1, -1, 1, 1), (0, 0, 1, 1, 1, 1, 1, -1, 1), (0, 0, 1, 1, 1, 1, 1, 1, -1)):
        refused(src, dst, [neg])                                                                        # a negative extent
    refused(src, dst, [(61 - 5 + 1, 0, 0, 0, 0, 0, 1, 1, 5)])                                           # last source row = src_rows
    refused(src, dst, [(0, 40 - 5 + 1, 0, 0, 0, 0, 1, 1, 5)])                                           # last destination row = dst_rows
    refused(src, dst, [(0, 0, 8, 1, 5, 1, 8, 1, 6)])                                                    # only the last run (b = 7) leaves: rows 56 .. 61 / 35 .. 40
    refused(src, dst, [(0, 0, 0, 0, 0, 0, 1, 1, 1), (-1, 0, 0, 0, 0, 0, 1, 1, 1)])                      # a negative row, second box: nothing of the first is copied
    refused(src, dst, [(3, 3, -1, 0, -1, 0, 5, 1, 1)])                                                  # a negative stride that leaves at the front
    ops.copy_row_boxes(src, dst, [(61 - 5, 40 - 5, 0, 0, 0, 0, 1, 1, 5)])                               # the last legal position
    assert torch.equal(_bits(dst[35:]), _bits(src[56:])) and (_bits(dst[:35]) == SENTINEL).all()


def test_the_plan_travels_by_value_through_a_captured_graph():
    from vista_amd import ops
    src = _random_rows(61, 64, torch.bfloat16, seed=4)
    dst = torch.zeros((40, 64), dtype=torch.bfloat16, device="cuda")
    plan = ops.row_boxes([BOX])
    ops.copy_row_boxes(src, dst, plan)       # (warm: the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.copy_row_boxes(src, dst, plan)
    plan.box[0].src_row, plan.box[0].dst_row, plan.box[0].ns, plan.n = 0, 0, 1, 1     # the host plan now says something else ...
    new_src = _random_rows(61, 64, torch.bfloat16, seed=5)
    src.copy_(new_src)                                                                   # ... and so does the source
    _bits(dst).fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    want = torch.empty_like(dst)
    _bits(want).fill_(SENTINEL)
    assert torch.equal(_bits(dst), _bits(_torch_copy(new_src, want, [BOX]))), "the replay copies the new src by the plan of the capture"
    del graph


# ---- FrameShard over thread ranks: HIP packing against the torch path ------------------------------------------------------------------
def _ops_of_a_rank(sh, T, S, C, B, seed):
    """Every packing entry point of one rank on deterministic data -> list of result tensors."""
    g = torch.Generator().manual_seed(seed * 100 + sh.rank)
    x = torch.randn(B * sh.t_local, S, C, generator=g).to(torch.bfloat16).cuda()
    xp = sh.to_pixels(x)
    back = sh.to_frames(xp, S)
    out = [xp, back]
    nch = 2   # every rank cuts its slice in two, also a rank whose slice has one pixel ((5, 5, 8) at P = 3): its second sub-range is empty
    if nch >= 1:
        chunked = torch.zeros_like(x)
        pend = [sh.to_frames_begin(xp[:, lo:hi].contiguous(), S, nch, ci) for ci, (lo, hi) in enumerate(sh.pixel_chunks(S, nch))]
        for p in pend:
            sh.to_frames_end(p, chunked)
        out.append(chunked)
    prev, nxt = sh.halo_exchange(x)
    out += [t if t is not None else torch.zeros(1) for t in (prev, nxt)]
    full = torch.randn(B * T, C, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).cuda()
    out += [sh.take_local_rows(full), sh.take_local_rows(full.float().view(B * T, 2, C // 2))]
    assert torch.equal(back, x), "to_frames(to_pixels(x)) is the identity"
    if nch >= 1:
        assert torch.equal(chunked, x), "the chunked way back is the identity too"
    assert torch.equal(out[-2], full[torch.tensor(sh.local_image_ids(), device="cuda")])
    return out


# P = 8 needs 25 frames (FrameShard refuses more ranks than frames); (5, 5, 8) is the shape with unequal, tiny pixel slices, at P = 3
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("P,T,S,C", [(2, 5, 12, 8), (3, 5, 12, 8), (2, 25, 144, 64), (3, 25, 144, 64), (8, 25, 144, 64), (3, 5, 5, 8)])
def test_frame_shard_packing_hip_equals_torch_bitwise(P, T, S, C, B, monkeypatch):
    from tests.test_parallel_gpu import run_ranks
    from vista_amd import ops, parallel
    from vista_amd.parallel import FrameShard
    calls = []
    real = ops.copy_row_boxes
    monkeypatch.setattr(ops, "copy_row_boxes", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = {}
    for on in (True, False):
        monkeypatch.setattr(parallel, "HIP_RESHARD", on)
        n0 = len(calls)
        res[on] = run_ranks(P, lambda comm: _ops_of_a_rank(FrameShard(T, comm, B=B), T, S, C, B, seed=P + S))
        assert (len(calls) > n0) == on, "the switch selects the path"
    for r in range(P):
        assert len(res[True][r]) == len(res[False][r])
        for i, (a, b) in enumerate(zip(res[True][r], res[False][r])):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (r, i)


def test_odd_row_widths_keep_the_torch_path(monkeypatch):
    from tests.test_parallel_gpu import run_ranks
    from vista_amd import ops
    from vista_amd.parallel import FrameShard
    monkeypatch.setattr(ops, "copy_row_boxes", lambda *a, **k: pytest.fail("a 12-byte row is not the kernel's"))

    def rank_fn(comm):
        sh = FrameShard(5, comm, B=2)
        x = torch.randn(2 * sh.t_local, 12, 6).to(torch.bfloat16).cuda()       # 6 bf16 channels = 12 bytes per row
        assert torch.equal(sh.to_frames(sh.to_pixels(x), 12), x)
        sh.halo_exchange(x)
        return sh.take_local_rows(torch.zeros(10, 6, device="cuda")).shape[0] == 2 * sh.t_local
    assert all(run_ranks(2, rank_fn))


@pytest.mark.parametrize("chunks", [1, 3])
def test_sharded_unet_forward_is_the_same_with_hip_and_torch_packing(chunks, monkeypatch):
    """The tiny-UNet sharded forward of test_parallel_gpu at P = 3: every re-shard, halo and row selection through the kernel or through torch."""
    monkeypatch.setenv("VISTA_A2A_CHUNKS", str(chunks))
    from oracle.make_golden import unet_inputs
    from tests.test_model_gpu import tiny_unet
    from tests.test_parallel_gpu import run_ranks
    from vista_amd import ops, parallel
    from vista_amd.modules.diffusionmodules.video_model import CIN_PAD
    from vista_amd.parallel import FrameShard
    net, _ = tiny_unet()
    g = torch.load(os.path.join(GOLD, "unet_tiny_t5.pt"))
    T, H, W = g["T"], g["H"], g["W"]
    x8, ts, ctx, y, mask = [t.cuda() for t in unet_inputs(T, H, W, seed=g["seed_x"], sigma=g["sigma"])]
    tokens = ops.nchw_to_tokens(x8.float(), CIN_PAD)

    def rank_fn(comm):
        sh = FrameShard(T, comm, B=2)
        assert sh.a2a_chunks == chunks
        return net.forward_tokens(sh.take_local_rows(tokens).contiguous(), ts, ctx, y, mask, T, H, W, shard=sh).clone()
    outs = {}
    for on in (True, False):
        monkeypatch.setattr(parallel, "HIP_RESHARD", on)
        outs[on] = run_ranks(3, rank_fn)
    for a, b in zip(outs[True], outs[False]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
