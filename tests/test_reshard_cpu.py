"""Exchange packing as strided boxes (vista_amd/parallel.py, csrc/reshard.hip), the parts a CPU can check: every box plan of FrameShard is
exactly the index tensor the torch path uses, the ctypes mirrors follow the header, and the multi-rank CLI refuses a bad size before it
touches torch.distributed."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (9216, 2304, 576, 144, 12, 5)
CPU = torch.device("cpu")


class _Rank:
    """A communicator that only says who it is (plans are pure functions of T, B, P, rank and S)."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world


def _shards():
    from vista_amd.parallel import FrameShard
    for T, B, P in itertools.product((5, 25), (1, 2), range(1, 9)):
        if P > T:
            continue   # (FrameShard refuses more ranks than frames)
        for r in range(P):
            yield FrameShard(T, _Rank(r, P), B=B)


def _gather_index(boxes, n_out):
    """The index tensor `out = in[index]` a box plan stands for; every output row must be written exactly once."""
    from tests._reshard_ref import expand_boxes
    src, dst = expand_boxes(boxes)
    assert dst.numel() == n_out and torch.equal(dst.sort().values, torch.arange(n_out)), "destination rows repeat or leave holes"
    index = torch.empty(n_out, dtype=torch.int64)
    index[dst] = src
    return index


def test_box_plans_expand_to_the_index_tensors():
    n_plans = 0
    for sh in _shards():
        for S in SIZES:
            pl = sh._plan(S, CPU)
            assert not any(name in pl.keys() for name in ("pack_fp", "unpack_fp", "pack_pf", "unpack_pf")), "index tensors are built on first use"
            n_fp, n_pf = sh.B * sh.t_local * S, sh.B * sh.T * pl["s_r"]
            for name, n_out in (("pack_fp", n_fp), ("unpack_fp", n_pf), ("pack_pf", n_pf), ("unpack_pf", n_fp)):
                assert len(pl["boxes"][name]) == sh.P <= 32
                # what the HIP path reads instead of the index tensor: the row count and "is the identity", both from the boxes alone
                assert pl["rows"][name] == n_out and pl["identity"][name] == (pl[name] is None), (sh.T, sh.B, sh.P, sh.rank, S, name)
                want = torch.arange(n_out) if pl[name] is None else pl[name]
                assert torch.equal(_gather_index(pl["boxes"][name], n_out), want), (sh.T, sh.B, sh.P, sh.rank, S, name)
                n_plans += 1
    assert n_plans == 4 * 6 * sum(P for T in (5, 25) for B in (1, 2) for P in range(1, 9) if P <= T)


@pytest.mark.parametrize("chunks", [1, 3])
def test_chunk_box_plans_expand_to_the_index_tensors(chunks):
    from tests._reshard_ref import expand_boxes
    for sh in _shards():
        for S in SIZES:
            for c in range(chunks):
                pl = sh._chunk_plan(S, chunks, c, CPU)
                assert "pack" not in pl.keys() and "dest" not in pl.keys() and not pl["identity"]["pack"]
                where = (sh.T, sh.B, sh.P, sh.rank, S, chunks, c)
                assert torch.equal(_gather_index(pl["boxes"]["pack"], pl["pack"].numel()), pl["pack"]), where
                # the way back is a scatter: received row j goes to row dest[j] of the frame-sharded result
                src, dst = expand_boxes(pl["boxes"]["dest"])
                assert torch.equal(src, torch.arange(pl["dest"].numel())) and torch.equal(dst, pl["dest"]), where
                assert dst.unique().numel() == dst.numel(), "destination rows of one plan never repeat"
                assert sum(pl["out_rows"]) == dst.numel() and sum(pl["in_rows"]) == pl["pack"].numel()
                assert pl["rows"]["pack"] == pl["pack"].numel() and pl["rows"]["dest"] == pl["dest"].numel()


def test_halo_and_local_row_plans():
    from tests._reshard_ref import expand_boxes
    for sh in _shards():
        src, dst = expand_boxes(sh.local_rows_boxes())
        assert src.tolist() == sh.local_image_ids() and torch.equal(dst, torch.arange(sh.B * sh.t_local))
        S, B, t_l = 12, sh.B, sh.t_local
        rows = torch.arange(B * t_l * S).view(B, t_l, S)
        parts = ([rows[:, 0].reshape(-1)] if sh.rank > 0 else []) + ([rows[:, t_l - 1].reshape(-1)] if sh.rank < sh.P - 1 else [])
        src, dst = expand_boxes(sh.halo_boxes(S))
        assert len(sh.halo_boxes(S)) == len(parts) <= 2
        assert torch.equal(src, torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64)) and torch.equal(dst, torch.arange(src.numel()))


def test_zero_pixel_slices_give_zero_size_boxes():
    from vista_amd.parallel import FrameShard
    seen = 0
    for r in range(8):
        sh = FrameShard(25, _Rank(r, 8), B=2)
        pl = sh._plan(5, CPU)
        assert pl["sc"] == [1, 1, 1, 1, 1, 0, 0, 0]
        for q in range(8):
            empty = pl["sc"][q] == 0
            for name in ("pack_fp", "unpack_pf"):   # the frame-sharded side cuts by the PEER's slice
                assert (pl["boxes"][name][q][6:] == (0, 0, 0)) == empty, (r, q, name)
            seen += empty
        mine_empty = pl["s_r"] == 0
        for name in ("unpack_fp", "pack_pf"):       # the pixel-sharded side by this rank's own
            assert all((b[6:] == (0, 0, 0)) == mine_empty for b in pl["boxes"][name]), (r, name)
        cp = sh._chunk_plan(5, 3, 2, CPU)
        assert all(b[8] == 0 for b in cp["boxes"]["pack"]) == (cp["n_c"] == 0)
    assert seen == 8 * 3


def _struct_fields(hdr, name):
    start = hdr.index("typedef struct %s {" % name) + len("typedef struct %s {" % name)
    body = re.sub(r"/\*.*?\*/", "", hdr[start:hdr.index("} %s;" % name)], flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?(void|float|int32_t|int64_t|VkRowBox)\s*\*?", "", decl.strip()).strip()
        if decl:
            names += [n.strip().lstrip("*").split("[")[0] for n in decl.split(",")]
    return names


def test_row_box_layout_matches_header():
    """Field order of the ctypes mirrors must follow the C structs (a silent mismatch would send the kernel a scrambled plan)."""
    import ctypes
    from vista_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    assert _struct_fields(hdr, "VkRowBox") == [f[0] for f in _lib.VkRowBox._fields_]
    assert _struct_fields(hdr, "VkRowBoxes") == [f[0] for f in _lib.VkRowBoxes._fields_]
    assert int(re.search(r"#define VK_RESHARD_MAX_BOXES (\d+)", hdr).group(1)) == _lib.VK_RESHARD_MAX_BOXES == 32
    assert ctypes.sizeof(_lib.VkRowBox) == 64 and ctypes.sizeof(_lib.VkRowBoxes) == 8 + 32 * 64
    assert _lib.ABI_VERSION == 9 and "vk_copy_row_boxes" in _lib.SIGNATURES


def test_row_boxes_builds_the_struct():
    from vista_amd import ops
    rb = ops.row_boxes([(1, 2, 3, 4, 5, 6, 7, 8, 9), (0, 0, 0, 0, 0, 0, 0, 0, 0)])
    b = rb.box[0]
    assert rb.n == 2 and (b.src_row, b.dst_row, b.src_stride_b, b.src_stride_t, b.dst_stride_b, b.dst_stride_t, b.nb, b.nt, b.ns) == tuple(range(1, 10))
    assert ops.row_boxes([]).n == 0 and ops.row_boxes([(0,) * 9] * 33).n == 33
    with pytest.raises(ValueError):
        ops.row_boxes([(1, 2, 3)])


def test_multi_rank_cli_refuses_a_bad_size_before_torch_distributed(monkeypatch):
    import torch.distributed as dist
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(dist, "init_process_group", lambda *a, **k: pytest.fail("the process group must not be created for a refused size"))
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused size"))
    with pytest.raises(ValueError, match="attention level"):
        sample.main(["--height", "576", "--width", "1088"])
    # a frame-shard group larger than the window is refused by name, again before the rendezvous
    monkeypatch.setenv("WORLD_SIZE", "8")
    monkeypatch.setenv("VISTA_SHARD", "frames")
    with pytest.raises(ValueError, match="WORLD_SIZE 8 .*--n_frames is 5"):
        sample.main(["--n_frames", "5", "--height", "128", "--width", "256"])
