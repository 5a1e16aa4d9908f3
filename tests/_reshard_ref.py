"""Reference expansion of a box plan (include/vista_hip.h, VkRowBox) into row indices, shared by the reshard tests."""
import torch


def expand_boxes(boxes):
    """(source rows, destination rows) of a box plan as two int64 tensors, box after box, (b, t, s) order inside a box."""
    ar = torch.arange
    src, dst = [torch.empty(0, dtype=torch.int64)], [torch.empty(0, dtype=torch.int64)]
    for s0, d0, sb, st, db, dt, nb, nt, ns in boxes:
        src.append((s0 + ar(nb)[:, None, None] * sb + ar(nt)[None, :, None] * st + ar(ns)[None, None, :]).reshape(-1))
        dst.append((d0 + ar(nb)[:, None, None] * db + ar(nt)[None, :, None] * dt + ar(ns)[None, None, :]).reshape(-1))
    return torch.cat(src), torch.cat(dst)
