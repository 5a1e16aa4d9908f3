"""The definition vk_candidate_frame_stats is held to, in float64 torch on the CPU: the unbiased ensemble variance of every candidate's members,
summed per scored frame, the frames added in order, and the selection rule. Shared by tests/test_plan_cpu.py (which also patches it in for
ops.candidate_frame_stats, so that the planner's host side runs without a GPU) and tests/test_plan_gpu.py."""
import torch


def select(totals):
    """The index of the smallest total: ties to the lowest index, a NaN never, -1 if every total is NaN."""
    best = -1
    for k, v in enumerate(totals):
        v = float(v)
        if v != v:
            continue
        if best < 0 or v < float(totals[best]):
            best = k
    return best


def variance(x, t0):
    """x (K, E, T, C, h, w) -> the float64 unbiased variance over the members of the frames [t0, T): (K, T - t0, C, h, w)."""
    return x.detach().cpu().double()[:, :, t0:].var(1, unbiased=True)


def candidate_frame_stats(x, t0, want_map=False):
    """ops.candidate_frame_stats' signature and result layout (on the CPU): (frame_sum (K, T') float64, total (K,) float64, best 0-dim int32,
    map (K, T', h, w) float32 or None)."""
    var = variance(x, t0)
    frame_sum = var.sum(dim=(2, 3, 4))
    total = torch.zeros(var.shape[0], dtype=torch.float64)
    for t in range(var.shape[1]):          # frames in order
        total = total + frame_sum[:, t]
    fmap = var.mean(dim=2).float() if want_map else None
    return frame_sum, total, torch.tensor(select(total.tolist()), dtype=torch.int32), fmap
