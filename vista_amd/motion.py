"""Motion scores of predicted frames: block-matching optical flow on the bytes of the saved pictures.

A driving world model is scored on how its frames move. A learned flow network is in no Vista checkpoint, so the flow here is hierarchical
block matching on 8-bit luma (csrc/flow.hip; the definition is in include/vista_hip.h): 8 x 8 blocks, three pyramid levels, a coarse search
of [-7, 7]^2 and refinements of [-2, 2]^2, whole pixels only, at most 30 px per frame step. Integer arithmetic from the bytes to the sums: the
same bytes give the same bits, online, from the saved pictures, and in a plain numpy restatement. Per frame i (the pair i - 1 -> i; entry 0 has
no predecessor and is NaN):

  rms        sqrt(sum |v|^2 / blocks): how far the frame's blocks moved, in pixels
  moving     the share of blocks with a non-zero vector ("dynamic degree")
  warp_err   sum SAD / (H W): the mean absolute luma residual after motion compensation, in 8-bit levels
  diff       sum SAD at zero / (H W): the mean absolute luma difference of the two frames, in 8-bit levels
  epe        with a real stack: sqrt(sum |v_pred - v_real|^2 / blocks), the end-point error of the predicted flow against the real clip's

What these numbers are not: the vectors are the best whole-pixel block match, not a learned or a regularised flow; a flat block has the vector
zero whatever moved; nothing handles occlusion; a motion beyond 30 px a step saturates (README "Motion scores"). The arithmetic from the sums
to the scores is float64 on the host.
"""
from dataclasses import dataclass

import numpy as np

from . import ops

BLOCK, LEVELS, COARSE_RANGE, REFINE_RANGE = ops.FLOW_BLOCK, ops.FLOW_LEVELS, ops.FLOW_COARSE_RANGE, ops.FLOW_REFINE_RANGE
REACH_PX = (COARSE_RANGE << (LEVELS - 1)) + REFINE_RANGE   # 30: translations up to here are recovered exactly


def motion_info():
    return {"block": BLOCK, "levels": LEVELS, "coarse_range": COARSE_RANGE, "refine_range": REFINE_RANGE, "reach_px": REACH_PX}


@dataclass
class MotionReport:
    rms: np.ndarray                  # (n,) float64, entry 0 NaN
    moving: np.ndarray
    warp_err: np.ndarray
    diff: np.ndarray
    rms_real: np.ndarray = None      # the same of the real stack, where one was given
    moving_real: np.ndarray = None
    warp_err_real: np.ndarray = None
    diff_real: np.ndarray = None
    epe: np.ndarray = None


def check_size(H, W, what="block_flow"):
    """Refuses, by name, frame sides the flow does not take (ops.flow_check_shape: the kernels' own rule, asked before any launch)."""
    ops.flow_check_shape(what, 1, H, W)


def _stack_shape(frames_u8, what):
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        raise ValueError(f"{what}: expected an (n, H, W, 3) uint8 stack of at least one frame, got {tuple(frames_u8.shape)}")
    return frames_u8.shape[:3]


def block_flow(frames_u8):
    """frames_u8 (n, H, W, 3) uint8 on the GPU, H and W multiples of 32 -> (flow (n - 1, H/8, W/8, 2) int16, sad (n - 1, H/8, W/8, 2) uint16),
    on the GPU: per pair of consecutive frames and block the vector (vy, vx), its SAD and the SAD at zero. One frame: empty, no launch."""
    import torch
    n, H, W = _stack_shape(frames_u8, "block_flow")
    ops.flow_check_shape("block_flow", n, H, W)
    if n == 1:
        ops._need(frames_u8, torch.uint8, "frames_u8")
        return (torch.empty((0, H // BLOCK, W // BLOCK, 2), dtype=torch.int16, device=frames_u8.device),
                torch.empty((0, H // BLOCK, W // BLOCK, 2), dtype=torch.uint16, device=frames_u8.device))
    return ops.block_flow_u8(ops.flow_luma_pyramid_u8(frames_u8.contiguous()), n, H, W)


def _columns(sums, n, H, W):
    """(n - 1, 5) int64 sums -> the four per-frame lists (and the fifth column's), entry 0 NaN."""
    sums = np.asarray(sums, dtype=np.int64).reshape(-1, 5)
    if sums.shape[0] != n - 1:
        raise ValueError(f"report_from_sums: {sums.shape[0]} pairs of sums for {n} frames")
    blocks = (H // BLOCK) * (W // BLOCK)
    lead = np.full((1,), np.nan)
    col = lambda v: np.concatenate([lead, v])   # noqa: E731
    s = sums.astype(np.float64)
    return (col(np.sqrt(s[:, 1] / blocks)), col(s[:, 0] / blocks), col(s[:, 2] / float(H * W)), col(s[:, 3] / float(H * W)),
            col(np.sqrt(s[:, 4] / blocks)))


def report_from_sums(pred_sums, H, W, real_sums=None):
    """(n - 1, 5) int64 pair sums of ops.flow_pair_sums for (H, W) frames (the predicted field's, its fifth column against the real field
    where real_sums is given) -> MotionReport over n frames, in float64 on the host."""
    n = np.asarray(pred_sums).reshape(-1, 5).shape[0] + 1
    rms, moving, warp, diff, epe = _columns(pred_sums, n, H, W)
    report = MotionReport(rms=rms, moving=moving, warp_err=warp, diff=diff)
    if real_sums is not None:
        report.rms_real, report.moving_real, report.warp_err_real, report.diff_real, _ = _columns(real_sums, n, H, W)
        report.epe = epe
    return report


def clip_motion(pred_u8, real_u8=None):
    """pred_u8 (and real_u8, of the same shape) (n, H, W, 3) uint8 on the GPU -> MotionReport: per frame the motion scores of the step from
    its predecessor; with real_u8 the real stack's too and the end-point error between the two flow fields."""
    n, H, W = _stack_shape(pred_u8, "clip_motion")
    if real_u8 is not None and real_u8.shape != pred_u8.shape:
        raise ValueError(f"clip_motion: pred has {tuple(pred_u8.shape)} bytes, real {tuple(real_u8.shape)}: the stacks must pair up frame by frame")
    flow_p, sad_p = block_flow(pred_u8)
    if real_u8 is None:
        sums = ops.flow_pair_sums(flow_p, sad_p).cpu().numpy() if n > 1 else np.zeros((0, 5), np.int64)
        return report_from_sums(sums, H, W)
    flow_r, sad_r = block_flow(real_u8)
    if n == 1:
        return report_from_sums(np.zeros((0, 5), np.int64), H, W, np.zeros((0, 5), np.int64))
    sums_p, sums_r = ops.flow_pair_sums(flow_p, sad_p, flow_r), ops.flow_pair_sums(flow_r, sad_r)
    return report_from_sums(sums_p.cpu().numpy(), H, W, sums_r.cpu().numpy())   # (the copies to the host end the stage)


class RunScores:
    """The motion side of an evaluation run (the counterpart of perceptual.RunScores; it keeps nothing between scenes)."""

    def scene(self, pred_u8, real_u8):
        """Two (n, H, W, 3) uint8 stacks -> the scene's MotionReport over all frames (which of them are conditioning frames is the record's
        business: a first predicted frame steps from the last conditioning frame)."""
        return clip_motion(pred_u8, real_u8)

    def summary(self):
        """-> the `motion=` argument of evaluate.summarize."""
        return motion_info()
