"""Times the motion stage of `evaluate` (VISTA_EVAL_MOTION=1) on one MI355X at full size: the 2 x 91 frames of one evaluated 4-round rollout
scene at 576 x 1024, predicted and real. motion.clip_motion over both stacks (wall clock, its copies to the host included) beside
fidelity.frame_metrics over the same bytes in the same process, then the stage split per kernel with device events: vk_flow_luma_pyramid_u8 and
vk_block_flow_u8 per stack, vk_flow_pair_sums for the predicted field against the real one. Every figure is ONE run after one warm-up: the
spread is not measured. Nothing is asserted. profiles/motion_time.txt holds one such run.
    python tools/motion_time.py [--out profiles/motion_time.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vista_amd import fidelity, motion, ops  # noqa: E402
from tools.mjpeg_time import H, W, device_ms, frames_u8, wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "motion_time.txt"))
    opt = ap.parse_args()
    n = 91
    real = frames_u8(n)
    pred = torch.roll(real, shifts=(2, -3), dims=(1, 2)).contiguous()   # the same scene, displaced: two flow fields that differ
    one = lambda ms: f"{ms[0]:9.3f} ms"   # noqa: E731
    t_stage = wall_ms(lambda: motion.clip_motion(pred, real), 1)
    t_fid = wall_ms(lambda: fidelity.frame_metrics(pred, real), 1)
    t_pyr = device_ms(lambda: ops.flow_luma_pyramid_u8(pred), 1)
    pyr_p, pyr_r = ops.flow_luma_pyramid_u8(pred), ops.flow_luma_pyramid_u8(real)
    t_flow = device_ms(lambda: ops.block_flow_u8(pyr_p, n, H, W), 1)
    (flow_p, sad_p), (flow_r, _sad_r) = ops.block_flow_u8(pyr_p, n, H, W), ops.block_flow_u8(pyr_r, n, H, W)
    t_sums = device_ms(lambda: ops.flow_pair_sums(flow_p, sad_p, flow_r), 1)
    rep = motion.clip_motion(pred, real)
    blocks = (n - 1) * (H // 8) * (W // 8)
    lines = [f"Motion stage of evaluate, {torch.cuda.get_device_name(0)}, 2 x {n} frames of {H} x {W} (one 4-round rollout scene, predicted and real): "
             "tools/motion_time.py",
             "one run after one warm-up, spread not measured; stages: wall clock with the copies to the host; kernels: device events around one call", "",
             "stages, both stacks",
             f"  motion.clip_motion                      {one(t_stage)}",
             f"  fidelity.frame_metrics                  {one(t_fid)}", "",
             f"kernels, one stack of {n} frames ({n - 1} pairs, {blocks} blocks)",
             f"  flow_luma_pyramid_u8                    {one(t_pyr)}",
             f"  block_flow_u8                           {one(t_flow)}   ({blocks / (t_flow[0] * 1e-3) / 1e6:.1f} x 10^6 blocks per second)",
             f"  flow_pair_sums, two fields              {one(t_sums)}", "",
             f"the scores of frame 1: flow_rms {rep.rms[1]:.4f}, flow_rms_real {rep.rms_real[1]:.4f}, flow_epe {rep.epe[1]:.4f}, "
             f"warp_err {rep.warp_err[1]:.4f}, diff {rep.diff[1]:.4f}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
