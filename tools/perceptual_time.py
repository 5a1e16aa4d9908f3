"""Times the CLIP-space scoring path on one MI355X at full size, on seeded ViT-H/14 weights: the 2 x 91 frames of one evaluated 4-round rollout
scene at 576 x 1024. The preprocessing from bytes (vk_clip_preprocess_patches_u8) beside the fp32 detour it replaces (the conversion of the
bytes to fp32 NCHW frames plus vk_clip_preprocess_patches), same box, same call; the tower over the 182 frames (perceptual.embed_frames, which
includes the preprocessing); vk_embed_row_stats; vk_embed_mmd_sums for one scene (91 x 91 x 1024) and for a run of 50 scenes
(4550 x 4550 x 1024). Device events; every figure is the median of RUNS runs after one warm-up, with the smallest and the largest beside it.
Nothing is asserted. profiles/perceptual_time.txt holds one run.
    python tools/perceptual_time.py [--out profiles/perceptual_time.txt] [--runs 5]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vista_amd import ops, perceptual, synth  # noqa: E402
from tools.mjpeg_time import H, W, device_ms, frames_u8, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "perceptual_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    opt = ap.parse_args()
    from vista_amd.modules.encoders.modules import FrozenOpenCLIPImageEmbedder
    n = 182
    x = frames_u8(n)
    lines = [f"CLIP-space scoring path, {torch.cuda.get_device_name(0)}, {n} frames of {H} x {W} (one 4-round rollout scene, predicted and real), "
             "seeded ViT-H/14 weights: tools/perceptual_time.py", "device events around the calls named; the fp32 detour and the kernel from bytes in the same process", ""]

    def detour():
        with ops.storage(torch.bfloat16):
            return ops.clip_preprocess_patches(x.permute(0, 3, 1, 2).float() / 127.5 - 1.0)

    def from_bytes():
        with ops.storage(torch.bfloat16):
            return ops.clip_preprocess_patches_u8(x)

    def convert_only():
        return (x.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()

    t_u8, t_detour, t_conv = device_ms(from_bytes, opt.runs), device_ms(detour, opt.runs), device_ms(convert_only, opt.runs)
    lines += [f"preprocessing, {n} frames -> {n * 257} x 640 patch operand",
              f"  clip_preprocess_patches_u8 (bytes)                {stats(t_u8)}",
              f"  .float() / 127.5 - 1 + clip_preprocess_patches    {stats(t_detour)}",
              f"    of which the conversion to fp32 NCHW            {stats(t_conv)}", ""]
    tower = FrozenOpenCLIPImageEmbedder()
    tower.load_state_dict(synth.seeded_state_dict({k: tuple(v.shape) for k, v in tower.state_dict().items()}, 5), strict=True)
    tower = tower.cuda().eval()
    t_tower = device_ms(lambda: perceptual.embed_frames(tower, x), opt.runs)
    e = perceptual.embed_frames(tower, x)
    a, b = e[:91].contiguous(), e[91:].contiguous()
    t_stats = device_ms(lambda: ops.embed_row_stats(a, b), opt.runs)
    t_mmd = device_ms(lambda: ops.embed_mmd_sums(a, b, perceptual.SIGMA), opt.runs)
    g = torch.Generator(device="cuda").manual_seed(1)
    big = [(torch.randn(4550, 1024, generator=g, device="cuda") + 3 * torch.randn(1, 1024, generator=g, device="cuda")).contiguous() for _ in range(2)]
    t_big = device_ms(lambda: ops.embed_mmd_sums(big[0], big[1], perceptual.SIGMA), opt.runs)
    pairs = 4550 * 4549 + 4550 * 4550
    lines += [f"tower, embed_frames over {n} frames in chunks of {perceptual.EMBED_CHUNK} (preprocessing included)",
              f"  perceptual.embed_frames                           {stats(t_tower)}", "",
              "scores", f"  embed_row_stats, 91 x 1024                        {stats(t_stats)}",
              f"  embed_mmd_sums, 91 x 91 x 1024 (one scene)        {stats(t_mmd)}",
              f"  embed_mmd_sums, 4550 x 4550 x 1024 (50 scenes)    {stats(t_big)}",
              f"    = {pairs} pairs of 1024 columns: {pairs * 1024 / (sorted(t_big)[len(t_big) // 2] * 1e-3) / 1e12:.2f} x 10^12 differences squared and added per second", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
