"""Headline benchmark: denoise steps/s of the EulerEDM x VideoUNet hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

N = 1 runs in this process. N > 1 with no WORLD_SIZE in the environment re-launches itself as
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same args>` (one rank per GPU,
backend "nccl" = RCCL); when the driver has already launched the ranks (WORLD_SIZE set) each rank just runs.

One "step" = one EulerEDMSampler.sampler_step (reference sampling.py:78-89): mask replace -> CFG-doubled UNet forward on
50 images (2 x 25 frames, latent 4x72x128 = 576x1024 pixels) -> guider combine -> Euler update, on the 50-step
sigma schedule. Inputs are synthetic and resident in HBM before the timed region; weights are random-init for the shipped
1.65 B-parameter configuration (every tensor non-zero). Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line. --full adds everything else on top: the level-0 attention
roofline (extra eager steps), the idle-stream host enqueue step, the side figures (unless --no-extras) and the CPU baseline (unless
--no-cpu-baseline). --dump-outputs DIR writes the latents after the last timed step as DIR/latents.npy (float32); the inputs and
weights are seeded, so equal arguments give equal inputs. K + W above the 50-step schedule restart the window from its initial noise.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_STEP_CFG = 1.604e14   # algorithmic FLOP of one CFG step at N=50, 72x128 (torch flop counter on the reference)
FLOP_ATTN_PER_STEP = 3.10e13   # of which spatial self-attention cores
MFMA_BF16_PEAK = 2.5e15        # dense bf16 MFMA peak, MI355X_MICROARCH.md
HBM_PEAK = 8.0e12              # HBM3E spec peak, same guide
METRIC = "denoise steps/sec, 25-frame 576x1024 latent, 50-step EDM @ 1/2/4/8 GPU"
EDM = {"target": "vwm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": {"sigma_min": 0.002, "sigma_max": 700.0, "rho": 7.0}}


def build_model(model_channels, seed=0):
    from vista_amd.config import unet_kwargs
    from vista_amd.modules.diffusionmodules.video_model import VideoUNet
    with torch.device("cuda"):
        net = VideoUNet(**unet_kwargs(model_channels))
    net = net.cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():  # re-randomise EVERY tensor: the default init zeroes 403 of them and the net would output 0
        for name, p in net.named_parameters():
            if name.endswith("mix_factor"):
                p.normal_(0, 0.5, generator=g)
            elif p.dim() >= 2:
                p.normal_(0, float(p[0].numel()) ** -0.5, generator=g)
            elif name.endswith(".weight"):
                p.normal_(1.0, 0.1, generator=g)
            else:
                p.normal_(0, 0.1, generator=g)
    return net.eval()


def cpu_baseline(net, T, H, W, seed):
    """CPU leg, on the host cores of the GPU box, bounded to about a minute: REAL full-size pieces of the timed step run through the fp32 CPU
    restatement of the reference (oracle/vista_oracle.py -- the ORACLE, a restatement, NOT the reference itself: /root/reference does not
    exist on the GPU box, so kind is always "port"; the oracle is pinned to the reference's own modules at <= 2e-4 of output rms by
    tests/test_oracle_cpu.py and calls the same ATen ops), with the network's own weights, one clip (T frames) of the CFG pair each:
      level 0 (width 320, 72x128):  input_blocks.1.1 SpatialVideoTransformer (spatial + temporal transformer block) and input_blocks.1.0
                                    VideoResBlock (2-D ResBlock + 3x1x1 temporal ResBlock + blend),
      level 1 (width 640, 36x64):   input_blocks.5.1 / input_blocks.5.0,
      level 2 (width 1280, 18x32):  input_blocks.8.1 / input_blocks.8.0.
    Their FLOPs are counted by torch's flop counter. A step holds 2 clips x 5 such (transformer, ResBlock) pairs per level (2 input + 3 output
    blocks; the output blocks' first convolutions are wider, so the share below is a slight under-count): `share_of_step_flop` of the step is
    measured, the rest is estimated at the blended rate of the measured pieces. Nothing is read from earlier rounds' files. Also returns the HIP
    path's relative L2 error against the oracle on every piece (the same modules of the timed network, same inputs)."""
    from torch.utils.flop_counter import FlopCounterMode
    from oracle import vista_oracle as O
    from vista_amd import ops, synth
    cores = torch.get_num_threads()
    sd = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731  (inputs representable in the HIP path's storage type)
    emb = bf(torch.randn(T, 1280, generator=g) * 0.7)
    w = synth.window_inputs(T=T, H=2, W=2, seed=seed, trajectory=[0.5, 0, 1.0, 0, 1.5, 0.1, 2.0, 0.2])
    ctx = bf(w["c"]["crossattn"])   # (T, 1, 3456): CLIP-like token + action sinusoids
    rel = lambda a, r: ((a - r).pow(2).sum().sqrt() / r.pow(2).sum().sqrt()).item()  # noqa: E731
    frame_idx = torch.arange(T, dtype=torch.float32).cuda()
    ctx_dev = ops.cast_to_bf16(ctx.reshape(T, -1).cuda())
    emb_dev = torch.nn.functional.silu(emb).to(torch.bfloat16).cuda()
    pieces, parity = [], {}
    with torch.no_grad():
        for level, (blk, width, h, wd) in enumerate(((1, 320, H, W), (5, 640, H // 2, W // 2), (8, 1280, H // 4, W // 4))):
            x = bf(torch.randn(T, width, h, wd, generator=g))
            tok = x.permute(0, 2, 3, 1).reshape(T, h * wd, -1).to(torch.bfloat16).cuda().contiguous()
            nchw = lambda t: t.float().cpu().view(T, h, wd, -1).permute(0, 3, 1, 2)  # noqa: E731
            for name, fn, hip in ((f"level-{level} SpatialVideoTransformer (input_blocks.{blk}.1)",
                                   lambda: O.spatial_video_transformer(sd, f"input_blocks.{blk}.1", x, ctx, T, True),
                                   lambda: net.input_blocks[blk][1](tok, ctx_dev, frame_idx, T, h, wd)),
                                  (f"level-{level} VideoResBlock (input_blocks.{blk}.0)",
                                   lambda: O.video_resblock(sd, f"input_blocks.{blk}.0", x, emb, T),
                                   lambda: net.input_blocks[blk][0](tok, emb_dev, T, h, wd))):
                with FlopCounterMode(display=False) as fc:
                    t0 = time.perf_counter()
                    ref = fn()
                    dt = time.perf_counter() - t0
                pieces.append((name, dt, float(fc.get_total_flops())))
                parity[name] = rel(nchw(hip()), ref)
                del ref
    f_meas = sum(f for _, _, f in pieces)
    t_meas = sum(t for _, t, _ in pieces)
    rate = f_meas / t_meas
    est_s = FLOP_PER_STEP_CFG / rate
    share = 2 * 5 * f_meas / FLOP_PER_STEP_CFG   # 2 clips x 5 (transformer, ResBlock) pairs per level and forward
    return {"value": 1.0 / est_s, "unit": "steps/s", "cores": cores, "kind": "port",
            "sample": f"six full-size pieces of the step timed in this run on the host ({cores} threads) through the ORACLE (oracle/vista_oracle.py: fp32 restatement "
                      f"of the reference, pinned to the reference's own modules by tests/test_oracle_cpu.py -- not the reference itself, which does not exist on "
                      f"this box; its attention is the literal matmul / softmax / matmul walked in head slices of <= 2 GB of scores, where the reference's "
                      f"shimmed xformers call would be one fused SDPA: a pessimistic baseline for the level-0 transformer piece), one 25-frame clip each, network weights: "
                      + "; ".join(f"{n}: {t:.1f} s, {f / 1e12:.2f} TFLOP" for n, t, f in pieces) +
                      f" -> {rate / 1e12:.3f} TFLOP/s blended; 2 clips x 5 such pairs per level are {100 * share:.0f} % of the step's {FLOP_PER_STEP_CFG:.3e} FLOP; "
                      f"the rest is EXTRAPOLATED at the blended rate: {est_s:.0f} s/step",
            "measured": {"seconds": t_meas, "flop": f_meas, "share_of_step_flop": share},
            "parity_rel_l2_hip_vs_oracle": parity}


def attn_traffic_record(root):
    """(bytes per level-0 attention launch | None, where it came from). The HBM bytes come from separate rocprofv3 PMC passes (they cannot share a
    run with the timed region): the newest profiles/r*_attn_traffic.json, which is STAMPED with the sha256 of the csrc/attention.hip it was measured
    on -- a kernel source that has changed since reports no traffic rather than stale bytes (tests/test_bench_launch_cpu.py pins both branches)."""
    import glob
    import hashlib
    sha = hashlib.sha256(open(os.path.join(root, "vista_amd", "csrc", "attention.hip"), "rb").read()).hexdigest()
    cands = sorted(glob.glob(os.path.join(root, "profiles", "r*_attn_traffic.json")))
    if not cands:
        return None, "no profiles/r*_attn_traffic.json"
    rec = json.load(open(cands[-1]))
    name = os.path.relpath(cands[-1], root)
    if rec.get("attention_hip_sha256") == sha:
        return rec["traffic_bytes_per_launch"], f"rocprofv3 PMC passes of the same kernel and shape, {name} (sha256 of csrc/attention.hip matches the loaded tree)"
    return None, f"{name} was measured on another csrc/attention.hip (sha256 mismatch): traffic dropped, re-run tools/prof_r05.sh"


def spawn_ranks(n):
    """`python bench.py --gpus N` from a plain shell: become the launcher of N ranks (one per GPU) and relay their exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def plumbing_only(args, world, rank, dist, backend, device="cpu"):
    """Launch / rendezvous / partition check with no model work: builds both shard layouts and runs FrameShard.selfcheck on each
    (every collective signature of a sharded step -- unequal-split all_to_all_single at the four UNet levels, zero-length halo splits,
    the 512-byte statistics all-reduce, padded all_gather lists -- with value checks). On the host over gloo (CPU test of the N > 1 launch
    path) or, where GPUs are visible, on device tensors over RCCL: `bench.py --gpus N --plumbing-only` is the first thing to run on a
    multi-GPU box."""
    from vista_amd.parallel import DistComm, make_shard
    T = args.frames

    def make_group(ranks):
        g = dist.new_group(ranks=ranks)
        return DistComm(g) if rank in ranks else None
    layouts = {}
    for mode in ("hybrid", "frames"):
        sh = make_shard(T, world, rank, mode=mode, make_group=make_group)
        layouts[mode] = {"t_counts": sh.t_counts, "cfg_half": sh.cfg_half}
        sh.selfcheck(device)
    t = torch.tensor([float(rank)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    assert int(t.item()) == world - 1
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "steps/s", "n_gpus": world, "plumbing_only": True, "backend": backend,
                          "device": str(device), "layouts": layouts}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def gemm_rooflines(ops, n_img, H, W):
    """Per-kernel roofline entries for the three GEMM buckets of the kernel trace (level-0 shapes of the BASELINE config), timed here
    with HIP events on the launch stream, 10 launches each after 2 warm-ups."""
    dev = "cuda"
    M, C = n_img * H * W, 320
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = rn(M, C).to(torch.bfloat16)
    res = rn(M, C).to(torch.bfloat16)
    pw_lin = ops.pack_linear(rn(C, C) * C ** -0.5, rn(C))
    pw_geglu = ops.pack_geglu(rn(8 * C, C) * C ** -0.5, rn(8 * C))
    pw_conv = ops.pack_conv3x3(rn(C, C, 3, 3) * (9 * C) ** -0.5, rn(C))
    x3 = x.view(n_img, H * W, C)
    pw_ffo = ops.pack_ff_out(rn(C, 4 * C) * (4 * C) ** -0.5, rn(C))
    pw_ffo_plain = ops.pack_linear(rn(C, 4 * C) * (4 * C) ** -0.5, rn(C))
    cases = [
        # (since round 4 the launcher sends this shape to gemm_stream.hip: weights in registers, activations through an LDS-DMA ring)
        ("gemm_stream_kernel / gemm_kernel[dense,linear] level-0 projection 460800x320x320 (+residual)", lambda: ops.linear(x, pw_lin, res1=res),
         2.0 * M * C * C, 3.0 * M * C * 2, "hbm"),
        # (level-0 GEGLU as its own launch: no longer on the step's path since round 4 -- the level-0 FeedForward is ff_fused_kernel, next entry --
        #  kept as the figure VERDICT r3 tracks; levels 1 / 2 still run this kernel)
        ("gemm_kernel[dense,geglu,256x256] level-0 GEGLU 460800x320->2560 (gated to 1280)", lambda: ops.linear(x, pw_geglu),
         2.0 * M * 8 * C * C, M * C * 2 + M * 4 * C * 2, "mfma"),
        ("ff_fused_kernel level-0 FeedForward 460800x320->1280(GEGLU)->320 (+residual), hidden activation never written", lambda: ops.ff_fused(x, pw_geglu, pw_ffo, res1=res),
         2.0 * M * 8 * C * C + 2.0 * M * 4 * C * C, 3.0 * M * C * 2, "mfma"),
        ("the same FeedForward as two launches (GEGLU GEMM + out-projection GEMM: the round-3 path, out-projection on the pipelined kernel)", lambda: ops.linear(ops.linear(x, pw_geglu), pw_ffo_plain, res1=res),
         2.0 * M * 8 * C * C + 2.0 * M * 4 * C * C, 3.0 * M * C * 2 + 2.0 * M * 4 * C * 2, "mfma"),
        ("gemm_pipe_kernel[conv3x3,linear,256x320 pipelined] level-0 conv 320->320 @72x128", lambda: ops.conv3x3(x3, pw_conv, n_img, H, W),
         2.0 * M * C * 9 * C, 2.0 * M * C * 2, "mfma"),
    ]
    # the level-0 q|k|v projection (folded LayerNorm, K = 320 -> N = 960: HBM-bound) and the level-1 FeedForward pieces
    M1, C1 = n_img * (H // 2) * (W // 2), 640
    x1 = rn(M1, C1).to(torch.bfloat16)
    res1 = rn(M1, C1).to(torch.bfloat16)

    class _LN:   # LayerNorm parameter container for the fold (ops._ln_tuple)
        def __init__(self, c):
            self.weight, self.bias, self.eps = 1.0 + 0.1 * rn(c), 0.1 * rn(c), 1e-5
    pw_qkv = ops.pack_linear_cat([rn(C, C) * C ** -0.5 for _ in range(3)], ln=_LN(C))
    st0 = ops.rowstats(x)
    pw_geglu1 = ops.pack_geglu(rn(8 * C1, C1) * C1 ** -0.5, rn(8 * C1), ln=_LN(C1))
    pw_ffo1 = ops.pack_linear(rn(C1, 4 * C1) * (4 * C1) ** -0.5, rn(C1))
    st1 = ops.rowstats(x1)
    cases += [
        ("gemm_pipe_kernel[dense,linear,LayerNorm fold] level-0 q|k|v projection 460800x320->960", lambda: ops.linear(x, pw_qkv, ln=st0),
         2.0 * M * 3 * C * C, M * C * 2 + M * 3 * C * 2 + M * 8.0, "hbm"),
        ("gemm_pipe_kernel[dense,geglu,LayerNorm fold] level-1 GEGLU 115200x640->5120 (gated to 2560)", lambda: ops.linear(x1, pw_geglu1, ln=st1),
         2.0 * M1 * 8 * C1 * C1, M1 * C1 * 2 + M1 * 4 * C1 * 2, "mfma"),
        ("level-1 FeedForward as it runs (GEGLU GEMM + out-projection GEMM with residual and row sums; not fused at width 640)",
         lambda: ops.linear(ops.linear(x1, pw_geglu1, ln=st1), pw_ffo1, res1=res1, emit_stats=True),
         2.0 * M1 * 8 * C1 * C1 + 2.0 * M1 * 4 * C1 * C1, 3.0 * M1 * C1 * 2 + 2.0 * M1 * 4 * C1 * 2, "mfma"),
    ]
    # the temporal ResBlock's 3x1x1 convolution at level 0 (video_model.py:38-52; K = 3 C = 960: shallow for the pipelined kernel)
    pw_t3 = ops.pack_conv_t3(rn(C, C, 3, 1, 1) * (3 * C) ** -0.5, rn(C))
    T = 25 if n_img % 25 == 0 else n_img
    cases.append(("gemm_pipe_kernel[temporal3,linear,256x320 pipelined] level-0 temporal conv 3x1x1 320->320, T = 25 @72x128",
                  lambda: ops.conv_t3(x3, pw_t3, T, H * W), 2.0 * M * 3 * C * C, 2.0 * M * C * 2, "mfma"))
    return _time_cases(cases)


def hbm_rooflines(ops, n_img, H, W):
    """roofline entries of the two HBM-bound kernels the north-star names beside the attention (GroupNorm+SiLU, temporal attention), level-0 shapes
    of the BASELINE config: algorithmic bytes (input read once + output written once, bf16) / HIP-event time / 8 TB/s."""
    dev = "cuda"
    C, S, heads = 320, H * W, 5
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(n_img, S, C, device=dev, generator=g).to(torch.bfloat16)
    gam, bet = torch.randn(C, device=dev, generator=g), torch.randn(C, device=dev, generator=g)
    T = 25 if n_img % 25 == 0 else n_img
    B = n_img // T
    qkv = torch.randn(n_img * S, 3 * C, device=dev, generator=g).to(torch.bfloat16)
    nbytes = float(x.numel() * 2)
    cases = [
        ("GroupNorm(32)+SiLU level 0 (50 x 9216 x 320): gn_stats + gn_apply (the apply pass folds the statistics slots itself since round 6)",
         lambda: ops.groupnorm(x, gam, bet, 1e-5, True), 10.0 * x.numel(), 2.0 * nbytes, "hbm"),   # (the two-pass form reads x twice: its traffic is up to 3 x nbytes)
        ("attn_temporal_kernel level 0: 92160 (pixel, head) problems of 25 x 25 x 64 (video_attention.py:116-127)",
         lambda: ops.attn_temporal(qkv, B, T, S, heads), 4.0 * B * S * heads * T * T * 64, 4.0 * nbytes, "hbm"),   # q | k | v read + o written
    ]
    return _time_cases(cases)


def fp16_side_figure(args):
    import subprocess
    env = dict(os.environ, VISTA_ACT_DTYPE="fp16")
    env.pop("VISTA_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--full", "--no-cpu-baseline", "--no-extras"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        d = json.loads(line)
        return {"value": d["value"], "unit": "steps/s", "ms_per_step": d["ms_per_step"], "dtype": d["dtype"],
                "attention_frac": (d.get("roofline") or {}).get("frac"),
                "note": "same step, fp16 activations / weights (v_mfma_f32_32x32x16_f16; softmax numerators and V stay bf16), own process: "
                        "VISTA_ACT_DTYPE=fp16 python bench.py; parity: tests/test_f16_gpu.py (full-width UNet within 6e-3 of the fp32 reference "
                        "against the bf16 build's 1.2e-2)"}
    except Exception as e:  # noqa: BLE001 -- a side figure never takes the headline line down
        return {"error": f"{type(e).__name__}: {e}"[:300]}


def _time_cases(cases):
    out = []
    for name, fn, flop, byts, bound in cases:
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        tf, gbs = flop / ms / 1e9, byts / ms / 1e6
        out.append({"kernel": name, "bound": bound, "avg_ms": ms, "tflops": tf, "algorithmic_GBps": gbs,
                    "achieved": gbs if bound == "hbm" else tf, "peak": HBM_PEAK / 1e9 if bound == "hbm" else MFMA_BF16_PEAK / 1e12,
                    "unit": "GB/s" if bound == "hbm" else "TFLOP/s",
                    "frac": gbs / (HBM_PEAK / 1e9) if bound == "hbm" else tf / (MFMA_BF16_PEAK / 1e12)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--latent-h", type=int, default=72)
    ap.add_argument("--latent-w", type=int, default=128)
    ap.add_argument("--model-channels", type=int, default=320)
    ap.add_argument("--full", action="store_true", help="besides the headline: attention roofline, idle-stream enqueue step, side figures, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the latents after the last timed step to DIR/latents.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the side figures (IdentityGuider N=25, GEMM rooflines, config-3 layout)")
    ap.add_argument("--shard", choices=["hybrid", "frames"], default="hybrid")
    ap.add_argument("--plumbing-only", action="store_true", help="N > 1: rendezvous + partition/exchange check on the host, no GPU work")
    ap.add_argument("--graph", action="store_true", help="replay every step's UNet forward from one captured hipGraph (FusedLoop(graph=True)): the DEFAULT on one "
                    "GPU since round 6 (same kernels on the same buffers, bitwise the eager loop's result: tests/test_model_gpu.py::test_hipgraph_*; 165.2 vs 165.4 "
                    "ms per step, host enqueue 0.4 vs 10 ms); the level-0 attention launches of the roofline object are timed on two extra eager steps. N > 1: "
                    "refused over RCCL (capturing its collectives hangs on this stack, DESIGN section 6) unless VISTA_HIPGRAPH_RCCL=1")
    ap.add_argument("--one-stream", action="store_true", help="one GPU, graph replay: the step's two guidance halves as ONE forward of 50 images on one stream (the form of "
                    "rounds 1-5) instead of two concurrent 25-image graphs on two streams (FusedLoop(cfg_streams=True), the default since round 6: -2.4 %%)")
    ap.add_argument("--eager", action="store_true", help="one GPU: enqueue every launch from Python each step instead of replaying the captured graph")
    ap.add_argument("--fp8", action="store_true",
                    help="BASELINE config 5, NOT the headline: FeedForward GEMMs AND the ResBlock convolutions in fp8 e4m3 (reported dtype says so)")
    ap.add_argument("--fp8-no-attn", action="store_true", help="with --fp8: keep the attention score product and the attention-out projection in bf16 (the round-2 form)")
    ap.add_argument("--fp8-ff", action="store_true",
                    help="BASELINE config 5 experiment, NOT the headline: FeedForward GEMMs in fp8 e4m3 (reported dtype says so)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("VISTA_DIST_BACKEND", "nccl")  # "gloo" + VISTA_FORCE_DEVICE=0: dry run of the N>1 path on one GPU
    if "VISTA_FORCE_DEVICE" in os.environ:
        local_rank = int(os.environ["VISTA_FORCE_DEVICE"])
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.plumbing_only and not (torch.cuda.is_available() and backend == "nccl"):
            dist.init_process_group("gloo")
            return plumbing_only(args, world, rank, dist, "gloo")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))  # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend)
        if args.plumbing_only:
            return plumbing_only(args, world, rank, dist, backend, device=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(local_rank)
    if args.fp8_ff or args.fp8:
        from vista_amd.modules import attention as _att
        _att.FP8["feedforward"] = True
        _att.FP8["conv"] = bool(args.fp8)
        _att.FP8["attention"] = _att.FP8["proj"] = bool(args.fp8) and not args.fp8_no_attn
    from vista_amd import _lib, ops, synth
    from vista_amd.modules.diffusionmodules.denoiser import Denoiser
    from vista_amd.modules.diffusionmodules.sampling import EulerEDMSampler, FusedDenoiser, FusedLoop
    from vista_amd.modules.diffusionmodules.wrappers import OpenAIWrapper
    _lib.load()

    T, H, W = args.frames, args.latent_h, args.latent_w
    shards = {None: None}
    if world > 1:
        from vista_amd.parallel import DistComm, make_shard

        def make_group(ranks):  # collective: every rank creates every group, members get a communicator
            g = dist.new_group(ranks=ranks)
            return DistComm(g) if rank in ranks else None
        # 'hybrid' (default): CFG halves x frame groups -- 8 GPUs = 2 x (7/6/6/6); 'frames': 4/3/3/3/3/3/3/3 (BASELINE config 3)
        shards = {args.shard: make_shard(T, world, rank, mode=args.shard, make_group=make_group)}
        other = "frames" if args.shard == "hybrid" else "hybrid"
        if args.full and not args.no_extras and world % 2 == 0:  # odd worlds have one layout only
            shards[other] = make_shard(T, world, rank, mode=other, make_group=make_group)
        # Plumbing pass BEFORE any model work: every collective signature of the sharded step on tiny device tensors, synchronised one by
        # one, so that a transport problem on a box this code has never seen is reported by name within seconds (vista_amd/parallel.py).
        for key, sh in shards.items():
            try:
                sh.selfcheck(torch.device("cuda", local_rank))
            except Exception as e:  # noqa: BLE001
                print(f"[bench rank {rank}] multi-GPU plumbing check FAILED for layout '{key}': {e}", file=sys.stderr, flush=True)
                raise
    net = build_model(args.model_channels)
    w = synth.window_inputs(T=T, H=H, W=W, seed=0)
    cu = lambda d: {k: v.cuda() for k, v in d.items()}  # noqa: E731
    den = Denoiser(scaling_config={"target": "vwm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"}, num_frames=T)
    sampler = EulerEDMSampler(num_steps=50, discretization_config=EDM,
                              guider_config={"target": "vwm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 2.5}}, device="cuda")
    noise = w["noise"].cuda()
    x, sigmas, _, cond, uc = sampler.prepare_sampling_loop(noise, cu(w["c"]), cu(w["uc"]))
    sig = [float(s) for s in sigmas]
    nsteps = len(sig) - 1
    fd = FusedDenoiser(den, OpenAIWrapper(net))

    def timed_loop(shard, profile_attn, graph=False, settle=0, after=True, keep=False):
        """W warm-up + K timed steps of a fresh window; returns (seconds for K steps = MAX over ranks, host enqueue seconds, loop, the whole
        window's latents after the last timed step if `keep`). Step j runs schedule step j % 50: past its end the window restarts from its
        initial noise. after: the idle-stream enqueue step and the attention-timing steps behind the timed region (--full).
        settle: extra untimed steps of a throw-away window first (a path that has just been switched on builds its weight packs in its first
        step and the allocator re-settles in the next one or two: config 5 measured 160.8 ms with one warm-up step, 151.7 with three)."""
        if settle:
            tmp = FusedLoop(sampler, fd, x.float().clone(), cond, uc, w["cond_frame"].cuda(), w["cond_mask"].cuda(), True, sig, shard=shard)
            for i in range(settle):
                tmp.step(i)
            del tmp
        loop = FusedLoop(sampler, fd, x.float().clone(), cond, uc, w["cond_frame"].cuda(), w["cond_mask"].cuda(), True, sig, shard=shard,
                         graph=graph, cfg_streams=bool(graph and shard is None and not args.one_stream))
        x_start = loop.xw.clone() if args.warmup + args.steps > nsteps else None

        def step(j):
            if j and j % nsteps == 0:
                loop.xw.copy_(x_start)
            loop.step(j % nsteps)
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.warmup, args.warmup + args.steps):
            step(i)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dist is not None:  # MAX over ranks
            tdt = torch.tensor([dt], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(tdt, op=dist.ReduceOp.MAX)
            dt = float(tdt.item())
        assert torch.isfinite(loop.xw).all(), "non-finite latents"
        last = None
        if keep:
            last = (loop.xw if shard is None else shard.gather_frames(loop.xw)).float().cpu()
        # Host cost of enqueueing ONE step, measured OUTSIDE the timed region from an idle stream (sync, enqueue, stop the clock before the
        # next sync): inside the timed region the launch queue is full and the host clock only sees the GPU's back-pressure.
        t_enq = None
        nxt = args.warmup + args.steps
        if after and nxt < nsteps:
            t1 = time.perf_counter()
            loop.step(nxt)
            t_enq = time.perf_counter() - t1
            torch.cuda.synchronize()
            nxt += 1
            if dist is not None:
                dist.barrier()
        # The roofline kernel's launches are timed with HIP events (recorded on the launch stream, ops.attn_spatial) on up to two MORE steps of
        # the same window, right after the timed region: the timed region itself carries no profiling work
        if after and profile_attn and not graph:
            ops.PROFILE_ATTN = []
            for i in range(nxt, min(nxt + 2, nsteps)):
                loop.step(i)
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
        return dt, t_enq, loop, last

    main_key = args.shard if world > 1 else None
    shard = shards[main_key]
    # one GPU: graph replay unless --eager; N > 1: eager unless --graph (the sharded forward's capture has only ever run with the mock communicator)
    args.graph = (not args.eager) if world == 1 else bool(args.graph)
    dt, t_enqueue, _, latents = timed_loop(shard, not args.graph, graph=args.graph, after=args.full, keep=bool(args.dump_outputs))
    if args.graph and args.full:  # a replayed graph runs no Python between launches: time the roofline kernel's launches on two eager steps of the same state
        eager = FusedLoop(sampler, fd, x.float().clone(), cond, uc, w["cond_frame"].cuda(), w["cond_mask"].cuda(), True, sig, shard=shard, graph=False)
        eager.step(0)
        torch.cuda.synchronize()
        ops.PROFILE_ATTN = []
        eager.step(1)
        eager.step(2)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
    prof, ops.PROFILE_ATTN = ops.PROFILE_ATTN or [], None
    ms_per_step = dt * 1e3 / args.steps
    value = args.steps / dt
    full = (T, H, W, args.model_channels) == (25, 72, 128, 320)

    l0 = [(e0.elapsed_time(e1), nbh) for (S, nbh, e0, e1) in prof if S == H * W]
    roofline = None
    if l0:
        nbh = l0[0][1]  # (local images) x heads of this rank's level-0 launches
        l0 = [t for t, _ in l0]
        avg_ms = sum(l0) / len(l0)
        flop = 4.0 * nbh * float(H * W) ** 2 * 64
        ach = flop / (avg_ms * 1e-3) / 1e12
        # HBM bytes per launch come from separate rocprofv3 PMC passes (they cannot share a run with the timed region): the newest
        # profiles/r*_attn_traffic.json, which is STAMPED with the sha256 of the csrc/attention.hip it was measured on -- a kernel source that
        # has changed since reports no traffic rather than stale bytes
        traffic, traffic_src = (None, "reduced configuration / multi-GPU run: no traffic figure") if not (full and world == 1) else attn_traffic_record(ROOT)
        roofline = {"kernel": "level-0 spatial self-attention, vk_attn_spatial_qkv_log2_bf16: attn_spatial_pipe_kernel<4> (software-pipelined zero-base form; "
                              "VISTA_ATTN_PIPE=0 selects the round-4 attn_spatial_kernel<8,2>)", "bound": "mfma", "achieved": ach,
                    "peak": MFMA_BF16_PEAK / 1e12, "unit": "TFLOP/s", "frac": ach / (MFMA_BF16_PEAK / 1e12), "traffic": traffic,
                    "traffic_source": traffic_src,
                    "launches_timed": len(l0), "avg_ms": avg_ms, "flop_per_launch": flop,
                    "timed_on": "HIP events on the launch stream around each level-0 launch of up to two extra steps of the same window, immediately after the timed region"}

    act_name = "fp16" if _lib.ACT_DTYPE == "fp16" else "bf16"   # the 16-bit storage type of this process (VISTA_ACT_DTYPE; default bf16 = BASELINE config 2's)

    def layout(sh):
        return (("CFG-split x2 x " if sh.cfg_half is not None else "") + "frame-sharded " + "/".join(str(c) for c in sh.t_counts)) if sh else "single GPU"
    res = {
        "metric": METRIC, "value": value, "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": (("bf16 + fp8(e4m3) ResBlock convolutions, FeedForward GEMMs from width 640 up" + ("" if args.fp8_no_attn else ", attention QK^T, attention-out projections from width 640 up") + " [config 5]") if args.fp8 else
                  "bf16 + fp8(e4m3) FeedForward GEMMs [config 5, FeedForward only]" if args.fp8_ff else act_name),
        "data": "synthetic" if backend == "nccl" or world == 1 else "synthetic (DRY RUN: gloo host-staged transport, ranks share one GPU -- not a result)",
        "config": {"workload": (f"{world}xMI355X " + layout(shard) +
                                ": 25x576x1024 (latent 25x4x72x128), 50-step EulerEDM, VanillaCFG 2.5 (N=50 images per UNet call), "
                                f"{act_name}, random-init 1.65B VideoUNet, synthetic latents") if full else
                   f"REDUCED (not the BASELINE config): T={T} latent {H}x{W} model_channels={args.model_channels}, {world} rank(s) " + layout(shard),
                   "frames": T, "latent": [4, H, W], "cfg_images_per_call": 2 * T, "sampler": "EulerEDM s_churn=0, 50-step schedule",
                   "t_counts": shard.t_counts if shard else [T], "shard": main_key,
                   "windows_per_s": value / 50.0,
                   "parallelism": "single GPU" if shard is None else
                   (("CFG halves on 2 rank groups (one output exchange per step) x " if shard.cfg_half is not None else "") +
                    f"frame-shard x{shard.P} (spatial half) + pixel-shard x{shard.P} (temporal half), 2 RCCL all-to-alls per block pair, "
                    "weights replicated")},
        "roofline": roofline,
        "hipgraph": bool(args.graph),
        # the two guidance halves of every step as two concurrent 25-image hipGraphs on two streams (exact: the halves only share the batch axis)
        "cfg_streams": bool(args.graph and shard is None and not args.one_stream),
        "host_enqueue_ms_idle_stream": None if t_enqueue is None else t_enqueue * 1e3,  # one step enqueued after a sync, outside the timed region
        "step_mfma_frac": (FLOP_PER_STEP_CFG / (ms_per_step * 1e-3) / (MFMA_BF16_PEAK * world)) if full else None,
    }
    # ---- side figures (never `value`) ----
    if args.full and not args.no_extras:
        for key, sh in shards.items():  # the other multi-GPU layout, e.g. BASELINE config 3's 4/3/3/3/3/3/3/3 next to the hybrid default
            if key == main_key:
                continue
            dt2 = timed_loop(sh, False)[0]
            res["config3_frames_layout" if key == "frames" else "hybrid_layout"] = {
                "layout": layout(sh), "t_counts": sh.t_counts, "value": args.steps / dt2, "ms_per_step": dt2 * 1e3 / args.steps}
        if world == 1:
            # N = 25 images per UNet call (IdentityGuider: no classifier-free guidance), through the reference-shaped generic sampler path
            ident = EulerEDMSampler(num_steps=50, discretization_config=EDM, guider_config=None, device="cuda")
            xi = x.float().clone()
            n = xi.shape[0]
            maskf = w["cond_mask"].cuda().float()

            def ident_step(i):
                i %= nsteps
                s0, s1 = torch.full((n,), sig[i], device="cuda"), torch.full((n,), sig[i + 1], device="cuda")
                return ident.sampler_step(s0, s1, fd, xi, cond, maskf, uc, 0.0)
            for i in range(args.warmup):
                ident_step(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.warmup, args.warmup + args.steps):
                ident_step(i)
            torch.cuda.synchronize()
            dti = time.perf_counter() - t0
            res["identity_guider_n25"] = {"value": args.steps / dti, "unit": "steps/s", "ms_per_step": dti * 1e3 / args.steps,
                                          "note": "IdentityGuider: one UNet forward on N=25 images per step (half the CFG work), generic sampler path"}
            if full:
                res["roofline_gemm"] = gemm_rooflines(ops, 2 * T, H, W)
                res["roofline_hbm"] = hbm_rooflines(ops, 2 * T, H, W)
            if full and not (args.fp8 or args.fp8_ff):
                # BASELINE config 5 as a side figure of the default (bf16) line: the same step with FeedForward GEMMs, ResBlock convolutions, the
                # attention score product and the attention-out projection in fp8 e4m3; the fp8 weight packs are built during the
                # warm-up steps. Not the headline: `value` above stays bf16.
                from vista_amd.modules import attention as _att
                saved = dict(_att.FP8)
                try:
                    for k in ("feedforward", "conv", "attention", "proj"):
                        _att.FP8[k] = True
                    dt8 = timed_loop(None, False, settle=2)[0]
                    res["config5_fp8"] = {"value": args.steps / dt8, "unit": "steps/s", "ms_per_step": dt8 * 1e3 / args.steps,
                                          "note": "same step, fp8(e4m3) ResBlock convolutions, attention QK^T, and -- from block width 640 up, where fp8 still beats the bf16 kernels -- FeedForward GEMMs and attention-out projections; "
                                                  "parity: tests/test_fp8_gpu.py, tests/test_blocks_gpu.py"}
                finally:
                    _att.FP8.update(saved)
            if full and not (args.fp8 or args.fp8_ff) and _lib.ACT_DTYPE == "bf16":
                # The fp16-storage build (libvista_hip_f16.so: the reference's own autocast width, sample_utils.py:301-303) as a side
                # figure: the same step in a process of its own (the storage type is fixed per process). Never `value`: BASELINE config 2 names bf16.
                res["fp16_storage"] = fp16_side_figure(args)
    if args.full and not args.no_cpu_baseline and rank == 0 and world == 1:
        res["cpu_baseline"] = cpu_baseline(net, T, H, W, seed=1) if full else None
    else:
        res["cpu_baseline"] = None
    if rank == 0:
        if args.dump_outputs:
            import numpy as np
            os.makedirs(args.dump_outputs, exist_ok=True)
            np.save(os.path.join(args.dump_outputs, "latents.npy"), latents.numpy().astype(np.float32))
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
