"""Frame-sharded execution validated on ONE GPU: P ranks run as threads of this process (vista_amd.parallel.ThreadComm,
same FrameShard / all-to-all code path as the RCCL run, in-memory transport) and must reproduce the unsharded result and the
reference's golden output. Tolerance = the unsharded one (the 5-D GroupNorm partial sums are combined in a different order
across ranks, which bf16 amplifies to its noise floor)."""
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRAJ = [0.5, 0, 1.0, 0, 1.5, 0.1, 2.0, 0.2]


def rel_l2(a, b):
    return ((a.float() - b.float()).pow(2).sum().sqrt() / b.float().pow(2).sum().sqrt()).item()


def run_ranks(P, fn):
    from vista_amd.parallel import ThreadComm
    shared = ThreadComm.Shared(P)
    out, errs = [None] * P, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            out[rank] = fn(ThreadComm(shared, rank))
        except Exception as e:  # noqa: BLE001
            import traceback
            errs.append((rank, traceback.format_exc()))
            shared.barrier.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs[0][1]
    return out


@pytest.mark.parametrize("P,chunks", [(2, 1), (3, 1), (2, 2), (3, 3)])
def test_sharded_unet_forward_matches_unsharded_and_golden(P, chunks, monkeypatch):
    """chunks > 1 = VISTA_A2A_CHUNKS: the temporal block on pixel sub-ranges with one (asynchronously started) all-to-all per sub-range."""
    monkeypatch.setenv("VISTA_A2A_CHUNKS", str(chunks))
    from oracle.make_golden import unet_inputs
    from tests.test_model_gpu import tiny_unet
    from vista_amd import ops
    from vista_amd.modules.diffusionmodules.video_model import CIN_PAD
    from vista_amd.parallel import FrameShard
    net, _ = tiny_unet()
    g = torch.load(os.path.join(GOLD, "unet_tiny_t5.pt"))
    T, H, W = g["T"], g["H"], g["W"]
    x8, ts, ctx, y, mask = [t.cuda() for t in unet_inputs(T, H, W, seed=g["seed_x"], sigma=g["sigma"])]
    tokens = ops.nchw_to_tokens(x8.float(), CIN_PAD)                       # (2T, S, 64), (b t) order
    ref_tok = net.forward_tokens(tokens, ts, ctx, y, mask, T, H, W).clone()

    def rank_fn(comm):
        sh = FrameShard(T, comm, B=2)
        local = sh.take_local_rows(tokens).contiguous()
        return sh, net.forward_tokens(local, ts, ctx, y, mask, T, H, W, shard=sh)

    outs = run_ranks(P, rank_fn)
    full = torch.empty_like(ref_tok)
    for sh, o in outs:
        full[torch.tensor(sh.local_image_ids(), device="cuda")] = o
    r_un = rel_l2(full, ref_tok)
    gold = g["out"].cuda().permute(0, 2, 3, 1).reshape(2 * T, H * W, 4)
    r_gold = rel_l2(full, gold)
    print(f"[parity] sharded P={P} chunks={chunks}: vs unsharded {r_un:.3e}, vs reference golden {r_gold:.3e}")
    assert r_un <= 2.5e-2 and r_gold <= 2.5e-2
    assert all(sh.a2a_chunks == chunks for sh, _ in outs)


def test_sharded_sampler_matches_golden():
    from tests.test_model_gpu import _sampler, tiny_unet
    from vista_amd import synth
    from vista_amd.modules.diffusionmodules.denoiser import Denoiser
    from vista_amd.modules.diffusionmodules.sampling import FusedDenoiser
    from vista_amd.modules.diffusionmodules.wrappers import OpenAIWrapper
    from vista_amd.parallel import FrameShard
    g = torch.load(os.path.join(GOLD, "sampler_tiny.pt"))
    net, _ = tiny_unet()
    T, H, W = g["T"], g["H"], g["W"]
    w = synth.window_inputs(T=T, H=H, W=W, seed=g["seed_x"], n_cond=1, trajectory=TRAJ)
    den = Denoiser(scaling_config={"target": "vwm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"}, num_frames=T)
    fused = FusedDenoiser(den, OpenAIWrapper(net))
    cfg = {"target": "vwm.modules.diffusionmodules.guiders.LinearPredictionGuider", "params": {"num_frames": T, "max_scale": 2.5, "min_scale": 1.0}}

    def rank_fn(comm):
        s = _sampler(cfg)
        s.shard = FrameShard(T, comm, B=2)
        cu = lambda d: {k: v.clone().cuda() for k, v in d.items()}  # noqa: E731
        return s(fused, w["noise"].clone().cuda(), cond=cu(w["c"]), uc=cu(w["uc"]), cond_frame=w["cond_frame"].cuda(),
                 cond_mask=w["cond_mask"].cuda()).cpu()

    outs = run_ranks(2, rank_fn)
    assert torch.equal(outs[0], outs[1]), "every rank must return the same gathered window"
    r = rel_l2(outs[0], g["linear"])
    print(f"[parity] sharded sampler P=2: rel-L2 {r:.3e}")
    assert r <= 4e-2 and torch.equal(outs[0][0], w["cond_frame"][0])


@pytest.mark.parametrize("world,mode", [(2, "hybrid"), (4, "hybrid"), (6, "hybrid"), (3, "hybrid"), (8, "hybrid")])
def test_hybrid_cfg_x_frame_sampler_matches_golden(world, mode):
    """CFG x frame hybrid (make_shard): world=2 -> pure CFG split, 4 -> 2x2, 6 -> 2x3; odd world falls back to frame sharding."""
    from tests.test_model_gpu import _sampler, tiny_unet
    from vista_amd import synth
    from vista_amd.modules.diffusionmodules.denoiser import Denoiser
    from vista_amd.modules.diffusionmodules.sampling import FusedDenoiser
    from vista_amd.modules.diffusionmodules.wrappers import OpenAIWrapper
    from vista_amd.parallel import ThreadGroups, make_shard
    g = torch.load(os.path.join(GOLD, "sampler_tiny.pt"))
    net, _ = tiny_unet()
    T, H, W = g["T"], g["H"], g["W"]
    w = synth.window_inputs(T=T, H=H, W=W, seed=g["seed_x"], n_cond=1, trajectory=TRAJ)
    den = Denoiser(scaling_config={"target": "vwm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"}, num_frames=T)
    fused = FusedDenoiser(den, OpenAIWrapper(net))
    cfg = {"target": "vwm.modules.diffusionmodules.guiders.TrianglePredictionGuider", "params": {"num_frames": T, "max_scale": 2.5, "min_scale": 1.0}}
    groups = ThreadGroups()
    outs, errs = [None] * world, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            s = _sampler(cfg)
            s.shard = make_shard(T, world, rank, mode=mode, make_group=groups.make(rank))
            cu = lambda d: {k: v.clone().cuda() for k, v in d.items()}  # noqa: E731
            outs[rank] = s(fused, w["noise"].clone().cuda(), cond=cu(w["c"]), uc=cu(w["uc"]), cond_frame=w["cond_frame"].cuda(),
                           cond_mask=w["cond_mask"].cuda()).cpu()
        except Exception:  # noqa: BLE001
            import traceback
            errs.append(traceback.format_exc())
            groups.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs[0]
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "every rank must end with the same window"
    r = rel_l2(outs[0], g["triangle"])
    print(f"[parity] hybrid world={world}: rel-L2 {r:.3e}")
    assert r <= 4e-2 and torch.equal(outs[0][0], w["cond_frame"][0])


def test_eight_ranks_25_frames_hybrid_and_frames_layouts_vs_config1_golden():
    """The 8-GPU layouts of the bench in miniature, with thread ranks on one GPU: 25 frames, 10 EDM steps, VanillaCFG 2.5
    (config1_tiny golden from the real reference sampler). hybrid = 2 CFG halves x (7/6/6/6); frames = BASELINE config 3's 4/3/3/3/3/3/3/3."""
    from tests.test_model_gpu import _sampler, tiny_unet
    from vista_amd import synth
    from vista_amd.modules.diffusionmodules.denoiser import Denoiser
    from vista_amd.modules.diffusionmodules.sampling import FusedDenoiser
    from vista_amd.modules.diffusionmodules.wrappers import OpenAIWrapper
    from vista_amd.parallel import ThreadGroups, make_shard
    g = torch.load(os.path.join(GOLD, "config1_tiny.pt"))
    net, _ = tiny_unet()
    T, H, W, world = g["T"], g["H"], g["W"], 8
    w = synth.window_inputs(T=T, H=H, W=W, seed=g["seed_x"], n_cond=1)
    den = Denoiser(scaling_config={"target": "vwm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"}, num_frames=T)
    fused = FusedDenoiser(den, OpenAIWrapper(net))
    cfg = {"target": "vwm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 2.5}}
    for mode, counts in (("hybrid", [7, 6, 6, 6]), ("frames", [4, 3, 3, 3, 3, 3, 3, 3])):
        groups = ThreadGroups()
        outs, errs, seen = [None] * world, [], [None] * world

        def run(rank):
            try:
                torch.cuda.set_device(0)
                s = _sampler(cfg, steps=g["steps"])
                s.shard = make_shard(T, world, rank, mode=mode, make_group=groups.make(rank))
                seen[rank] = list(s.shard.t_counts)
                cu = lambda d: {k: v.clone().cuda() for k, v in d.items()}  # noqa: E731
                outs[rank] = s(fused, w["noise"].clone().cuda(), cond=cu(w["c"]), uc=cu(w["uc"]), cond_frame=w["cond_frame"].cuda(),
                               cond_mask=w["cond_mask"].cuda()).cpu()
            except Exception:  # noqa: BLE001
                import traceback
                errs.append(traceback.format_exc())
                groups.abort()

        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs[0]
        assert all(c == counts for c in seen), seen
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        r = rel_l2(outs[0], g["out"].float())
        print(f"[parity] 8 ranks, 25 frames, 10 steps, {mode}: rel-L2 {r:.3e}")
        assert r <= 4e-2


# ------------------------------------------------------------------------------------------------ real process groups
def _run(cmd, env_extra, timeout=900):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    import json
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stdout[-3000:]
    return json.loads(lines[-1])


def _torchrun(n, port, script, *args):
    import sys
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port",
            str(port), script, *args]


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_2_end_to_end_dry_run_on_one_gpu():
    """`python bench.py --gpus 2` with WORLD_SIZE unset: bench.py spawns the two ranks itself and the whole multi-rank path (both shard
    layouts, exchanges, MAX-over-ranks timing, one JSON line) runs -- here host-staged over gloo with both ranks on GPU 0 (labelled a dry
    run in `data`); on a multi-GPU node the same command runs over RCCL."""
    import sys
    res = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "5", "--latent-h", "16",
                "--latent-w", "32", "--model-channels", "64", "--full", "--no-cpu-baseline"], {"VISTA_DIST_BACKEND": "gloo", "VISTA_FORCE_DEVICE": "0"})
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["steps"] == 2
    assert res["config"]["t_counts"] == [5] and res["config"]["shard"] == "hybrid"
    assert res["config3_frames_layout"]["t_counts"] == [3, 2] and res["config3_frames_layout"]["value"] > 0
    assert "DRY RUN" in res["data"]


@pytest.mark.parametrize("mode", ["hybrid", "frames"])
def test_two_process_gloo_ranks_on_one_gpu_match_golden(mode):
    """Real torch.distributed process group (2 OS processes, gloo, host-staged transport, both on GPU 0) through DistComm."""
    res = _run(_torchrun(2, 29641 if mode == "hybrid" else 29642, os.path.join(ROOT, "tests", "_dist_worker.py"), mode),
               {"VISTA_DIST_BACKEND": "gloo", "VISTA_FORCE_DEVICE": "0"})
    assert res["world"] == 2 and all(r <= 4e-2 for r in res["rel_l2"]) and all(res["cond_frame_exact"])
    assert len(set(res["checksums"])) == 1, "every rank must end with the same window"
    print(f"[parity] 2 gloo processes, {mode}: rel-L2 {res['rel_l2']}")


@pytest.mark.parametrize("mode", ["hybrid", "frames"])
def test_two_ranks_over_rccl_match_golden(mode):
    """One process per GPU over RCCL (backend "nccl"); needs two visible GPUs (skipped on the 1-GPU test boxes)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    res = _run(_torchrun(2, 29643 if mode == "hybrid" else 29644, os.path.join(ROOT, "tests", "_dist_worker.py"), mode), {"VISTA_DIST_BACKEND": "nccl"})
    assert res["world"] == 2 and res["backend"] == "nccl" and all(r <= 4e-2 for r in res["rel_l2"]) and all(res["cond_frame_exact"])
    assert len(set(res["checksums"])) == 1


@pytest.mark.parametrize("chunks", [1, 2])
def test_single_rank_group_over_rccl_matches_golden(chunks):
    """The sharded step with every collective issued on a real RCCL process group of ONE rank (a one-GPU box cannot hold two: RCCL
    refuses duplicate devices). FrameShard.selfcheck and the 3-step CFG sampler run through DistComm(backend "nccl"): the call
    signatures, dtypes, zero-length splits, asynchronous Work handles (chunks = 2) and the stream ordering between RCCL's stream and
    the kernels' are the library's own; what stays untested without a second GPU is the transport."""
    res = _run(_torchrun(1, 29645 + chunks, os.path.join(ROOT, "tests", "_dist_worker.py"), "rccl1"),
               {"VISTA_DIST_BACKEND": "nccl", "VISTA_A2A_CHUNKS": str(chunks)})
    assert res["world"] == 1 and res["backend"] == "nccl" and res["a2a_chunks"] == chunks and res["selfcheck_steps"] >= 10
    cc = res["collective_calls"]   # selfcheck + 3 steps x one CFG-doubled forward: re-shards, halos and 5-D GroupNorm sums all went through RCCL
    assert cc["all_to_all"] >= 100 and cc["all_reduce_sum"] >= 30 and cc["all_gather_list"] >= 1, cc
    assert all(r <= 4e-2 for r in res["rel_l2"]) and all(res["cond_frame_exact"])
    print(f"[parity] one-rank RCCL group, VISTA_A2A_CHUNKS={chunks}: rel-L2 {res['rel_l2']}, {res['selfcheck_steps']} selfcheck steps, collectives {cc}")
