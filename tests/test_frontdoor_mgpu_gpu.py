"""The sampling front door on several ranks, validated on ONE GPU: `sample.run(shard=)` over thread ranks, `sample.main` as two gloo processes
that share GPU 0, and the sharded step through a one-rank RCCL group. The pipeline is the tiny one of tests/test_frontdoor_gpu.py (5 frames,
128 x 256, 3 steps). A sharded run differs from the unsharded one by the order in which the 5-D GroupNorm partial sums are combined, which bf16
amplifies to its noise floor: the bound is the 4e-2 rel-L2 tests/test_parallel_gpu.py uses for sharded sampler runs of this model class."""
import json
import os
import re
import subprocess
import sys
import threading
import traceback

import pytest
import torch

from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_sample_dist_worker.py")
BOUND = 4e-2
_RANDN = torch.randn


def rel_l2(a, b):
    return ((a.float() - b.float()).pow(2).sum().sqrt() / b.float().pow(2).sum().sqrt()).item()


class _NoisePerThread:
    """Thread ranks share one process and so ONE GPU random generator, where real ranks each own one and seed it alike. While this is
    installed every thread draws its GPU noise from a generator of its own, all seeded alike: each rank sees the stream a process of its own
    would see, and so does the unsharded run it is compared with."""

    def __init__(self, seed, monkeypatch):
        self.seed, self.tls, self._randn = seed, threading.local(), _RANDN
        monkeypatch.setattr(torch, "randn_like", self.randn_like)
        monkeypatch.setattr(torch, "randn", self.randn)

    def gen(self):
        if not hasattr(self.tls, "g"):
            self.tls.g = torch.Generator(device="cuda").manual_seed(self.seed)
        return self.tls.g

    def randn_like(self, t):
        assert t.is_cuda
        return self._randn(t.shape, generator=self.gen(), device=t.device, dtype=t.dtype)

    def randn(self, *size, **kw):
        if "generator" in kw or torch.device(kw.get("device") or "cpu").type != "cuda":
            return self._randn(*size, **kw)
        return self._randn(*size, generator=self.gen(), **kw)


def _run_args(world, n_rounds):
    return dict(height=H, width=W, n_frames=T, n_rounds=n_rounds, n_steps=STEPS, cond_aug=0.02)


@pytest.fixture(scope="module")
def rank_models(world):
    """A pipeline per thread rank, as every process of a real job builds its own (do_sample switches flags on the conditioner between rounds)."""
    from vista_amd import sample_utils as SU
    return [SU.init_model({"config": world["config"], "ckpt": world["ckpt"]}) for _ in range(3)]


def _sharded(world, rank_models, n_ranks, mode, monkeypatch, hip, eager=True):
    """run(shard=) on `n_ranks` thread ranks -> [(samples, samples_z, inputs)] per rank."""
    from vista_amd import parallel, sample
    from vista_amd.parallel import ThreadGroups, make_shard
    monkeypatch.setattr(parallel, "HIP_RESHARD", hip)
    _NoisePerThread(7, monkeypatch)
    groups, outs, errs = ThreadGroups(), [None] * n_ranks, []

    def rank_fn(rank):
        try:
            torch.cuda.set_device(0)
            shard = make_shard(T, n_ranks, rank, mode=mode, make_group=groups.make(rank))
            outs[rank] = sample.run(rank_models[rank], world["frames"], None, eager=eager, shard=shard, **_run_args(world, 2))
        except Exception:  # noqa: BLE001
            errs.append(traceback.format_exc())
            groups.abort()
    th = [threading.Thread(target=rank_fn, args=(r,)) for r in range(n_ranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs[0]
    return outs


@pytest.fixture(scope="module")
def unsharded(world, model):
    from vista_amd import sample
    mp = pytest.MonkeyPatch()
    try:
        _NoisePerThread(7, mp)
        return sample.run(model, world["frames"], None, eager=True, **_run_args(world, 2))
    finally:
        mp.undo()


@pytest.mark.parametrize("n_ranks,mode", [(2, "hybrid"), (3, "frames")])
def test_run_with_a_shard_over_thread_ranks(world, rank_models, unsharded, n_ranks, mode, monkeypatch):
    from vista_amd import sample_utils as SU
    made, make = [], SU.init_sampling
    monkeypatch.setattr(SU, "init_sampling", lambda **k: (made.append(make(**k)), made[-1])[1])
    on = _sharded(world, rank_models, n_ranks, mode, monkeypatch, hip=True, eager=False)   # eager=False: a shard forces the eager step all the same
    assert len(made) == n_ranks and all(s.graph is False and s.cfg_streams is False and s.shard is not None for s in made)
    assert sorted(s.shard.rank + (s.shard.cfg_half or 0) * s.shard.P for s in made) == list(range(n_ranks))
    frames = 2 * (T - 3) + 3
    assert on[0][0].shape == (frames, 3, H, W) and on[0][1].shape == (frames, 4, H // 8, W // 8) and on[0][2].shape == (T, 3, H, W)
    for r in range(1, n_ranks):
        for name, a, b in zip(("samples", "samples_z", "inputs"), on[r], on[0]):
            assert torch.equal(a, b), f"rank {r} ends with another {name} than rank 0"
    rel = rel_l2(on[0][1], unsharded[1])
    print(f"[parity] run(shard=) {n_ranks} thread ranks, {mode}: samples_z rel-L2 vs the unsharded run {rel:.3e}")
    assert rel <= BOUND and torch.equal(on[0][2], unsharded[2])
    off = _sharded(world, rank_models, n_ranks, mode, monkeypatch, hip=False)
    assert torch.equal(on[0][1], off[0][1]), "HIP packing and torch packing must give the same latents bit for bit"


# ---- real process groups ---------------------------------------------------------------------------------------------------------------------
def _cli_flags(world, save):
    return ["--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES", "--data_root", world["data_root"], "--anno_file",
            world["anno"], "--action", "traj", "--n_frames", str(T), "--height", str(H), "--width", str(W), "--n_steps", str(STEPS), "--cond_aug",
            "0.02", "--rand_gen", "--save", save]


def _child(cmd, env_extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return res


def _free_port():
    """A rendezvous port nobody holds right now (asked of the kernel, so two checkouts running the suite side by side do not collide)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _torchrun(n, *args):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port",
            str(_free_port()), WORKER, *args]


def _files(top):
    return sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs)


def test_two_gloo_processes_on_one_gpu_write_what_one_process_writes(world):
    """`sample.main` under torch.distributed.run, two ranks host-staged over gloo on GPU 0, against the single-process CLI."""
    from vista_amd import sample_utils as SU
    one, two, log = (str(world["dir"] / n) for n in ("mgpu_one", "mgpu_two", "mgpu_log"))
    os.makedirs(log)
    _child([sys.executable, "-m", "vista_amd.sample", *_cli_flags(world, one)], {}, timeout=600)
    res = _child(_torchrun(2, "cli", *_cli_flags(world, two)),
                 {"VISTA_DIST_BACKEND": "gloo", "VISTA_FORCE_DEVICE": "0", "VISTA_TEST_LOG": log}, timeout=900)
    assert _files(two) == _files(one) and len(_files(one)) == 2 * (T + 2)
    assert os.listdir(log) == ["rank0.log"], "only global rank 0 writes"
    calls = open(os.path.join(log, "rank0.log")).read().splitlines()
    assert len(calls) == len(set(calls)) == 6, calls          # (virtual, real) x (videos, grids, images), each once
    assert len(re.findall(r"^sample 0: load ", res.stdout, flags=re.M)) == 1, res.stdout[-3000:]
    for sub in ("virtual", "real"):
        for f in os.listdir(os.path.join(one, sub, "videos")):
            if f.endswith(".apng"):
                a, b = (SU.read_video_frames(os.path.join(top, sub, "videos", f)) for top in (one, two))
                assert a.shape == b.shape == (T, H, W, 3)


def test_front_door_through_a_one_rank_rccl_group(world, model):
    """run(shard=) with every exchange of the sharded step issued on a real RCCL process group of one rank (`always_exchange`)."""
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    out = str(world["dir"] / "rccl1_samples_z.pt")
    res = _child(_torchrun(1, "rccl1", *_cli_flags(world, str(world["dir"] / "unused"))),
                 {"VISTA_DIST_BACKEND": "nccl", "VISTA_TEST_OUT": out}, timeout=900)
    info = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    cc = info["collective_calls"]
    assert info["backend"] == "nccl" and cc["all_to_all"] >= 50 and cc["all_reduce_sum"] >= 10 and cc["all_gather_list"] >= 1, cc
    sample.seed_everything(23)   # the flags' default --seed, as the worker seeds
    frame_list, _, _, action = SU.get_sample(0, "NUSCENES", T, "traj", data_root=world["data_root"], anno_file=world["anno"])
    want = sample.run(model, frame_list, action, eager=True, **_run_args(world, 1))[1]
    got = torch.load(out)
    rel = rel_l2(got, want.cpu())
    print(f"[parity] front door over a one-rank RCCL group: samples_z rel-L2 vs the single-process run {rel:.3e}, collectives {cc}")
    assert got.shape == want.shape and rel <= BOUND
