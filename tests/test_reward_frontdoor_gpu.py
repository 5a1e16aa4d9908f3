"""The reward front door on the MI355X: the two kernels of csrc/reward.hip against torch fp64 / numpy float32, `reward.run` and `reward.main` on
the tiny world of tests/test_frontdoor_gpu.py (5 frames, 128 x 256, 3 steps, 3 ensemble members), and the ensemble-parallel form over thread
ranks. Bounds: the per-element variance is fp32 arithmetic summed in fp64 -- 1e-5 relative against torch's fp64 variance, the bar of
tests/test_reward_gpu.py for the same arithmetic; two fp64 sums of the same fp32 terms in another order agree to 1e-10; everything else is
bitwise."""
import json
import math
import os
import threading
import traceback

import numpy as np
import pytest
import torch

from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)
from tests.test_frontdoor_mgpu_gpu import _NoisePerThread, rank_models  # noqa: F401

pytestmark = pytest.mark.gpu
ENS = 3


# ---- vk_ensemble_frame_stats ----------------------------------------------------------------------------------------------------------------
STAT_SHAPES = [(2, 1, 4, 1, 1), (3, 7, 4, 7, 11), (5, 5, 4, 16, 32), (64, 2, 4, 8, 8), (16, 2, 4, 72, 128)]


def _ensemble(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 3 + 1


@pytest.mark.parametrize("shape", STAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_stats_equal_torch_fp64(shape):
    from vista_amd import ops
    x = _ensemble(shape, seed=sum(shape))
    E, Tn, C, h, w = shape
    frame_sum, fmap = ops.ensemble_frame_stats(x.cuda())
    assert frame_sum.shape == (Tn,) and frame_sum.dtype == torch.float64 and frame_sum.is_cuda
    assert fmap.shape == (Tn, h, w) and fmap.dtype == torch.float32 and fmap.is_cuda
    var = x.double().var(0, unbiased=True)                          # (T, C, h, w)
    want_sum, want_map = var.sum(dim=(1, 2, 3)), var.mean(dim=1)
    rel_sum = ((frame_sum.cpu() - want_sum).abs() / want_sum).max().item()
    rel_map = ((fmap.cpu().double() - want_map).abs() / want_map).max().item()
    total = ops.ensemble_variance_sum(x.cuda())
    rel_total = abs(float(frame_sum.sum()) - total) / total
    print(f"[parity] ensemble_frame_stats {shape}: frame_sum {rel_sum:.2e}, map {rel_map:.2e}, sum of frames vs ensemble_variance_sum {rel_total:.2e}")
    assert rel_sum <= 1e-5 and rel_map <= 1e-5 and rel_total <= 1e-10
    again_sum, again_map = ops.ensemble_frame_stats(x.cuda())
    assert torch.equal(again_sum, frame_sum) and torch.equal(again_map, fmap), "fixed-order reduction must be bitwise repeatable"
    only_sum, no_map = ops.ensemble_frame_stats(x.cuda(), want_map=False)
    assert no_map is None and torch.equal(only_sum, frame_sum)


@pytest.mark.parametrize("shape", [(3, 5, 4, 7, 11), (5, 5, 4, 16, 32), (4, 5, 4, 72, 128)], ids=["odd_hw", "tiny_latent", "full_latent"])
def test_a_frame_sum_does_not_depend_on_the_frames_around_it(shape):
    from vista_amd import ops
    x = _ensemble(shape, seed=3).cuda()
    all_sum, all_map = ops.ensemble_frame_stats(x)
    two_sum, two_map = ops.ensemble_frame_stats(x[:, 0:2])
    assert torch.equal(all_sum[0:2], two_sum) and torch.equal(all_map[0:2], two_map)
    last_sum, _ = ops.ensemble_frame_stats(x[:, 4:5])
    assert torch.equal(all_sum[4:5], last_sum)
    tail = ops.ensemble_frame_stats(x[:, 1:])[0]
    assert torch.equal(tail, all_sum[1:])


def test_frame_stats_refuse_what_they_cannot_take():
    from vista_amd import _lib, ops
    x = _ensemble((3, 2, 4, 4, 4)).cuda()
    with pytest.raises(_lib.VistaHipError, match="-22"):
        ops.ensemble_frame_stats(x[:1])
    with pytest.raises(_lib.VistaHipError, match="-22"):
        ops.ensemble_frame_stats(torch.zeros(65, 1, 4, 2, 2).cuda())
    with pytest.raises(TypeError):
        ops.ensemble_frame_stats(x.double())
    with pytest.raises(TypeError):
        ops.ensemble_frame_stats(x.bfloat16())
    with pytest.raises(ValueError):
        ops.ensemble_frame_stats(x[0])
    lib, p, s = _lib.load(), ops._p, ops._stream()
    fs, ws = torch.zeros(2, dtype=torch.float64).cuda(), torch.zeros(2 * ops.FRAME_STATS_BLOCKS, dtype=torch.float64).cuda()
    assert lib.vk_ensemble_frame_stats(None, p(fs), None, p(ws), 3, 2, 4, 16, s) == -22
    assert lib.vk_ensemble_frame_stats(p(x), None, None, p(ws), 3, 2, 4, 16, s) == -22
    assert lib.vk_ensemble_frame_stats(p(x), p(fs), None, None, 3, 2, 4, 16, s) == -22
    for E, Tn, C, hw in ((3, 0, 4, 16), (3, 2, 0, 16), (3, 2, 4, 0), (3, -1, 4, 16)):
        assert lib.vk_ensemble_frame_stats(p(x), p(fs), None, p(ws), E, Tn, C, hw, s) == -22
    assert lib.vk_ensemble_frame_stats(p(x), p(fs), None, p(ws), 3, 2, 4, 16, s) == 0
    torch.cuda.synchronize()


# ---- vk_heat_overlay_u8 ----------------------------------------------------------------------------------------------------------------------
HEAT_COLOUR = np.array([255.0, 32.0, 0.0], dtype=np.float32)


def _numpy_overlay(frames, fmap, cell, vmax, alpha):
    """The kernel's expression in numpy float32, one rounding per operation."""
    x = frames.numpy()
    f = 255.0 * (x + 1.0) / 2.0                                      # what frames_to_u8(real=True) forms before its cast
    m = np.repeat(np.repeat(fmap.numpy(), cell, axis=1), cell, axis=2)[:, None]
    inv = np.float32(1) / np.float32(vmax)
    a = np.float32(alpha) * np.minimum(np.float32(1), m * inv)
    k = HEAT_COLOUR[None, :, None, None]
    out = f + a * (k - f)
    assert f.dtype == a.dtype == out.dtype == np.float32
    return out.astype(np.uint8).transpose(0, 2, 3, 1)


def _frames_and_map(n, Hh, Ww, cell, seed, vmax):
    g = torch.Generator().manual_seed(seed)
    frames = torch.rand(n, 3, Hh, Ww, generator=g) * 2.0 - 1.0
    frames.view(-1)[:3] = torch.tensor([-1.0, 1.0, 0.0])
    fmap = torch.rand(n, Hh // cell, Ww // cell, generator=g) * (2.0 * vmax)   # half of the cells above vmax
    flat = fmap.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 3)]] = 0.0
    return frames, fmap


@pytest.mark.parametrize("n,Hh,Ww,cell", [(1, 8, 8, 8), (3, 16, 24, 8), (2, 128, 256, 8), (2, 6, 10, 2)])
def test_heat_overlay_equals_numpy_float32(n, Hh, Ww, cell):
    from vista_amd import ops
    vmax, alpha = 0.37, 0.6
    frames, fmap = _frames_and_map(n, Hh, Ww, cell, seed=Hh + Ww, vmax=vmax)
    maps = [fmap] if fmap.numel() > 1 else [torch.full_like(fmap, v) for v in (0.0, 0.5 * vmax, 2.0 * vmax)]   # a one-cell map: one value at a time
    plain = ops.frames_to_u8(frames.cuda(), real=True).cpu().numpy()
    for m in maps:
        got = ops.heat_overlay_u8(frames.cuda(), m.cuda(), vmax, alpha=alpha)
        assert got.dtype == torch.uint8 and got.shape == (n, Hh, Ww, 3)
        got = got.cpu().numpy()
        want = _numpy_overlay(frames, m, cell, vmax, alpha)
        assert np.array_equal(got, want), int((got != want).sum())
        zero = np.repeat(np.repeat(m.numpy() == 0, cell, axis=1), cell, axis=2)
        assert np.array_equal(got[zero], plain[zero]), "a cell without disagreement shows the frame as frames_to_u8 writes it"
        hot = np.repeat(np.repeat(m.numpy() >= vmax, cell, axis=1), cell, axis=2)
        if hot.any():
            assert not np.array_equal(got[hot], plain[hot])
    if fmap.numel() > 1:
        assert (fmap == 0).any() and (fmap > vmax).any() and ((fmap > 0) & (fmap < vmax)).any()
        full = ops.heat_overlay_u8(frames.cuda(), fmap.cuda(), vmax, alpha=1.0).cpu().numpy()
        assert np.array_equal(full, _numpy_overlay(frames, fmap, cell, vmax, 1.0))


def test_heat_overlay_refuses_what_it_cannot_take():
    from vista_amd import _lib, ops
    frames, fmap = torch.zeros(2, 3, 16, 24).cuda(), torch.ones(2, 2, 3).cuda()
    with pytest.raises(_lib.VistaHipError, match="-22"):
        ops.heat_overlay_u8(frames, fmap, 1.0, alpha=1.5)
    with pytest.raises(_lib.VistaHipError, match="-22"):
        ops.heat_overlay_u8(frames, fmap, 1.0, alpha=-0.1)
    with pytest.raises(ValueError):
        ops.heat_overlay_u8(frames, torch.ones(2, 3, 5).cuda(), 1.0)      # 16 x 24 frames are not tiled by a 3 x 5 map
    with pytest.raises(ValueError):
        ops.heat_overlay_u8(frames, fmap, 0.0)
    with pytest.raises(TypeError):
        ops.heat_overlay_u8(frames.double(), fmap, 1.0)
    lib, p, s = _lib.load(), ops._p, ops._stream()
    out = torch.zeros(2, 16, 24, 3, dtype=torch.uint8).cuda()
    assert lib.vk_heat_overlay_u8(p(frames), p(fmap), p(out), 2, 16, 24, 5, 1.0, 0.5, s) == -22      # H % cell
    assert lib.vk_heat_overlay_u8(p(frames), p(fmap), p(out), 2, 16, 24, 16, 1.0, 0.5, s) == -22     # W % cell
    assert lib.vk_heat_overlay_u8(p(frames), p(fmap), p(out), 2, 16, 24, 0, 1.0, 0.5, s) == -22
    assert lib.vk_heat_overlay_u8(p(frames), None, p(out), 2, 16, 24, 8, 1.0, 0.5, s) == -22
    assert lib.vk_heat_overlay_u8(p(frames), p(fmap), None, 2, 16, 24, 8, 1.0, 0.5, s) == -22
    for inv in (float("inf"), float("nan"), -1.0):
        assert lib.vk_heat_overlay_u8(p(frames), p(fmap), p(out), 2, 16, 24, 8, inv, 0.5, s) == -22
    assert lib.vk_heat_overlay_u8(p(frames), p(fmap), p(out), 2, 16, 24, 8, 1.0, float("nan"), s) == -22
    assert lib.vk_heat_overlay_u8(p(frames), p(fmap), p(out), 2, 16, 24, 8, 1.0, 0.5, s) == 0
    torch.cuda.synchronize()


# ---- reward.run / reward.main on the tiny world -----------------------------------------------------------------------------------------------
TRAJ = {"trajectory": torch.tensor([0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2])}


def _run(model, world, actions, eager, seed=7, **kw):
    from vista_amd import reward
    torch.manual_seed(seed)
    return reward.run(model, world["frames"], actions, height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02, ens_size=ENS, eager=eager, **kw)


def _same(a, b):
    return (torch.equal(a.reward, b.reward) and a.mean_variance == b.mean_variance and torch.equal(a.frame_variance, b.frame_variance)
            and torch.equal(a.frame_reward, b.frame_reward) and (a.map is None) == (b.map is None) and (a.map is None or torch.equal(a.map, b.map)))


def test_graph_replay_equals_eager_bitwise_and_one_graph_per_half_serves_every_member(world, model):
    timings = {}
    fast = _run(model, world, [TRAJ], eager=False, want_map=True, timings=timings)
    cache = model.model.diffusion_model.__dict__["_hipgraph_cache"]
    assert len(cache) == 2, "one captured graph per guidance half, replayed by every member"
    graphs = [id(g["graph"]) for g in cache.values()]
    slow = _run(model, world, [TRAJ], eager=True, want_map=True)
    assert len(fast) == len(slow) == 1 and _same(fast[0], slow[0])
    rep = fast[0]
    assert rep.reward.dim() == 0 and rep.reward.device.type == "cpu" and rep.frame_variance.shape == (T,) and rep.frame_variance.dtype == torch.float64
    assert rep.map.shape == (T, H // 8, W // 8) and rep.map.is_cuda and rep.map.dtype == torch.float32
    assert float(rep.frame_variance[0]) == 0.0 and float(rep.map[0].abs().max()) == 0.0 and (rep.frame_variance[1:] > 0).all()
    assert abs(float(rep.reward) - math.exp(-float(rep.frame_variance.mean()))) <= 1e-12
    assert 0.0 < float(rep.reward) < 1.0 and math.isfinite(rep.mean_variance)
    assert sorted(timings) == ["condition", "encode", "load", "sample"] and all(v >= 0 for v in timings.values())
    again = _run(model, world, [TRAJ, {}], eager=False, want_map=True)
    assert len(cache) == 2 and [id(g["graph"]) for g in cache.values()] == graphs, "later candidates and runs replay the same graphs"
    assert _same(again[0], rep)
    other = _run(model, world, [TRAJ], eager=False, seed=8)
    assert other[0].map is None and other[0].mean_variance != rep.mean_variance, "another seed, another ensemble"


def test_two_candidates_share_one_set_of_noise(world, model, monkeypatch):
    drawn, real = [], torch.randn_like
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: (drawn.append(tuple(t.shape)), real(t, **k))[1])
    both = _run(model, world, [TRAJ, {}], eager=False)
    latent = (T, 4, H // 8, W // 8)
    assert drawn.count(latent) == ENS and len(drawn) == ENS + 1, drawn       # + the augmentation noise of the conditioning frame
    assert not _same(both[0], both[1]) and both[0].mean_variance != both[1].mean_variance
    drawn.clear()
    _run(model, world, [{}], eager=False)
    assert drawn.count(latent) == ENS and len(drawn) == ENS + 1, "one candidate draws as many"


def test_estimate_of_one_candidate_equals_do_sample(world, model, monkeypatch):
    """Same noise_fn, same sampler settings: reward_utils.do_sample (vk_ensemble_variance_sum) against estimate (vk_ensemble_frame_stats)."""
    from vista_amd import ops, reward_utils, sample
    from vista_amd import sample_utils as SU
    images = SU.load_img_seq(world["frames"], H, W)
    vd = dict(SU.init_embedder_options(set(e.input_key for e in model.conditioner.embedders)), cond_frames_without_noise=images[:1], cond_aug=0.0,
              cond_frames=images[:1], **TRAJ)
    seen, real = [], ops.ensemble_variance_sum
    monkeypatch.setattr(reward_utils.ops, "ensemble_variance_sum", lambda x: (seen.append((real(x), x[0].numel())), seen[-1][0])[1])

    def noise_fn():
        g = torch.Generator(device="cuda").manual_seed(11)
        return lambda like: torch.randn(like.shape, generator=g, device=like.device, dtype=like.dtype)

    def sampler():
        s = SU.init_sampling(guider="VanillaCFG", steps=STEPS, cfg_scale=2.5, num_frames=T)
        s.graph = s.cfg_streams = True
        return s
    kw = dict(num_frames=T, ensemble_size=ENS, force_uc_zero_embeddings=sample.UC_KEYS, initial_cond_indices=[0])
    torch.manual_seed(3)                                   # (the first stage's posterior sample draws from the process generator)
    _, reward = reward_utils.do_sample(images, model, sampler(), dict(vd), noise_fn=noise_fn(), **kw)
    torch.manual_seed(3)
    rep = reward_utils.estimate(images, model, sampler(), dict(vd), noise_fn=noise_fn(), **kw)[0]
    neg_log = seen[0][0] / seen[0][1]                      # do_sample's -log(reward) before its float32 tensor rounds it
    print(f"[parity] estimate vs do_sample: -log reward {rep.mean_variance!r} vs {neg_log!r}")
    assert neg_log > 0 and abs(rep.mean_variance - neg_log) <= 1e-10 * neg_log
    assert abs(float(rep.reward) - float(reward)) <= 2.0 ** -23 * float(reward), "do_sample's tensor is float32"


def test_cli_writes_the_record_the_real_frames_and_the_heat_videos(world, model, capsys):
    from vista_amd import ops, reward
    from vista_amd import sample_utils as SU
    save = str(world["dir"] / "reward_out")
    flags = ["--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES", "--data_root", world["data_root"], "--anno_file",
             world["anno"], "--n_frames", str(T), "--height", str(H), "--width", str(W), "--n_steps", str(STEPS), "--cond_aug", "0.02",
             "--ens_size", str(ENS), "--rand_gen", "--save", save]
    assert reward.main(flags + ["--action", "traj,free,steer", "--save_maps"]) == 0
    out = capsys.readouterr().out
    lines = open(os.path.join(save, "rewards.jsonl")).read().splitlines()
    assert len(lines) == 1
    record = json.loads(lines[0])
    assert sorted(record) == ["actions", "ens_size", "frames", "index", "n_steps", "seed", "timings"]
    assert (record["index"], record["seed"], record["ens_size"], record["n_steps"], record["frames"]) == (0, 23, ENS, STEPS, [world["frames"][0]])
    assert [a["action"] for a in record["actions"]] == ["traj", "free", "steer"]
    assert record["actions"][2] == {"action": "steer", "reward": None, "reason": "the scene's annotation has no speed / angle record"}
    assert sorted(record["timings"]) == ["condition", "encode", "load", "sample", "save"]

    reward.seed_everything(23)   # the CLI's default --seed
    frame_list, index, total, cands = reward.scene_candidates(0, "NUSCENES", T, ["traj", "free", "steer"], data_root=world["data_root"], anno_file=world["anno"])
    inputs = []
    reports = reward.run(model, frame_list, [a for _, a, _ in cands if a is not None], height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02,
                         ens_size=ENS, want_map=True, inputs_out=inputs)
    assert (index, total) == (0, 1) and len(reports) == 2
    for got, rep in zip(record["actions"], reports):
        assert got["reward"] == float(rep.reward) and got["mean_variance"] == rep.mean_variance
        assert got["frame_variance"] == [float(v) for v in rep.frame_variance] and got["frame_variance"][0] == 0.0
    assert f"reward 0: traj {float(reports[0].reward):.6f}, free {float(reports[1].reward):.6f}, steer null | " in out

    real = os.path.join(save, "real")
    assert sorted(os.listdir(real)) == ["grids", "images", "videos"]
    assert sorted(os.listdir(os.path.join(real, "images"))) == [f"NUSCENES_000000_{i:04}.png" for i in range(T)]
    assert os.listdir(os.path.join(real, "grids")) == ["NUSCENES_000000.png"]
    assert os.listdir(os.path.join(real, "videos")) in (["NUSCENES_000000.apng"], ["NUSCENES_000000.mp4"])
    assert sorted(os.listdir(os.path.join(save, "heat"))) == ["free", "traj"], "one heat video per candidate that ran"
    vmax = max(float(rep.map.max()) for rep in reports)
    for name, rep in zip(("traj", "free"), reports):
        videos = os.listdir(os.path.join(save, "heat", name, "videos"))
        assert videos in (["NUSCENES_000000.apng"], ["NUSCENES_000000.mp4"])
        if videos[0].endswith(".apng"):
            frames = SU.read_video_frames(os.path.join(save, "heat", name, "videos", videos[0]))
            assert frames.shape == (T, H, W, 3)
            assert np.array_equal(frames, ops.heat_overlay_u8(inputs[0], rep.map, vmax, alpha=reward.HEAT_ALPHA).cpu().numpy())
            assert np.array_equal(frames[0], ops.frames_to_u8(inputs[0][:1], real=True)[0].cpu().numpy()), "frame 0 carries no disagreement"
    # without --save_maps: a second record in the same file, no heat tree of its own
    save2 = str(world["dir"] / "reward_out_plain")
    assert reward.main(flags[:-1] + [save2, "--action", "free"]) == 0
    assert sorted(os.listdir(save2)) == ["real", "rewards.jsonl"]
    plain = json.loads(open(os.path.join(save2, "rewards.jsonl")).read())
    assert [a["action"] for a in plain["actions"]] == ["free"] and 0.0 < plain["actions"][0]["reward"] < 1.0


# ---- ensemble-parallel over thread ranks --------------------------------------------------------------------------------------------------------
def _one_rank(model, world, monkeypatch):
    _NoisePerThread(7, monkeypatch)        # (a new instance: a fresh generator, seeded alike, for this thread too)
    from vista_amd import reward
    return reward.run(model, world["frames"], [TRAJ, {}], height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02, ens_size=ENS, eager=True,
                      want_map=True)


def _distance(a, b):
    """The largest relative difference between two lists of reports: frame variances and maps."""
    worst = 0.0
    for x, y in zip(a, b):
        scale = float(y.frame_variance.abs().max())
        worst = max(worst, float((x.frame_variance - y.frame_variance).abs().max()) / scale,
                    float((x.map.double() - y.map.double()).norm() / y.map.double().norm()), abs(x.mean_variance - y.mean_variance) / y.mean_variance)
    return worst


@pytest.fixture(scope="module")
def one_rank_twice(world, model):
    mp = pytest.MonkeyPatch()
    try:
        return _one_rank(model, world, mp), _one_rank(model, world, mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_members_over_thread_ranks_give_the_one_rank_reports(world, rank_models, one_rank_twice, n_ranks, monkeypatch):
    """Each thread rank owns a pipeline and a CUDA generator, all seeded alike, samples the members e % n_ranks == rank and meets the others in one
    all_reduce per candidate. Thread ranks launch every step's kernels from the host (eager=True): they share one process, and a graph capture of
    one thread does not tolerate the launches of another; graph replay against eager is pinned bitwise above. The bound is the measured
    difference between two one-rank runs + 25 % -- zero, i.e. bitwise, when those agree bit for bit."""
    from vista_amd import reward
    from vista_amd.parallel import ThreadGroups
    first, second = one_rank_twice
    floor = _distance(second, first)
    print(f"[determinism] two one-rank reward runs differ by {floor:.3e}" + (" (bitwise equal)" if all(_same(a, b) for a, b in zip(first, second)) else ""))
    _NoisePerThread(7, monkeypatch)
    groups, outs, errs = ThreadGroups(), [None] * n_ranks, []

    def rank_fn(rank):
        try:
            torch.cuda.set_device(0)
            comm = groups.make(rank)(list(range(n_ranks)))
            outs[rank] = reward.run(rank_models[rank], world["frames"], [TRAJ, {}], height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02,
                                    ens_size=ENS, eager=True, want_map=True, members=(rank, n_ranks), comm=comm)
        except Exception:  # noqa: BLE001
            errs.append(traceback.format_exc())
            groups.abort()
    th = [threading.Thread(target=rank_fn, args=(r,)) for r in range(n_ranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs[0]
    for r in range(1, n_ranks):
        assert len(outs[r]) == 2 and all(_same(a, b) for a, b in zip(outs[r], outs[0])), f"rank {r} ends with other reports than rank 0"
    got = _distance(outs[0], first)
    print(f"[parity] reward members over {n_ranks} thread ranks vs one rank: {got:.3e} (run-to-run floor {floor:.3e})")
    assert got <= 1.25 * floor
    if floor == 0.0:
        assert all(_same(a, b) for a, b in zip(outs[0], first))
