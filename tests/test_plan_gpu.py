"""The planner on the MI355X: vk_candidate_frame_stats against the kernel it extends (bitwise), against float64 (tests/_plan_ref.py; 1e-5
relative, the bar tests/test_reward_frontdoor_gpu.py holds the same fp32 arithmetic to) and its selection rule; then vista_amd.plan.Planner and
the CLI on the tiny world of tests/test_frontdoor_gpu.py (T = 5, 128 x 256, 3 steps; 2 ensemble members, 2 scoring steps, 2 rounds), where every
comparison is bitwise."""
import itertools
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _plan_ref as R  # noqa: E402
from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: E402,F401  (fixtures, by import)

# ---- vk_candidate_frame_stats -------------------------------------------------------------------------------------------------------------------------
#        (K, E, T, C, h, w), t0
CASES = [((1, 2, 1, 4, 1, 1), 0),        # the smallest legal call
         ((3, 3, 7, 4, 7, 11), 3),       # odd hw: the scalar path
         ((2, 5, 5, 4, 16, 32), 0),      # the vector path
         ((2, 5, 5, 4, 16, 32), 3),
         ((2, 64, 2, 4, 8, 8), 1),       # the largest E
         ((2, 4, 4, 4, 72, 128), 3),     # the real latent frame
         ((2, 2, 2, 4, 130, 128), 0),    # more than 16 * 256 four-pixel groups per frame: the vector path's grid-stride loop
         ((2, 2, 2, 4, 67, 67), 1)]      # the same loop on the scalar path


def _members(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 3 + 1


def _same(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("shape,t0", CASES, ids=["x".join(map(str, s)) + f"-t0_{t}" for s, t in CASES])
def test_candidate_stats_equal_the_existing_kernel_bitwise_and_float64(shape, t0):
    from vista_amd import ops
    K, E, Tn, C, h, w = shape
    x = _members(shape, seed=sum(shape) + t0)
    xg = x.cuda()
    frame_sum, total, best, fmap = ops.candidate_frame_stats(xg, t0, want_map=True)
    assert frame_sum.shape == (K, Tn - t0) and frame_sum.dtype == torch.float64 and total.shape == (K,) and total.dtype == torch.float64
    assert best.dim() == 0 and best.dtype == torch.int32 and fmap.shape == (K, Tn - t0, h, w) and fmap.dtype == torch.float32
    assert frame_sum.is_cuda and total.is_cuda and best.is_cuda and fmap.is_cuda
    for k in range(K):
        one_sum, one_map = ops.ensemble_frame_stats(xg[k][:, t0:])
        assert torch.equal(frame_sum[k], one_sum) and torch.equal(fmap[k], one_map), f"candidate {k}: not the existing kernel's bits"
        acc = 0.0
        for v in frame_sum[k].tolist():
            acc += v
        assert float(total[k]) == acc, "total: the frame sums added left to right"
    var = R.variance(x, t0)
    want_sum, want_map = var.sum(dim=(2, 3, 4)), var.mean(dim=2)
    rel_sum = ((frame_sum.cpu() - want_sum).abs() / want_sum).max().item()
    rel_map = ((fmap.cpu().double() - want_map).abs() / want_map).max().item()
    print(f"[parity] candidate_frame_stats {shape} t0 {t0}: frame_sum {rel_sum:.2e}, map {rel_map:.2e} against float64")
    assert rel_sum <= 1e-5 and rel_map <= 1e-5
    assert int(best) == R.select(total.tolist()) == int(R.candidate_frame_stats(x, t0)[2])
    assert _same(ops.candidate_frame_stats(xg, t0, want_map=True), (frame_sum, total, best, fmap)), "a second call gives the same bits"
    plain = ops.candidate_frame_stats(xg, t0)
    assert plain[3] is None and _same(plain[:3], (frame_sum, total, best)), "want_map=False changes nothing else"


@pytest.mark.parametrize("shape,t0", [((3, 3, 4, 4, 7, 11), 1), ((3, 3, 4, 4, 16, 32), 1)], ids=["scalar", "vector"])
def test_selection_ties_nans_and_permutations(shape, t0):
    from vista_amd import ops
    nan = float("nan")
    x = _members(shape, seed=5)
    x[1] *= 2.0                    # candidate 1 disagrees most
    x[2] = x[0]                    # a copy of candidate 0 at index 2
    frame_sum, total, best, _ = ops.candidate_frame_stats(x.cuda(), t0)
    assert float(total[0]) == float(total[2]) < float(total[1]) and int(best) == 0, "the tie goes to the lowest index"
    # the frames before t0 are never read: a NaN there changes nothing
    y = x.clone()
    y[:, :, :t0] = nan
    assert _same(ops.candidate_frame_stats(y.cuda(), t0, want_map=True), ops.candidate_frame_stats(x.cuda(), t0, want_map=True))
    # a NaN in a scored frame: that candidate is never best
    y = x.clone()
    y[0, 1, 2, 3, 0, 0] = nan
    _, total_n, best_n, _ = ops.candidate_frame_stats(y.cuda(), t0)
    assert math.isnan(total_n[0]) and int(best_n) == 2 and torch.equal(total_n[1:], total[1:])
    y[2, 0, t0, 0, -1, -1] = nan
    assert int(ops.candidate_frame_stats(y.cuda(), t0)[2]) == 1, "the only candidate with a number, however large"
    y[1, 2, 3, 1, 1, 1] = nan
    _, total_n, best_n, _ = ops.candidate_frame_stats(y.cuda(), t0)
    assert int(best_n) == -1 and all(math.isnan(v) for v in total_n)
    # permuting the candidates permutes the totals bitwise, and best follows
    z = _members(shape, seed=6)
    for k in range(shape[0]):
        z[k] *= (1.0 + 0.5 * ((k + 1) % 3))     # distinct totals, the smallest in the middle
    fs, tot, b, _ = ops.candidate_frame_stats(z.cuda(), t0)
    assert len(set(tot.tolist())) == shape[0]
    for perm in itertools.permutations(range(shape[0])):
        fs_p, tot_p, b_p, _ = ops.candidate_frame_stats(z[list(perm)].cuda(), t0)
        assert torch.equal(tot_p, tot[list(perm)]) and torch.equal(fs_p, fs[list(perm)]) and perm[int(b_p)] == int(b), perm


def test_candidate_stats_refuse_what_they_cannot_take():
    from vista_amd import _lib, ops
    x = _members((2, 3, 4, 4, 4, 4)).cuda()
    for bad, t0 in ((x[:, :1], 0), (torch.zeros(1, 65, 1, 4, 2, 2).cuda(), 0), (x, -1), (x, 4), (x, 7), (x[:0], 0), (x[..., :0], 0), (x[:, :, :, :0], 0)):
        with pytest.raises(_lib.VistaHipError, match="-22"):
            ops.candidate_frame_stats(bad, t0)
    with pytest.raises(TypeError):
        ops.candidate_frame_stats(x.double(), 0)
    with pytest.raises(TypeError):
        ops.candidate_frame_stats(x.bfloat16(), 0)
    with pytest.raises(TypeError):
        ops.candidate_frame_stats(x, 1.0)
    with pytest.raises(ValueError):
        ops.candidate_frame_stats(x[0], 0)
    lib, p, s = _lib.load(), ops._p, ops._stream()
    rows = 2 * 4
    fs, tot = torch.zeros(rows, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.float64).cuda()
    best, ws = torch.zeros((), dtype=torch.int32).cuda(), torch.zeros(rows * ops.FRAME_STATS_BLOCKS, dtype=torch.float64).cuda()
    fmap = torch.zeros(rows * 16 + 4).cuda()

    def call(px=p(x), pfs=p(fs), ptot=p(tot), pbest=p(best), pmap=None, pws=p(ws), K=2, E=3, Tn=4, t0=0, C=4, hw=16):
        return lib.vk_candidate_frame_stats(px, pfs, ptot, pbest, pmap, pws, K, E, Tn, t0, C, hw, s)
    for null in ("px", "pfs", "ptot", "pbest", "pws"):
        assert call(**{null: None}) == -22, null
    for kw in (dict(K=0), dict(K=-1), dict(E=1), dict(E=65), dict(t0=-1), dict(t0=4), dict(t0=5), dict(Tn=0), dict(C=0), dict(hw=0), dict(hw=-4),
               dict(K=65536), dict(Tn=65536), dict(Tn=65540, t0=4)):
        assert call(**kw) == -22, kw
    # hw % 4 == 0 takes the 16-byte path only: a pointer off that boundary is refused, x's or the map's (an odd hw takes any)
    off = ops._p(x.view(-1)[1:])
    assert call(px=off) == -22 and call(pmap=ops._p(fmap[1:])) == -22
    assert call(pmap=p(fmap)) == 0 and call() == 0 and call(t0=3) == 0
    torch.cuda.synchronize()


# ---- Planner on the tiny world --------------------------------------------------------------------------------------------------------------------------
A = {"trajectory": torch.tensor([0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2])}
B = {"command": torch.tensor(2), "goal": torch.tensor([0.25, 0.75])}
ENS, SCORE_STEPS, SCORE_SEED = 2, 2, 5


def _session(model, world, eager, seed=7):
    from vista_amd import drive
    torch.manual_seed(seed)
    return drive.DriveSession(model, world["frames"], height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02, eager=eager)


def _planner(session, **kw):
    from vista_amd import plan
    return plan.Planner(session, ens_size=ENS, score_steps=SCORE_STEPS, score_seed=SCORE_SEED, **kw)


def _row(scores, k):
    return scores.reward[k], scores.mean_variance[k], scores.frame_variance[k]


def _rows_equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def planned(world, model):
    """Two planned rounds over [A, B] under graph replay and eagerly, computed once: {eager: (session, [CandidateScores, ...])}."""
    out = {}
    for eager in (False, True):
        s = _session(model, world, eager)
        p = _planner(s)
        out[eager] = (s, [p.step([A, B])[1] for _ in range(2)])
    return out


@pytest.mark.parametrize("eager", [False, True], ids=["graph", "eager"])
def test_replaying_the_chosen_actions_gives_the_planned_rollout(world, model, planned, eager):
    """Scoring leaves behind neither a moved random stream nor a stale conditioning buffer in a captured graph: a fresh session under the same
    seed, stepped with the chosen actions and no planner, ends with the same bits."""
    from vista_amd import drive, plan
    s, scores = planned[eager]
    assert s.rounds == 2 and s.samples_z.shape[0] == 2 * (T - 3) + 3
    for r, sc in enumerate(scores):
        assert isinstance(sc, plan.CandidateScores) and sc.best in (0, 1) and sc.t0 == (1 if r == 0 else 3) and sc.map is None
        assert sc.reward.shape == (2,) and sc.frame_variance.shape == (2, T - sc.t0) and (sc.frame_variance > 0).all()
        assert sc.best == int(torch.argmax(sc.reward)) and torch.equal(sc.reward, torch.exp(-sc.mean_variance))
        assert not torch.equal(sc.frame_variance[0], sc.frame_variance[1]), "two actions, two scores"
    chosen = [[A, B][sc.best] for sc in scores]
    assert [list(a) for a in s.actions] == [list(a) for a in chosen]
    replay = _session(model, world, eager)
    for a in chosen:
        assert isinstance(replay.step(a), drive.RoundResult)
    assert torch.equal(replay.samples_z, s.samples_z) and torch.equal(replay.frames(), s.frames())


def test_planning_under_graph_replay_equals_planning_eagerly(planned):
    (fast, fast_scores), (slow, slow_scores) = planned[False], planned[True]
    assert torch.equal(fast.samples_z, slow.samples_z) and torch.equal(fast.frames(), slow.frames())
    for a, b in zip(fast_scores, slow_scores):
        assert a.best == b.best and torch.equal(a.reward, b.reward) and torch.equal(a.frame_variance, b.frame_variance)


@pytest.fixture(scope="module")
def stepped_once(world, model):
    s = _session(model, world, False, seed=9)
    s.step(A)
    return s


def _untouched(session, planner, actions):
    before = (session.rounds, None if session._sample is None else session._sample.clone(), [t.clone() for t in session._latents], session._z.clone(),
              session._cond_frames.clone(), session.inputs.clone(), torch.get_rng_state(), torch.cuda.get_rng_state())
    scores = planner.score(actions)
    assert session.rounds == before[0] and (before[1] is None or torch.equal(session._sample, before[1]))
    assert len(session._latents) == len(before[2]) and all(torch.equal(a, b) for a, b in zip(session._latents, before[2]))
    assert torch.equal(session._z, before[3]) and torch.equal(session._cond_frames, before[4]) and torch.equal(session.inputs, before[5])
    assert torch.equal(torch.get_rng_state(), before[6]) and torch.equal(torch.cuda.get_rng_state(), before[7]), "scoring moved the caller's random stream"
    return scores


def test_scoring_leaves_the_session_and_the_generators_alone_and_orders_do_not_matter(world, model, stepped_once):
    """In round 0 and in a later round: score() changes nothing; [A, A] gives two equal rows and best 0; [A, B] and [B, A] give permuted rows
    and choose the same action."""
    from vista_amd import plan
    fresh = _session(model, world, False, seed=9)
    for session in (fresh, stepped_once.fork()):
        p = _planner(session)
        torch.manual_seed(123)
        torch.randn(3, device="cuda")          # (generators somewhere in the middle of their streams)
        ab = _untouched(session, p, [A, B])
        if session.rounds:
            assert torch.equal(session.samples_z, stepped_once.samples_z)
        aa = _untouched(session, p, [A, A])
        ba = _untouched(session, p, [B, A])
        assert _rows_equal(_row(aa, 0), _row(aa, 1)) and aa.best == 0
        assert _rows_equal(_row(aa, 0), _row(ab, 0)), "a candidate's score does not depend on its neighbours"
        assert _rows_equal(_row(ab, 0), _row(ba, 1)) and _rows_equal(_row(ab, 1), _row(ba, 0)) and not _rows_equal(_row(ab, 0), _row(ab, 1))
        assert ab.best == 1 - ba.best
        assert _rows_equal(_row(_untouched(session, p, [A, B]), 1), _row(ab, 1)), "a second score() draws the same noise"
        reseeded = plan.Planner(session, ens_size=ENS, score_steps=SCORE_STEPS, score_seed=SCORE_SEED + 1)
        assert not torch.equal(reseeded.score([A, B]).frame_variance, ab.frame_variance), "another score_seed, another ensemble"


def test_round_zero_scores_equal_estimate_under_the_planners_seeds(world, model):
    """frame_variance of every candidate == reward_utils.estimate(...).frame_variance[1:], with estimate's noise_fn reseeding to the planner's
    member seeds and its sampler the planner's (score_steps steps, the session's guider)."""
    from vista_amd import reward_utils, sample
    from vista_amd import sample_utils as SU
    s = _session(model, world, False, seed=7)
    scores = _planner(s).score([A, B])
    member = itertools.count()

    def noise_fn(like):
        torch.manual_seed(SCORE_SEED + 0 * ENS + next(member))
        return torch.randn_like(like)
    sampler = SU.init_sampling(guider=s.guider, steps=SCORE_STEPS, cfg_scale=2.5, num_frames=T)
    sampler.graph = sampler.cfg_streams = True
    base = dict(s._scalars, cond_aug=0.02, cond_frames_without_noise=s.inputs[:1], cond_frames=s._cond_frames)
    torch.manual_seed(7)
    torch.randn_like(s.inputs[:1])             # the generator where the session's encoder found it
    reports = reward_utils.estimate(s.inputs, model, sampler, [dict(base, **A), dict(base, **B)], num_frames=T, ensemble_size=ENS,
                                    force_uc_zero_embeddings=sample.UC_KEYS, initial_cond_indices=[0], noise_fn=noise_fn, want_map=False)
    assert next(member) == ENS
    for k, rep in enumerate(reports):
        assert float(rep.frame_variance[0]) == 0.0 and torch.equal(scores.frame_variance[k], rep.frame_variance[1:]), k
        # estimate averages over all T frames, the planner over the T - 1 predicted ones
        assert abs(rep.mean_variance * T / (T - 1) - float(scores.mean_variance[k])) <= 1e-12 * rep.mean_variance


def test_a_scored_round_decodes_once_and_conditions_once_per_candidate(world, model, stepped_once):
    s = stepped_once.fork()
    p = _planner(s)
    calls = {"decode": 0, "condition": 0}
    decode, condition = model.decode_first_stage, model.condition_fn
    had = {k: model.__dict__.get(k) for k in ("decode_first_stage", "condition_fn")}
    model.decode_first_stage = lambda *a, **k: (calls.__setitem__("decode", calls["decode"] + 1), decode(*a, **k))[1]
    model.condition_fn = lambda *a, **k: (calls.__setitem__("condition", calls["condition"] + 1), condition(*a, **k))[1]
    try:
        p.score([A, B])
        assert calls == {"decode": 1, "condition": 2}, "scoring K = 2: one tail decode, K conditioner runs"
        calls.update(decode=0, condition=0)
        result, scores = p.step([A, B])
        assert calls == {"decode": 2, "condition": 3}, "a planned round: one decode for scoring + one for the commit, K + 1 conditioner runs"
    finally:
        for k, old in had.items():
            if old is None:
                delattr(model, k)
            else:
                setattr(model, k, old)
    assert result.round == 1 and s.rounds == 2 and list(result.action) == list([A, B][scores.best])


def test_cli_writes_drives_files_and_a_record_whose_chosen_actions_replay_through_drive(world, model):
    """`python -m vista_amd.plan` once, as a fresh child process; then vista_amd.drive --script with the record's chosen actions writes the same
    pictures."""
    import subprocess
    from vista_amd import drive
    save, save2 = str(world["dir"] / "plan_out"), str(world["dir"] / "plan_replay")
    entries = [{"command": 1}, "scene", {"goal": [400, 600]}]
    cands = str(world["dir"] / "candidates.json")
    with open(cands, "w") as f:
        json.dump({"candidates": entries}, f)
    flags = ["--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES", "--data_root", world["data_root"], "--anno_file",
             world["anno"], "--action", "traj", "--n_frames", str(T), "--height", str(H), "--width", str(W), "--n_steps", str(STEPS), "--cond_aug",
             "0.02", "--rand_gen"]
    cmd = [sys.executable, "-m", "vista_amd.plan"] + flags + ["--n_rounds", "2", "--candidates", cands, "--ens_size", str(ENS), "--score_steps",
                                                              str(SCORE_STEPS), "--score_seed", "3", "--hud", "--save", save]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    n = 2 * (T - 3) + 3
    assert sorted(os.listdir(save)) == ["hud", "plan.jsonl", "real", "virtual"]
    for sub, count in (("virtual", n), ("real", T)):
        assert sorted(os.listdir(os.path.join(save, sub))) == ["grids", "images", "videos"]
        assert sorted(os.listdir(os.path.join(save, sub, "images"))) == [f"NUSCENES_000000_{i:04}.png" for i in range(count)]
    assert os.listdir(os.path.join(save, "hud", "videos")) in (["NUSCENES_000000.apng"], ["NUSCENES_000000.mp4"])
    lines = open(os.path.join(save, "plan.jsonl")).read().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert tuple(rec) == drive.RECORD_KEYS and (rec["index"], rec["seed"], rec["action"], rec["n_rounds"]) == (0, 23, "traj", 2)
    assert sorted(rec["timings"]) == ["decode", "hud", "load", "sample", "save", "score"] and all(v >= 0 for v in rec["timings"].values())
    for r, rnd in enumerate(rec["rounds"]):
        assert list(rnd) == ["round", "action", "frames", "candidates", "chosen"] and rnd["round"] == r and rnd["frames"] == list(drive.round_range(r, T))
        assert [c["action"] for c in rnd["candidates"]] == entries and rnd["action"] == entries[rnd["chosen"]]
        rewards = [c["reward"] for c in rnd["candidates"]]
        assert all(0.0 < v < 1.0 for v in rewards) and rnd["chosen"] == rewards.index(max(rewards))
        assert all(len(c["frame_variance"]) == T - (1 if r == 0 else 3) for c in rnd["candidates"])
    script = str(world["dir"] / "chosen.json")
    with open(script, "w") as f:
        json.dump({"rounds": [rnd["action"] for rnd in rec["rounds"]]}, f)
    assert drive.main(flags + ["--script", script, "--save", save2]) == 0
    for i in range(n):
        name = os.path.join("virtual", "images", f"NUSCENES_000000_{i:04}.png")
        assert open(os.path.join(save, name), "rb").read() == open(os.path.join(save2, name), "rb").read(), name
