"""Host side of the planner (vista_amd/plan.py) and the float64 definition of vk_candidate_frame_stats (tests/_plan_ref.py): flags, the
candidates file and its refusals, the header / ctypes / ops agreement, the record a planned round writes (with ops.candidate_frame_stats
replaced by the definition), and the definition's own known answers. No GPU. Every comparison is exact unless it says otherwise."""
import ctypes
import json
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _plan_ref as R  # noqa: E402


def test_flags_are_drives_without_script_plus_four():
    from vista_amd import drive, plan
    base = {a.dest: a for a in drive.parse_args()._actions if a.dest not in ("help", "script")}
    ours = {a.dest: a for a in plan.parse_args()._actions if a.dest != "help"}
    assert set(ours) == set(base) | {"candidates", "ens_size", "score_steps", "score_seed"} and "script" not in ours
    for name, a in base.items():
        b = ours[name]
        assert (b.option_strings, b.default, b.type, b.nargs, b.const, b.help) == (a.option_strings, a.default, a.type, a.nargs, a.const, a.help), name
    got = {k: (ours[k].default, ours[k].type) for k in ("candidates", "ens_size", "score_steps", "score_seed")}
    assert got == {"candidates": (None, str), "ens_size": (5, int), "score_steps": (10, int), "score_seed": (0, int)}
    opt = plan.parse_args().parse_args(["--candidates", "c.json", "--hud", "--n_rounds", "3"])
    assert (opt.candidates, opt.hud, opt.n_rounds, opt.ens_size, opt.score_steps, opt.score_seed) == ("c.json", True, 3, 5, 10, 0)
    assert plan.n_rounds_given(["--candidates", "c.json"]) is None and plan.n_rounds_given(["--n_round=2", "--score_steps", "4"]) == 2
    with pytest.raises(SystemExit):
        plan.parse_args().parse_args(["--script", "s.json"])


ENTRIES = [{"command": 1}, {"trajectory": [[0.5, 0.0], [1.0, 0.0], [1.5, 0.1], [2.0, 0.2]], "goal": [400, 600]}, {}, "scene"]


def test_both_forms_of_the_candidates_file_parse():
    from vista_amd import plan
    assert plan.parse_candidates({"candidates": ENTRIES}) == ("candidates", ENTRIES)
    assert plan.parse_candidates({"rounds": [ENTRIES[:2], ENTRIES[2:], [{}]]}) == ("rounds", [ENTRIES[:2], ENTRIES[2:], [{}]])


def test_cli_refuses_before_any_model_is_built(tmp_path, monkeypatch):
    from vista_amd import plan
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused run"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def file(obj):
        path = tmp_path / f"c{len(os.listdir(tmp_path))}.json"
        path.write_text(json.dumps(obj))
        return str(path)
    shared, two = file({"candidates": ENTRIES}), file({"rounds": [ENTRIES[:2], ENTRIES[2:]]})
    with pytest.raises(ValueError, match="--candidates FILE is required"):
        plan.main([])
    for obj, message in (({"candidates": []}, r"candidates \(every round\) is empty"), ({"rounds": []}, "\"rounds\" is empty"),
                         ({"rounds": [[{}], []]}, "candidates round 1 is empty"), ({"candidates": [{}], "fps": 3}, "the one key \"candidates\""),
                         ({"script": [{}]}, "the one key \"candidates\""), ([{}], "the one key \"candidates\""),
                         ({"candidates": {"command": 1}}, r"candidates \(every round\): expected a list of entries, got dict"),
                         ({"rounds": [[{}], {}]}, "candidates round 1: expected a list of entries, got dict"),
                         ({"candidates": [{}, {"brake": 1}]}, r"candidates \(every round\) candidate 1: unknown key 'brake'"),
                         ({"rounds": [[{}], [{}, {}, {"command": 1.5}]]}, "candidates round 1 candidate 2: command must be one integer"),
                         ({"rounds": [[{"goal": [1600, 450]}]]}, "candidates round 0 candidate 0: goal .* outside the open 1600 x 900"),
                         ({"rounds": [["free"]]}, "candidates round 0 candidate 0: expected an object of action keys")):
        with pytest.raises(ValueError, match=message):
            plan.main(["--candidates", file(obj)])
    with pytest.raises(ValueError, match="--n_rounds 3 disagrees with --candidates .* 2 rounds"):
        plan.main(["--candidates", two, "--n_rounds", "3"])
    with pytest.raises(ValueError, match="--n_rounds 0: a rollout has at least one round"):
        plan.main(["--candidates", shared, "--n_rounds", "0"])
    for flags, message in ((["--ens_size", "1"], "--ens_size 1: .* 2 .. 64 members"), (["--ens_size", "65"], "--ens_size 65: .* 2 .. 64 members"),
                           (["--score_steps", "0"], "--score_steps 0: .* at least one denoising step")):
        with pytest.raises(ValueError, match=message):
            plan.main(["--candidates", shared] + flags)
    # what drive.plan_run refuses through check_sizes, for the file's round count
    with pytest.raises(ValueError, match="carries 3 frames"):
        plan.main(["--candidates", two, "--n_frames", "3"])
    with pytest.raises(ValueError, match="carries 3 frames"):
        plan.main(["--candidates", shared, "--n_rounds", "2", "--n_frames", "3"])
    with pytest.raises(ValueError, match="attention level"):
        plan.main(["--candidates", shared, "--height", "576", "--width", "1088"])
    with pytest.raises(ValueError, match="n_frames 40"):
        plan.main(["--candidates", shared, "--n_frames", "40"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE 2: vista_amd.plan runs on one GPU"):
        plan.main(["--candidates", shared])
    monkeypatch.delenv("WORLD_SIZE")
    argv = ["--candidates", shared, "--n_rounds", "3", "--n_frames", "5", "--height", "128", "--width", "256"]
    assert plan.plan_run(plan.parse_args().parse_args(argv), argv) == [ENTRIES] * 3
    argv = ["--candidates", two, "--n_rounds", "2"]
    assert plan.plan_run(plan.parse_args().parse_args(argv), argv) == [ENTRIES[:2], ENTRIES[2:]]
    assert plan.plan_run(plan.parse_args().parse_args(argv[:2]), argv[:2]) == [ENTRIES[:2], ENTRIES[2:]], "the file's length decides"
    for bad in (dict(ens_size=1), dict(ens_size=65), dict(score_steps=0)):
        with pytest.raises(ValueError):
            plan.Planner(None, **bad)


def test_header_signature_table_and_ops_agree_on_the_new_entry():
    from vista_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    decl = re.search(r"^int vk_candidate_frame_stats\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const float* x", "double* frame_sum", "double* total", "int32_t* best", "float* map", "double* partial_ws", "int32_t K",
                    "int32_t E", "int32_t T", "int32_t t0", "int32_t C", "int32_t hw", "void* stream"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["vk_candidate_frame_stats"] == [vp] * 6 + [i32] * 6 + [vp]
    assert int(re.search(r"#define VK_FRAME_STATS_BLOCKS (\d+)", hdr).group(1)) == ops.FRAME_STATS_BLOCKS == 16
    assert _lib.ABI_VERSION == 9 and "vk_abi_version() stays 9" in hdr, "the entry is additive"
    assert os.path.exists(_lib.LIB_PATH) and hasattr(ctypes.CDLL(_lib.LIB_PATH), "vk_candidate_frame_stats")
    assert "reward.hip" in __import__("vista_amd.build", fromlist=["SOURCES"]).SOURCES
    # the op checks types and shapes before anything reaches the library
    with pytest.raises(TypeError):
        ops.candidate_frame_stats(torch.zeros(2, 2, 2, 4, 2, 2, dtype=torch.float64), 0)
    with pytest.raises(_lib.VistaHipError, match="no CPU fallback"):
        ops.candidate_frame_stats(torch.zeros(2, 2, 2, 4, 2, 2), 0)


# ---- the definition's own known answers ---------------------------------------------------------------------------------------------------------------
def test_reference_is_float64_variance_frames_added_in_order():
    K, E, T, C, h, w = 3, 4, 5, 4, 3, 2
    x = torch.randn(K, E, T, C, h, w, generator=torch.Generator().manual_seed(1)) * 3 + 1
    for t0 in (0, 3, 4):
        frame_sum, total, best, fmap = R.candidate_frame_stats(x, t0, want_map=True)
        assert frame_sum.shape == (K, T - t0) and frame_sum.dtype == total.dtype == torch.float64 and best.dtype == torch.int32 and best.dim() == 0
        assert fmap.shape == (K, T - t0, h, w) and fmap.dtype == torch.float32
        for k in range(K):
            for t in range(t0, T):
                elems = x[k, :, t].double().reshape(E, -1)
                want = sum(float(((elems[:, i] - elems[:, i].mean()) ** 2).sum() / (E - 1)) for i in range(elems.shape[1]))
                assert abs(float(frame_sum[k, t - t0]) - want) <= 1e-12 * want
            acc = 0.0
            for v in frame_sum[k].tolist():
                acc += v
            assert float(total[k]) == acc
        assert int(best) == min(range(K), key=lambda k: float(total[k]))
        assert R.candidate_frame_stats(x, t0)[3] is None
    # frames before t0 are not part of anything
    y = x.clone()
    y[:, :, :3] = float("nan")
    a, b = R.candidate_frame_stats(x, 3, True), R.candidate_frame_stats(y, 3, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # two members one apart: variance 0.5 per element, exactly
    z = torch.zeros(1, 2, 2, 4, 2, 2)
    z[0, 1] = 1.0
    frame_sum, total, best, fmap = R.candidate_frame_stats(z, 0, True)
    assert frame_sum.tolist() == [[8.0, 8.0]] and total.tolist() == [16.0] and int(best) == 0 and (fmap == 0.5).all()


def test_reference_selection_rule():
    nan = float("nan")
    assert R.select([3.0, 1.0, 2.0]) == 1 and R.select([1.0, 1.0, 0.5, 0.5]) == 2 and R.select([2.0]) == 0
    assert R.select([nan, 4.0, nan, 4.0]) == 1 and R.select([0.0, nan]) == 0 and R.select([nan, nan]) == -1 and R.select([nan]) == -1
    assert R.select([nan, float("inf")]) == 1 and R.select([float("inf"), 1e300]) == 1


# ---- the record of a planned round ----------------------------------------------------------------------------------------------------------------------
def _members(K=3, seed=2):
    x = torch.randn(K, 3, 5, 4, 2, 2, generator=torch.Generator().manual_seed(seed))
    for k in range(K):
        x[k] *= (K - k)       # candidate K - 1 disagrees least
    return x


class _Session:
    """What plan_rounds touches of a DriveSession."""
    guider, cfg_scale, n_frames = "VanillaCFG", 2.5, 5

    def __init__(self):
        self.stepped = []
        self.sampler = type("S", (), {"graph": False})()

    @property
    def rounds(self):
        return len(self.stepped)

    def step(self, action):
        self.stepped.append(action)


def test_scores_and_record_layout_with_the_reference_patched_in(monkeypatch):
    from vista_amd import ops, plan
    monkeypatch.setattr(ops, "candidate_frame_stats", R.candidate_frame_stats)
    x = _members()
    s = plan.scores_of(x, 3)
    assert isinstance(s, plan.CandidateScores) and s._fields == ("best", "reward", "mean_variance", "frame_variance", "t0", "map")
    assert (s.best, s.t0, s.map) == (2, 3, None) and s.reward.shape == s.mean_variance.shape == (3,) and s.frame_variance.shape == (3, 2)
    assert s.reward.dtype == s.mean_variance.dtype == s.frame_variance.dtype == torch.float64
    var = R.variance(x, 3)
    for k in range(3):
        assert abs(float(s.mean_variance[k]) - float(var[k].mean())) <= 1e-12 * float(var[k].mean()), "the mean is over the scored frames only"
        assert float(s.reward[k]) == math.exp(-float(s.mean_variance[k]))
        assert torch.equal(s.frame_variance[k], R.candidate_frame_stats(x, 3)[0][k] / 16)
    assert plan.scores_of(x, 3, want_map=True).map.shape == (3, 2, 2, 2)

    entries = [{"command": 1}, "scene", {"command": 2}, {}]
    extra = plan.round_extra(entries, [0, 2, 3], s, "the scene's annotation has no speed / angle record")
    assert list(extra) == ["candidates", "chosen"] and extra["chosen"] == 3 and len(extra["candidates"]) == 4
    assert extra["candidates"][1] == {"action": "scene", "reward": None, "reason": "the scene's annotation has no speed / angle record"}
    for k, i in ((0, 0), (2, 1), (3, 2)):
        c = extra["candidates"][k]
        assert list(c) == ["action", "reward", "mean_variance", "frame_variance"] and c["action"] == entries[k]
        assert (c["reward"], c["mean_variance"], c["frame_variance"]) == (float(s.reward[i]), float(s.mean_variance[i]), s.frame_variance[i].tolist())
    json.dumps(extra, allow_nan=False)
    # a candidate whose ensemble went NaN is never chosen and reports null; all NaN is an error that names the round
    x[2, 1, 4, 0, 0, 0] = float("nan")
    s = plan.scores_of(x, 3)
    assert s.best == 1 and plan.require_best(s, 0) == 1
    extra = plan.round_extra(entries[:3], [0, 1, 2], s, None)
    assert extra["chosen"] == 1 and extra["candidates"][2]["reward"] is None and extra["candidates"][2]["frame_variance"][0] is not None
    assert extra["candidates"][2]["frame_variance"][1] is None and extra["candidates"][1]["reward"] > extra["candidates"][0]["reward"]
    json.dumps(extra, allow_nan=False)
    x[:, 0, 3] = float("nan")
    s = plan.scores_of(x, 3)
    assert s.best == -1
    with pytest.raises(RuntimeError, match="round 4 of NUSCENES scene 7: .* 3 candidates is NaN"):
        plan.require_best(s, 4, "NUSCENES scene 7")
    with pytest.raises(RuntimeError, match="plan: round 4: "):
        plan.require_best(s, 4)


def test_planned_rounds_step_the_chosen_entries_and_drop_what_the_scene_cannot_supply(monkeypatch):
    from vista_amd import ops, plan
    monkeypatch.setattr(ops, "candidate_frame_stats", R.candidate_frame_stats)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    asked = []

    def score(self, actions, want_map=False):
        asked.append(actions)
        return plan.scores_of(_members(len(actions), seed=len(asked)), 1 if self.session.rounds == 0 else 3)
    monkeypatch.setattr(plan.Planner, "score", score)
    opt = plan.parse_args().parse_args(["--action", "steer", "--ens_size", "3", "--score_steps", "2"])
    rounds = [[{"command": 1}, "scene", {"command": 2}], ["scene", {}]]
    session, timings = _Session(), {}
    chosen, extras = plan.plan_rounds(opt, session, rounds, {}, timings, "NUSCENES scene 0")      # {}: the annotation has no steer record
    assert chosen == [{"command": 2}, {}] and [e["chosen"] for e in extras] == [2, 1] and list(timings) == ["score"] and timings["score"] >= 0
    assert [len(a) for a in asked] == [2, 1] and [list(a) for a in session.stepped] == [["command"], []]
    assert int(session.stepped[0]["command"]) == 2
    assert extras[0]["candidates"][1] == extras[1]["candidates"][0] == {"action": "scene", "reward": None,
                                                                        "reason": "the scene's annotation has no speed / angle record"}
    assert len(extras[0]["candidates"][0]["frame_variance"]) == 4 and len(extras[1]["candidates"][1]["frame_variance"]) == 2
    with pytest.raises(RuntimeError, match="round 1 of NUSCENES scene 3: no candidate is left"):
        plan.plan_rounds(opt, _Session(), [[{}], ["scene", "scene"]], {}, {}, "NUSCENES scene 3")
    # a scene that supplies the action, and a dataset without annotations (None): "scene" is a candidate
    assert plan.unsupplied("steer", {"speed": torch.ones(4)}) is None and plan.unsupplied("steer", None) is None
    assert plan.unsupplied("free", None) is None and "goal point" in plan.unsupplied("goal", {})
    asked.clear()
    session = _Session()
    chosen, extras = plan.plan_rounds(opt, session, [["scene", {}]], {"speed": torch.ones(4)}, {}, "x")
    assert len(asked[0]) == 2 and list(asked[0][0]) == ["speed"] and chosen == [{}] and extras[0]["candidates"][0]["reward"] is not None
    # Planner.step: score, then the session's own step under the best
    p = plan.Planner(_Session(), ens_size=3, score_steps=2)
    assert p.sampler.graph is False and p.sampler.num_steps == 2
    result, scores = p.step([{"command": torch.tensor(1)}, {}])
    assert result is None and scores.best == 1 and p.session.stepped == [{}]
