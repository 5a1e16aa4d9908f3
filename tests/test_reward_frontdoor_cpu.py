"""Host side of the reward front door (vista_amd/reward.py, vista_amd/reward_utils.estimate): CLI flags, candidate actions, the member
assignment of an ensemble-parallel run, the host logic of `estimate` with torch restatements in place of the kernels, the record writer. No GPU."""
import json
import math
import os
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_cli_flags_equal_the_reference_fixture():
    from vista_amd import reward
    parser = reward.parse_args()
    golden = json.load(open(os.path.join(GOLD, "reward_cli_flags.json")))["flags"]
    assert {f["name"]: f["default"] for f in golden if f["name"] in ("n_steps", "ens_size", "action", "rand_gen")} == \
        {"n_steps": 10, "ens_size": 5, "action": "traj", "rand_gen": True}
    actions = {a.dest: a for a in parser._actions if a.dest != "help"}
    kinds = {"str": str, "int": int, "float": float}
    for flag in golden:
        a = actions.pop(flag["name"])
        assert a.option_strings == ["--" + flag["name"]] and a.default == flag["default"] and type(a.default) is type(flag["default"]), flag
        if flag["kind"] in kinds:
            assert a.type is kinds[flag["kind"]] and a.nargs is None, flag
        else:
            assert a.nargs == 0 and a.const is (flag["kind"] == "store_true"), flag
    assert sorted(actions) == ["anno_file", "ckpt", "config", "data_root", "eager", "heat_max", "save_maps"], "what this package adds to the reference's flags"
    assert all(actions[k].default is None for k in ("anno_file", "ckpt", "config", "data_root", "heat_max"))
    assert actions["eager"].default is False and actions["save_maps"].default is False and actions["heat_max"].type is float
    opt = parser.parse_args(["--rand_gen", "--save_maps", "--heat_max", "0.25", "--ens_size", "3", "--action", "traj,free"])
    assert opt.rand_gen is False and opt.save_maps is True and opt.heat_max == 0.25 and opt.ens_size == 3 and opt.action == "traj,free"


def test_member_slots_cover_every_member_once():
    from vista_amd.reward_utils import member_slots
    assert member_slots(5, 1) == [[0, 1, 2, 3, 4]]
    assert member_slots(5, 2) == [[0, 2, 4], [1, 3]]
    assert member_slots(5, 3) == [[0, 3], [1, 4], [2]]
    assert member_slots(5, 5) == [[0], [1], [2], [3], [4]]
    for world in (1, 2, 3, 5):
        slots = member_slots(5, world)
        assert len(slots) == world and sorted(e for s in slots for e in s) == list(range(5))
        assert all(e % world == r for r, s in enumerate(slots) for e in s)
    with pytest.raises(ValueError, match=r"world 6 > ensemble_size 5"):
        member_slots(5, 6)
    with pytest.raises(ValueError, match="at least two"):
        member_slots(1, 1)


def _dataset(tmp_path):
    root = tmp_path / "nuscenes"
    (root / "cam").mkdir(parents=True)
    names = [f"cam/f{i}.jpg" for i in range(3)]
    for n in names:
        (root / n).write_bytes(b"x")
    scenes = [
        {"frames": names, "traj": [0.0, 0.0, 1.0, 0.5, 2.0, 1.0, 3.0, 1.5, 4.0, 2.0], "cmd": 2, "speed": [], "angle": [], "z": -1.0, "goal": [800.0, 450.0]},
        {"frames": names, "traj": [0.0] * 10, "cmd": 1, "speed": [1.0, 2.0, 3.0, 4.0, 5.0], "angle": [0.0, 78.0, 0.0, 0.0, 0.0], "z": 2.0, "goal": [800.0, 450.0]},
    ]
    anno = tmp_path / "anno.json"
    anno.write_text(json.dumps(scenes))
    return str(root), str(anno), names


def test_action_lists_and_candidates(tmp_path):
    from vista_amd import reward
    assert reward.parse_actions("traj") == ["traj"]
    assert reward.parse_actions("traj,cmd,free") == ["traj", "cmd", "free"]
    assert reward.parse_actions(" steer , goal ") == ["steer", "goal"]
    with pytest.raises(ValueError, match="Unsupported action mode fly"):
        reward.parse_actions("traj,fly")
    for bad in ("", "traj,,free", "traj,traj"):
        with pytest.raises(ValueError):
            reward.parse_actions(bad)
    root, anno, names = _dataset(tmp_path)
    frames, idx, total, cands = reward.scene_candidates(0, "NUSCENES", 2, ["traj", "cmd", "free", "steer", "goal"], data_root=root, anno_file=anno)
    assert frames == [os.path.join(root, n) for n in names[:2]] and (idx, total) == (0, 2)
    assert [c[0] for c in cands] == ["traj", "cmd", "free", "steer", "goal"]
    assert list(cands[0][1]) == ["trajectory"] and torch.equal(cands[1][1]["command"], torch.tensor(2)) and cands[2][1:] == ({}, None)
    assert cands[3][1] is None and "speed" in cands[3][2] and cands[4][1] is None and "goal" in cands[4][2]
    _, idx, _, cands = reward.scene_candidates(3, "NUSCENES", 2, ["steer", "goal"], data_root=root, anno_file=anno)   # 3 -> scene 1
    assert idx == 1 and sorted(cands[0][1]) == ["angle", "speed"] and cands[0][2] is None and list(cands[1][1]) == ["goal"]
    (tmp_path / "pics").mkdir()
    (tmp_path / "pics" / "a.png").write_bytes(b"x")
    frames, idx, total, cands = reward.scene_candidates(0, "IMG", 3, ["traj", "free"], data_root=str(tmp_path / "pics"))
    assert len(frames) == 3 and cands == [("traj", {}, None), ("free", {}, None)], "a dataset without annotations runs action-free, like the reference"


def test_cli_refuses_what_cannot_run_before_building_anything(monkeypatch):
    from vista_amd import reward
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused run"))
    with pytest.raises(ValueError, match="attention level"):
        reward.main(["--height", "576", "--width", "1088"])
    with pytest.raises(ValueError, match="n_frames 40"):
        reward.main(["--n_frames", "40"])
    with pytest.raises(ValueError, match=r"--ens_size 1.*at least two"):
        reward.main(["--ens_size", "1"])
    with pytest.raises(ValueError, match="Unsupported action mode fly"):
        reward.main(["--action", "traj,fly"])
    monkeypatch.setenv("WORLD_SIZE", "6")
    with pytest.raises(ValueError, match=r"world 6 > ensemble_size 5"):
        reward.main([])


# ---- estimate: host logic with torch restatements of the two kernels ------------------------------------------------------------------------
T, C, HL, WL = 4, 4, 3, 5


def _cpu_frame_stats(x, want_map=True):
    """What vk_ensemble_frame_stats computes, in torch."""
    var = x.double().var(dim=0, unbiased=True)            # (T, C, h, w)
    return var.sum(dim=(1, 2, 3)), (var.mean(dim=1).float() if want_map else None)


def _cpu_variance_sum(x):
    return float(x.double().var(dim=0, unbiased=True).sum())


class _Stub:
    """A pipeline, a conditioner and a sampler that are cheap functions of their inputs; the sampler scales its input in place like the real one."""

    def __init__(self):
        from vista_amd.sample_utils import VistaPipeline
        self.pipe = VistaPipeline(None, None, encode_fn=self.encode, scale_factor=1.0)
        self.encodes, self.conditions, self.noise_seen = 0, [], []

    def encode(self, x):
        self.encodes += 1
        return x * 0.5

    def get_condition(self, model, value_dict, num_frames, force_uc, device):
        self.conditions.append(value_dict["k"])
        return {"k": value_dict["k"]}, {"k": 0.0}

    def sampler(self, denoiser, x, cond, uc=None, cond_frame=None, cond_mask=None):
        self.noise_seen.append((cond["k"], x.clone()))
        x.mul_(3.0)                                        # (prepare_sampling_loop scales the noise in place)
        return torch.sin(x * cond["k"]) + 0.1 * x + cond_frame * (1 + cond_mask.view(-1, 1, 1, 1))


def _noise_fn(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda like: torch.randn(like.shape, generator=g, dtype=like.dtype)


@pytest.fixture
def kernels_in_torch(monkeypatch):
    from vista_amd import reward_utils
    monkeypatch.setattr(reward_utils.ops, "ensemble_frame_stats", _cpu_frame_stats, raising=False)
    monkeypatch.setattr(reward_utils.ops, "ensemble_variance_sum", _cpu_variance_sum)


def _images():
    return torch.randn(T, C, HL, WL, generator=torch.Generator().manual_seed(1))


def _estimate(stub, value_dicts, seed=5, E=3, **kw):
    from vista_amd import reward_utils
    return reward_utils.estimate(_images(), stub.pipe, stub.sampler, value_dicts, T, ensemble_size=E, device="cpu", get_condition=stub.get_condition,
                                 noise_fn=_noise_fn(seed), fused=False, **kw)


def test_estimate_shares_the_noise_between_candidates(kernels_in_torch):
    stub = _Stub()
    reports = _estimate(stub, [{"k": 1.0}, {"k": 2.5}])
    assert stub.encodes == 1 and stub.conditions == [1.0, 2.5], "one encode, one conditioner run per candidate"
    assert [k for k, _ in stub.noise_seen] == [1.0] * 3 + [2.5] * 3
    first, second = [n for k, n in stub.noise_seen if k == 1.0], [n for k, n in stub.noise_seen if k == 2.5]
    fresh = _noise_fn(5)
    draws = [fresh(_images()) for _ in range(3)]
    for a, b, d in zip(first, second, draws):
        assert torch.equal(a, b) and torch.equal(a, d), "E draws in member order, the same tensors for every candidate"
    assert not torch.equal(first[0], first[1])
    assert len(reports) == 2 and reports[0].mean_variance != reports[1].mean_variance
    for rep in reports:
        assert rep.reward.dim() == 0 and rep.reward.device.type == "cpu" and isinstance(rep.mean_variance, float)
        assert rep.frame_variance.shape == (T,) and rep.frame_variance.dtype == torch.float64 and rep.map.shape == (T, HL, WL)
        assert float(rep.frame_variance[0]) == 0.0 and (rep.frame_variance[1:] > 0).all(), "sample[0] = z[0]: the members agree on frame 0"
        assert float(rep.map[0].abs().max()) == 0.0
        assert torch.equal(rep.frame_reward, torch.exp(-rep.frame_variance)) and float(rep.frame_reward[0]) == 1.0
        assert abs(float(rep.reward) - math.exp(-float(rep.frame_variance.mean()))) <= 1e-12
        assert abs(rep.mean_variance - float(rep.map.double().mean())) <= 1e-6 * rep.mean_variance
    assert _estimate(_Stub(), {"k": 1.0}, want_map=False)[0].map is None, "a single dict is one candidate"


def test_estimate_of_one_candidate_equals_do_sample(kernels_in_torch, monkeypatch):
    from vista_amd import reward_utils
    seen = []

    def spy(x):
        seen.append(_cpu_variance_sum(x) / x[0].numel())
        return _cpu_variance_sum(x)
    monkeypatch.setattr(reward_utils.ops, "ensemble_variance_sum", spy)
    stub = _Stub()
    _, reward = reward_utils.do_sample(_images(), stub.pipe, stub.sampler, {"k": 1.7}, T, ensemble_size=4, device="cpu",
                                       get_condition=stub.get_condition, noise_fn=_noise_fn(9), fused=False)
    rep = _estimate(_Stub(), {"k": 1.7}, seed=9, E=4)[0]
    neg_log = seen[0]                                      # do_sample's -log(reward) before the float32 tensor rounds it
    assert neg_log > 0 and abs(rep.mean_variance - neg_log) <= 1e-10 * neg_log
    assert abs(float(rep.reward) - float(reward)) <= 2.0 ** -23 * float(reward), "do_sample's tensor is float32"


def test_estimate_over_thread_ranks_equals_one_rank(kernels_in_torch):
    from vista_amd import reward_utils
    from vista_amd.parallel import ThreadGroups
    one = _estimate(_Stub(), [{"k": 1.0}, {"k": 2.5}], E=5)
    for world in (2, 3):
        groups, outs, stubs, errs = ThreadGroups(), [None] * world, [_Stub() for _ in range(world)], []

        def rank_fn(rank):
            try:
                comm = groups.make(rank)(list(range(world)))
                outs[rank] = _estimate(stubs[rank], [{"k": 1.0}, {"k": 2.5}], E=5, members=(rank, world), comm=comm)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                groups.abort()
        th = [threading.Thread(target=rank_fn, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs[0]
        for rank in range(world):
            assert len(stubs[rank].noise_seen) == 2 * len(reward_utils.member_slots(5, world)[rank]), "a rank samples its own members only"
            for a, b in zip(outs[rank], one):
                assert a.mean_variance == b.mean_variance and torch.equal(a.frame_variance, b.frame_variance) and torch.equal(a.map, b.map)
                assert torch.equal(a.reward, b.reward)
    with pytest.raises(ValueError, match=r"world 6 > ensemble_size 5"):
        _estimate(_Stub(), {"k": 1.0}, E=5, members=(0, 6), comm=object())
    with pytest.raises(ValueError, match="comm="):
        _estimate(_Stub(), {"k": 1.0}, E=5, members=(0, 2))


def test_record_writer_keeps_null_candidates(tmp_path):
    from vista_amd import frontdoor, reward
    from vista_amd.reward_utils import RewardReport
    fv = torch.tensor([0.0, 0.25, 0.5], dtype=torch.float64)
    rep = RewardReport(reward=torch.tensor(math.exp(-0.25), dtype=torch.float64), mean_variance=0.25, frame_variance=fv, frame_reward=torch.exp(-fv))
    cands = [("traj", {"trajectory": torch.zeros(8)}, None), ("steer", None, "the scene's annotation has no speed / angle record")]
    record = reward.make_record(7, ["a/f0.jpg", "a/f1.jpg"], 23, 5, 10, cands, [rep], {"load": 0.5, "sample": 8.123456})
    path = frontdoor.append_record(str(tmp_path / "out"), reward.RECORDS_NAME, record)
    frontdoor.append_record(str(tmp_path / "out"), reward.RECORDS_NAME, record)
    lines = open(path).read().splitlines()
    assert path.endswith("rewards.jsonl") and len(lines) == 2 and lines[0] == lines[1]
    got = json.loads(lines[0])
    assert got == {"index": 7, "frames": ["a/f0.jpg"], "seed": 23, "ens_size": 5, "n_steps": 10, "timings": {"load": 0.5, "sample": 8.1235},
                   "actions": [{"action": "traj", "reward": math.exp(-0.25), "mean_variance": 0.25, "frame_variance": [0.0, 0.25, 0.5]},
                               {"action": "steer", "reward": None, "reason": "the scene's annotation has no speed / angle record"}]}


def test_frame_zero_is_stated_exactly_although_the_fp32_mean_leaves_a_residue(kernels_in_torch, monkeypatch):
    """(x + x + x) / 3 in fp32 is not always x: the kernel's sum over a frame whose members are equal can be ~1e-17 instead of 0."""
    from vista_amd import reward_utils

    def with_residue(x, want_map=True):
        fs, m = _cpu_frame_stats(x, want_map)
        fs[0] += 7.9e-17
        if m is not None:
            m[0] += 1e-19
        return fs, m
    monkeypatch.setattr(reward_utils.ops, "ensemble_frame_stats", with_residue)
    rep = _estimate(_Stub(), {"k": 1.0})[0]
    assert float(rep.frame_variance[0]) == 0.0 and float(rep.frame_reward[0]) == 1.0 and float(rep.map[0].abs().max()) == 0.0
    assert (rep.frame_variance[1:] > 0).all() and float(rep.map[1:].min()) > 0.0
