"""The drive front door on the MI355X (vista_amd/drive.py): a DriveSession against sample.run and against do_sample driven through its
get_condition hook, graph replay against eager, fork(), and the CLI's files. The tiny world of tests/test_frontdoor_gpu.py: T = 5, 128 x 256,
3 steps. Every comparison is bitwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _overlay_ref as R  # noqa: E402
from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: E402,F401  (fixtures, by import)

A = {"trajectory": torch.tensor([0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2])}
B = {"command": torch.tensor(2), "goal": torch.tensor([0.25, 0.75])}
NAMES = ("samples", "samples_z", "inputs")


def _session(model, world, eager, seed, guider="TrianglePredictionGuider"):
    from vista_amd import drive
    torch.manual_seed(seed)
    return drive.DriveSession(model, world["frames"], height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02, eager=eager, guider=guider)


def _drive(model, world, actions, eager, seed, guider="TrianglePredictionGuider"):
    s = _session(model, world, eager, seed, guider)
    results = [s.step(a) for a in actions]
    return s, results


def _run(model, world, n_rounds, eager, seed, action):
    from vista_amd import sample
    torch.manual_seed(seed)
    return sample.run(model, world["frames"], action, height=H, width=W, n_frames=T, n_rounds=n_rounds, n_steps=STEPS, cond_aug=0.02, eager=eager)


@pytest.fixture(scope="module")
def constant_a(world, model):
    """sample.run under the constant action A for R = 2 and 3 (graph replay), computed once."""
    return {R_: _run(model, world, R_, False, 7, A) for R_ in (2, 3)}


@pytest.fixture(scope="module")
def scripted(world, model):
    """The session stepped with [A, B, {}] under graph replay, computed once."""
    return _drive(model, world, [A, B, {}], False, 7)


@pytest.mark.parametrize("eager", [False, True], ids=["graph", "eager"])
@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_session_equals_sample_run_bitwise(world, model, constant_a, rounds, eager):
    from vista_amd import drive
    guider = "VanillaCFG" if rounds == 1 else "TrianglePredictionGuider"
    s, results = _drive(model, world, [A] * rounds, eager, 7, guider)
    want = constant_a[rounds] if rounds > 1 and not eager else _run(model, world, rounds, eager, 7, A)
    got = (s.frames(), s.samples_z, s.inputs)
    assert got[1].shape[0] == rounds * (T - 3) + 3 == s.rounds * (T - 3) + 3
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    for r, res in enumerate(results):
        assert isinstance(res, drive.RoundResult) and (res.round, res.lo, res.hi) == (r,) + drive.round_range(r, T)
        assert torch.equal(res.latents, want[1][res.lo:res.hi]) and list(res.action) == ["trajectory"]


def test_a_script_changes_the_rounds_it_names_and_equals_do_sample_through_its_hook(world, model, constant_a, scripted):
    """[A, B, {}]: round 0 is the constant-A run's, rounds 1 and 2 are not; the whole rollout is do_sample's when its get_condition hook swaps in
    the r-th round's action on its r-th call."""
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    s, results = scripted
    z = s.samples_z
    base = constant_a[3][1]
    assert torch.equal(z[:T], base[:T]), "round 0 ran under A"
    for r in (1, 2):
        lo, hi = results[r].lo, results[r].hi
        assert not torch.equal(z[lo:hi], base[lo:hi]), f"round {r} ran under another action"
    assert [list(r.action) for r in results] == [["trajectory"], ["command", "goal"], []]

    actions, calls = [A, B, {}], []

    def hook(mdl, value_dict, num_frames, force_uc_zero_embeddings, device):
        vd = {k: v for k, v in value_dict.items() if k not in ("command", "trajectory", "speed", "angle", "goal")}
        vd.update(actions[len(calls)])
        calls.append(sorted(vd))
        return SU.get_condition(mdl, vd, num_frames, force_uc_zero_embeddings, device)
    torch.manual_seed(7)
    images = SU.load_img_seq(world["frames"], H, W, "cuda")
    vd = SU.init_embedder_options(set(e.input_key for e in model.conditioner.embedders))
    vd.update(cond_frames_without_noise=images[:1], cond_aug=0.02, cond_frames=images[:1] + 0.02 * torch.randn_like(images[:1]))
    sampler = SU.init_sampling(guider="TrianglePredictionGuider", steps=STEPS, cfg_scale=2.5, num_frames=T)
    sampler.graph = sampler.cfg_streams = True
    want = SU.do_sample(images, model, sampler, vd, num_rounds=3, num_frames=T, force_uc_zero_embeddings=sample.UC_KEYS, initial_cond_indices=[0],
                        get_condition=hook)
    assert len(calls) == 3 and "trajectory" in calls[0] and "goal" in calls[1] and not set(calls[2]) & {"trajectory", "command", "goal"}
    for name, a, b in zip(NAMES, (s.frames(), z, s.inputs), want):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))


def test_graph_replay_equals_eager_for_a_script(world, model, scripted):
    """A stale static conditioning buffer in a captured graph would carry round 0's action into rounds 1 and 2."""
    fast = scripted[0]
    slow, _ = _drive(model, world, [A, B, {}], True, 7)
    assert torch.equal(fast.samples_z, slow.samples_z) and torch.equal(fast.frames(), slow.frames()) and torch.equal(fast.inputs, slow.inputs)


def test_fork_branches_are_independent_and_equal_under_the_same_reseed(world, model):
    parent, _ = _drive(model, world, [A], False, 11)
    child = parent.fork()
    assert child.rounds == 1 and torch.equal(child.samples_z, parent.samples_z) and child.samples_z.data_ptr() != parent.samples_z.data_ptr()
    assert child.model is parent.model and child.sampler is parent.sampler
    torch.manual_seed(3)
    parent.step(A)
    torch.manual_seed(3)
    child.step(A)
    assert torch.equal(parent.samples_z, child.samples_z) and parent.rounds == child.rounds == 2
    kept = parent.samples_z.clone()
    grand = child.fork()
    torch.manual_seed(4)
    grand.step(B)
    assert torch.equal(parent.samples_z, kept) and torch.equal(child.samples_z, kept) and grand.rounds == 3
    assert torch.equal(grand.samples_z[:kept.shape[0]], kept) and [list(a) for a in grand.actions] == [["trajectory"]] * 2 + [["command", "goal"]]
    torch.manual_seed(4)
    child.step(A)
    assert not torch.equal(child.samples_z[kept.shape[0]:], grand.samples_z[kept.shape[0]:]), "same noise, another action"


def test_cli_writes_the_rollout_the_record_and_the_hud(world, model):
    """`python -m vista_amd.drive` once, as a fresh child process, with a three-round script and --hud."""
    from PIL import Image
    from vista_amd import drive
    from vista_amd import sample_utils as SU
    save = str(world["dir"] / "drive_out")
    entries = [{"command": 1}, {"trajectory": [[0.5, 0.0], [1.0, 0.0], [1.5, 0.1], [2.0, 0.2]], "goal": [400, 600]}, "scene"]
    script = str(world["dir"] / "script.json")
    with open(script, "w") as f:
        json.dump({"rounds": entries}, f)
    cmd = [sys.executable, "-m", "vista_amd.drive", "--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES",
           "--data_root", world["data_root"], "--anno_file", world["anno"], "--action", "traj", "--n_frames", str(T), "--height", str(H),
           "--width", str(W), "--n_steps", str(STEPS), "--cond_aug", "0.02", "--rand_gen", "--script", script, "--hud", "--save", save]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    n = 3 * (T - 3) + 3
    for sub, count in (("virtual", n), ("real", T)):
        assert sorted(os.listdir(os.path.join(save, sub))) == ["grids", "images", "videos"]
        assert sorted(os.listdir(os.path.join(save, sub, "images"))) == [f"NUSCENES_000000_{i:04}.png" for i in range(count)]
        assert os.listdir(os.path.join(save, sub, "grids")) == ["NUSCENES_000000.png"]
        assert os.listdir(os.path.join(save, sub, "videos")) in (["NUSCENES_000000.apng"], ["NUSCENES_000000.mp4"])
    lines = open(os.path.join(save, "drive.jsonl")).read().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert tuple(rec) == drive.RECORD_KEYS and (rec["index"], rec["seed"], rec["action"], rec["n_rounds"]) == (0, 23, "traj", 3)
    assert rec["frames"] == [world["frames"][0]]
    assert rec["rounds"] == [{"round": r, "action": e, "frames": list(drive.round_range(r, T))} for r, e in enumerate(entries)]
    assert sorted(rec["timings"]) == ["decode", "hud", "load", "sample", "save"] and all(v >= 0 for v in rec["timings"].values())

    # the saved predicted frames are the session's, stepped in this process under the CLI's seeding
    from vista_amd import ops, sample
    sample.seed_everything(23)
    frame_list, _, _, scene = SU.get_sample(0, "NUSCENES", T, "traj", data_root=world["data_root"], anno_file=world["anno"])
    s = drive.DriveSession(model, frame_list, height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02)
    actions = [drive.entry_action(e, scene) for e in entries]
    for a in actions:
        s.step(a)
    plain = ops.frames_to_u8(s.frames().float()).cpu().numpy()
    saved = np.stack([np.asarray(Image.open(os.path.join(save, "virtual", "images", f"NUSCENES_000000_{i:04}.png"))) for i in range(n)])
    assert np.array_equal(saved, plain), "the plain frames are written unmodified"
    videos = os.listdir(os.path.join(save, "hud", "videos"))
    assert videos in (["NUSCENES_000000.apng"], ["NUSCENES_000000.mp4"])
    if videos[0].endswith(".apng"):
        hud = SU.read_video_frames(os.path.join(save, "hud", "videos", videos[0]))
        sets = [drive.hud_strokes(a, H, W) for a in actions]
        assert all(sets) and list(actions[2]) == ["trajectory"]
        want = np.stack([R.draw(saved[i], sets[drive.frame_round(i, T)]) for i in range(n)])
        assert hud.shape == want.shape and np.array_equal(hud, want)
        assert not np.array_equal(hud, saved)
