"""Scene-per-rank runs on the MI355X, on the tiny pipeline of tests/test_frontdoor_gpu.py (5 frames, 128 x 256, 3 steps) over three annotated
scenes: `evaluate` (with the CLIP-space and motion scores), `denoise_loss`, `step_sweep` and `evaluate --compare` as two ranks run one after
the other in this process with no group, and `evaluate` once as two real processes under torch.distributed.run that share GPU 0. Every
comparison with the single-process run is exact: the same lines once the wall times are taken out, the same summary plus "ranks", the same
bytes in every picture."""
import json
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_ENDED_BADLY = (124, 134, 137, 139, -6, -9, -11)   # a time limit, an abort, a kill, a segmentation fault: nothing more is started on the GPU


@pytest.fixture(scope="module")
def scenes(world):
    """The seven pictures and the two scenes of tests/test_fidelity_gpu.py's annotation, and a third scene: frames 1 .. 5."""
    from PIL import Image
    root = world["dir"] / "ranks_data"
    (root / "cam").mkdir(parents=True)
    names = []
    for i, src in enumerate(world["frames"]):
        names.append(f"cam/frame{i}.png")
        shutil.copy(src, root / names[-1])
    rng = np.random.default_rng(9)
    for i in (5, 6):
        yy, xx = np.mgrid[0:180, 0:320]
        img = np.stack([127 + 120 * np.sin(xx / (9.0 + i) + c) * np.cos(yy / (7.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (180, 320, 3))
        names.append(f"cam/frame{i}.png")
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(root / names[-1])
    traj = [0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2]
    anno = str(world["dir"] / "ranks_anno.json")
    with open(anno, "w") as f:
        json.dump([{"frames": names, "traj": traj, "cmd": 1, "speed": [], "angle": [], "z": 1.0, "goal": [800.0, 450.0]},
                   {"frames": names[2:], "traj": traj, "cmd": 2, "speed": [], "angle": [], "z": 1.0, "goal": [800.0, 450.0]},
                   {"frames": names[1:6], "traj": traj, "cmd": 3, "speed": [], "angle": [], "z": 1.0, "goal": [800.0, 450.0]}], f)
    return {"data_root": str(root), "anno": anno, "names": names}


def _flags(world, scenes, save):
    return ["--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES", "--data_root", scenes["data_root"], "--anno_file",
            scenes["anno"], "--action", "traj", "--n_frames", str(T), "--height", str(H), "--width", str(W), "--n_steps", str(STEPS),
            "--cond_aug", "0.02", "--rand_gen", "--save", save]


def _lines(save, name):
    return [json.loads(line) for line in open(os.path.join(save, name)).read().splitlines()]


def _without(value, keys):
    """The same JSON value without the wall times: every dict entry named in `keys`, at any depth."""
    if isinstance(value, dict):
        return {k: _without(v, keys) for k, v in value.items() if k not in keys}
    return [_without(v, keys) for v in value] if isinstance(value, list) else value


def _tree(top):
    """relative path -> bytes of every file under top/virtual and top/real."""
    out = {}
    for side in ("virtual", "real"):
        for d, _dirs, files in os.walk(os.path.join(top, side)):
            for f in files:
                out[os.path.relpath(os.path.join(d, f), top)] = open(os.path.join(d, f), "rb").read()
    return out


def _same_run(one, two, records_name, summary_name, times, world_size=2):
    """Two save directories: line by line the same records once the wall times are out, the same summary plus a last key "ranks"."""
    a, b = _lines(one, records_name), _lines(two, records_name)
    assert len(a) == len(b) == 3 and [r["index"] for r in b] == [0, 1, 2], "walk order"
    for x, y in zip(a, b):
        assert list(x) == list(y) and json.dumps(_without(x, times)) == json.dumps(_without(y, times)), x["index"]
    s1, s2 = (json.load(open(os.path.join(top, summary_name))) for top in (one, two))
    assert "ranks" not in s1 and list(s2) == list(s1) + ["ranks"] and s2["ranks"] == world_size
    assert json.dumps(_without(s2, times + ("ranks",))) == json.dumps(_without(s1, times))
    assert not [f for f in os.listdir(two) if ".rank" in f], "no part file remains"
    return a, s1, s2


class _RandomStateWatch:
    """frontdoor.walk with Python's `random` state compared across every scene body: the partition over ranks rests on it."""

    def __init__(self, monkeypatch):
        from vista_amd import frontdoor
        self.bodies, self.walk = [], frontdoor.walk
        monkeypatch.setattr(frontdoor, "walk", self)

    def __call__(self, opt, get_scene=None, n_scenes=0):
        for scene in self.walk(opt, get_scene, n_scenes):
            before = random.getstate()
            yield scene
            self.bodies.append(random.getstate() == before)


def _in_process_ranks(scenes_of_rank, save, records_name):
    """Rank 0 of 2, then rank 1 of 2, one after the other with no group; then the merge: rank 0 finishes last."""
    from vista_amd import frontdoor
    runs = [scenes_of_rank(frontdoor.SceneRanks(rank, 2)) for rank in (0, 1)]
    assert [f for f in sorted(os.listdir(save)) if f.startswith(records_name)] == [f"{records_name}.rank0", f"{records_name}.rank1"]
    parts = [_lines(save, f"{records_name}.rank{rank}") for rank in (0, 1)]
    assert [[e["k"] for e in part] for part in parts] == [[0, 2], [1]] and all(list(e) == ["k", "record"] for part in parts for e in part)
    assert [len(run.records) for run in runs] == [2, 1] and [run.count for run in runs] == [3, 3]
    runs[1].finish()
    assert not os.path.exists(os.path.join(save, records_name)), "rank 1 merges nothing"
    runs[0].finish()
    return runs


@pytest.fixture(scope="module")
def evaluated(world, scenes, model):
    """`evaluate` with both score hooks over the three scenes: once as a single process, once as two in-process ranks."""
    from vista_amd import evaluate
    from vista_amd import sample_utils as SU
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(SU, "init_model", lambda spec: model)        # (the fixture's pipeline: same config, same checkpoint)
        mp.setenv("VISTA_EVAL_CLIP", "1")
        mp.setenv("VISTA_EVAL_MOTION", "1")
        for name in ("WORLD_SIZE", "RANK", "VISTA_SCENE_RANKS"):
            mp.delenv(name, raising=False)
        watch = _RandomStateWatch(mp)
        one, two = str(world["dir"] / "ranks_eval_one"), str(world["dir"] / "ranks_eval_two")
        assert evaluate.main(_flags(world, scenes, one)) == 0
        opt = evaluate.parse_args().parse_known_args(_flags(world, scenes, two))[0]
        clip_parts = []

        def scenes_of_rank(ranks):
            run = evaluate._evaluate_scenes(opt, ranks)
            clip_parts.append(os.path.join(two, f"metrics.jsonl.clip.rank{ranks.rank}"))
            return run
        _in_process_ranks(scenes_of_rank, two, "metrics.jsonl")
        return {"one": one, "two": two, "bodies": watch.bodies, "clip_parts": clip_parts}
    finally:
        mp.undo()


# ---- 5. in-process ranks: evaluate ------------------------------------------------------------------------------------------------------------------
def test_evaluate_as_two_ranks_writes_what_one_process_writes(evaluated, capsys):
    one, two = evaluated["one"], evaluated["two"]
    records, s1, s2 = _same_run(one, two, "metrics.jsonl", "metrics_summary.json", ("timings",))
    assert all("clip_sim" in r and "flow_epe" in r and r["frames_scored"] == T for r in records)
    for key in ("biased", "unbiased"):   # the run-level MMD over the embeddings of both ranks: the same rows in the same order, the same bits
        assert isinstance(s1["clip_mmd"][key], float) and s2["clip_mmd"][key] == s1["clip_mmd"][key]
    assert s1["clip_mmd"]["m"] == s2["clip_mmd"]["m"] == 3 * (T - 1)
    assert not any(os.path.exists(p) for p in evaluated["clip_parts"]) and len(evaluated["clip_parts"]) == 2
    a, b = _tree(one), _tree(two)
    assert sorted(a) == sorted(b) and len(a) == 3 * 2 * (T + 2), "every rank wrote its own scenes' pictures"
    assert all(a[name] == b[name] for name in a), [name for name in a if a[name] != b[name]]
    assert sorted(os.listdir(two)) == sorted(os.listdir(one)) == ["metrics.jsonl", "metrics_summary.json", "real", "virtual"]
    assert evaluated["bodies"] == [True] * 9, "no scene body touches Python's random generator: three walks of three scenes"


def test_printed_lines_carry_the_rank(world, scenes, model, monkeypatch, capsys):
    from vista_amd import evaluate, frontdoor
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)
    opt = evaluate.parse_args().parse_known_args(_flags(world, scenes, str(world["dir"] / "ranks_eval_lines")) + ["--no_pictures"])[0]
    evaluate._evaluate_scenes(opt, frontdoor.SceneRanks(1, 3))
    out = [line for line in capsys.readouterr().out.splitlines() if "evaluate" in line]
    assert len(out) == 1 and out[0].startswith("[rank 1] evaluate 1: 5 frames, mean_psnr ")
    evaluate._evaluate_scenes(opt, frontdoor.SceneRanks()).finish()
    out = [line for line in capsys.readouterr().out.splitlines() if "evaluate" in line]
    assert [line[:12] for line in out] == ["evaluate 0: ", "evaluate 1: ", "evaluate 2: "], "a single process prints today's lines"


# ---- 6. in-process ranks: the other doors -------------------------------------------------------------------------------------------------------------
def test_denoise_loss_as_two_ranks_writes_what_one_process_writes(world, scenes, model, monkeypatch):
    from vista_amd import denoise_loss
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)
    watch = _RandomStateWatch(monkeypatch)
    one, two = str(world["dir"] / "ranks_loss_one"), str(world["dir"] / "ranks_loss_two")
    assert denoise_loss.main(_flags(world, scenes, one) + ["--n_sigmas", "2"]) == 0
    opt = denoise_loss.parse_args().parse_known_args(_flags(world, scenes, two) + ["--n_sigmas", "2"])[0]
    _in_process_ranks(lambda ranks: denoise_loss._loss_scenes(opt, ranks), two, "loss.jsonl")
    records, s1, _ = _same_run(one, two, "loss.jsonl", "loss_summary.json", ("timings",))
    assert s1["scenes"] == 3 and len({json.dumps(r["loss"]) for r in records}) == 3 and all(len(r["loss"]) == 2 for r in records)
    assert watch.bodies == [True] * 9


def test_step_sweep_as_two_ranks_writes_what_one_process_writes(world, scenes, model, monkeypatch):
    from vista_amd import frontdoor, step_sweep
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)
    watch = _RandomStateWatch(monkeypatch)
    one, two = str(world["dir"] / "ranks_sweep_one"), str(world["dir"] / "ranks_sweep_two")
    more = ["--budgets", "2,3", "--ref_steps", "4"]
    assert step_sweep.main(_flags(world, scenes, one) + more) == 0
    opt = step_sweep.parse_args().parse_known_args(_flags(world, scenes, two) + more)[0]
    samplers, budgets = step_sweep.check_run(opt, frontdoor.net_params(opt))
    _in_process_ranks(lambda ranks: step_sweep._sweep_scenes(opt, samplers, budgets, ranks), two, "steps.jsonl")
    records, s1, _ = _same_run(one, two, "steps.jsonl", "steps_summary.json", ("seconds", "ref_seconds"))
    assert s1["scenes"] == 3 and all([(r["sampler"], r["steps"]) for r in rec["runs"]] == [(s, n) for s in samplers for n in (2, 3)] for rec in records)
    assert len({json.dumps(_without(r["runs"], ("seconds",))) for r in records}) == 3
    assert watch.bodies == [True] * 9


# ---- 7. in-process ranks: compare ---------------------------------------------------------------------------------------------------------------------
def test_compare_as_two_ranks_gives_the_records_of_the_online_run(evaluated, world, monkeypatch):
    from tests.test_fidelity_gpu import _per_frame
    from tests.test_perceptual_gpu import _clip_part
    from vista_amd import evaluate
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", None)   # (no pipeline is built: every rank loads the tower alone)
    monkeypatch.setenv("VISTA_EVAL_CLIP", "1")
    monkeypatch.setenv("VISTA_EVAL_MOTION", "1")
    online, online_summary = _lines(evaluated["one"], "metrics.jsonl"), json.load(open(os.path.join(evaluated["one"], "metrics_summary.json")))
    top, kept = str(world["dir"] / "ranks_compare"), str(world["dir"] / "ranks_compare_single")
    shutil.copytree(evaluated["one"], top)   # (the pictures of the online run; a record names its first real picture, so both runs score this copy)
    flags = ["--compare", top, "--n_conds", "1", "--n_frames", str(T), "--action", "traj", "--config", world["config"], "--ckpt", world["ckpt"]]
    assert evaluate.main(flags) == 0
    os.makedirs(kept)
    for name in ("metrics.jsonl", "metrics_summary.json"):
        shutil.move(os.path.join(top, name), os.path.join(kept, name))
    opt = evaluate.parse_args().parse_known_args(flags)[0]
    _in_process_ranks(lambda ranks: evaluate._compare(opt, ranks), top, "metrics.jsonl")
    offline, s1, _ = _same_run(kept, top, "metrics.jsonl", "metrics_summary.json", ("timings",))
    assert all(sorted(r["timings"]) == ["clip", "load", "metrics", "motion"] for r in _lines(top, "metrics.jsonl"))

    def motion_part(records):
        return [[r[k] for k in r if "flow_" in k or "warp_" in k] + [[x["mean_flow_epe"] for x in r["rounds"]]] for r in records]
    assert _per_frame(offline) == _per_frame(online) and _clip_part(offline) == _clip_part(online) and motion_part(offline) == motion_part(online)
    assert s1 == online_summary, "the saved bytes are the ones the online run scored"


# ---- 8. one real launch -----------------------------------------------------------------------------------------------------------------------------
# Each child's time limit: tests/test_frontdoor_mgpu_gpu.py::test_two_gloo_processes_on_one_gpu_write_what_one_process_writes -- the same pair of
# children around vista_amd.sample, each building the tiny pipeline -- took 12.72 s on the same MI355X box; that time plus half, rounded up.
CHILD_SECONDS = 20


def _child(cmd, env_extra, timeout):
    """One child process with a time limit of its own. The test ends at the first child that does not end well."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "VISTA_SCENE_RANKS")}
    env.update(env_extra)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)   # (TimeoutExpired ends the test here)
    if res.returncode in CHILD_ENDED_BADLY:
        pytest.fail(f"a child ended with {res.returncode}; nothing more is started on the GPU\n" + res.stdout[-3000:] + res.stderr[-6000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return res


def _free_port():
    """A rendezvous port nobody holds right now (asked of the kernel, so two checkouts running the suite side by side do not collide)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_two_processes_on_one_gpu_write_what_one_process_writes(world, scenes):
    """`python -m torch.distributed.run --nproc-per-node 2 -m vista_amd.evaluate` with VISTA_SCENE_RANKS=1 and both ranks on GPU 0, against
    the single-process CLI in a child of its own. Measured on one MI355X box, one run: the test 17.2 s -- the single-process child 7.7 s, the
    two-rank job 9.5 s, each under its limit of CHILD_SECONDS; two ranks on one GPU are not faster than one, and nothing here says they are.
    The test ends at the first child that does not end well."""
    import time
    one, two = str(world["dir"] / "ranks_cli_one"), str(world["dir"] / "ranks_cli_two")
    hooks = {"VISTA_EVAL_CLIP": "1", "VISTA_EVAL_MOTION": "1"}
    t0 = time.perf_counter()
    single = _child([sys.executable, "-m", "vista_amd.evaluate", *_flags(world, scenes, one)], hooks, timeout=CHILD_SECONDS)
    t1 = time.perf_counter()
    job = _child([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
                  str(_free_port()), "-m", "vista_amd.evaluate", *_flags(world, scenes, two)],
                 {**hooks, "VISTA_SCENE_RANKS": "1", "VISTA_FORCE_DEVICE": "0", "VISTA_DIST_BACKEND": "nccl"}, timeout=CHILD_SECONDS)
    print(f"[time] the single-process child {t1 - t0:.1f} s, the two-rank job {time.perf_counter() - t1:.1f} s")
    _, s1, s2 = _same_run(one, two, "metrics.jsonl", "metrics_summary.json", ("timings",))
    for key in ("biased", "unbiased"):
        assert isinstance(s1["clip_mmd"][key], float) and s2["clip_mmd"][key] == s1["clip_mmd"][key]
    a, b = _tree(one), _tree(two)
    assert sorted(a) == sorted(b) and len(a) == 3 * 2 * (T + 2) and all(a[name] == b[name] for name in a)
    assert sorted(os.listdir(two)) == sorted(os.listdir(one)) == ["metrics.jsonl", "metrics_summary.json", "real", "virtual"]
    assert re.findall(r"^(.*)evaluate (\d+): 5 frames", single.stdout, flags=re.M) == [("", "0"), ("", "1"), ("", "2")]
    assert sorted(re.findall(r"^(.*)evaluate (\d+): 5 frames", job.stdout, flags=re.M)) == [("[rank 0] ", "0"), ("[rank 0] ", "2"), ("[rank 1] ", "1")]
