"""Scene-per-rank runs of evaluate / denoise_loss / step_sweep (vista_amd/frontdoor.py: scene_ranks, SceneRanks, read_parts, RankedRun) without
a GPU: the hook VISTA_SCENE_RANKS and what it refuses, the partition of the walk over ranks, the merge of the part files with its errors, the
three summaries over merged records, and three real gloo processes around a stub body. Every comparison is exact."""
import argparse
import importlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKER = os.path.join(ROOT, "tests", "_scene_ranks_worker.py")

from tests._scene_ranks_worker import DATASET_LENGTH, RECORDS_NAME, SUMMARY_NAME, body, get_scene  # noqa: E402

DOORS = ("evaluate", "denoise_loss", "step_sweep")
WORLD_MESSAGES = {   # tests/test_frontdoor_walk_cpu.py pins the same words without the hook
    "evaluate": "WORLD_SIZE 2: vista_amd.evaluate runs on one GPU (scene-per-rank evaluation with a merge of "
                "the records is not built); start it without torch.distributed.run",
    "denoise_loss": "WORLD_SIZE 2: vista_amd.denoise_loss runs on one GPU (scene-per-rank scoring with a merge of "
                    "the records is not built); start it without torch.distributed.run",
    "step_sweep": "WORLD_SIZE 2: vista_amd.step_sweep runs on one GPU (scene-per-rank sweeping with a merge of "
                  "the records is not built); start it without torch.distributed.run",
}


class _Reached(Exception):
    """The model would have been built."""


def _clean_env(monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VISTA_SCENE_RANKS"):
        monkeypatch.delenv(name, raising=False)


# ---- 1. the hook ----------------------------------------------------------------------------------------------------------------------------------
def test_the_hook_is_read_in_one_place(monkeypatch):
    from vista_amd import pipeline
    from vista_amd import sample_utils as SU
    assert SU.scene_ranks is pipeline.scene_ranks
    _clean_env(monkeypatch)
    assert SU.scene_ranks() is False
    for text, want in (("", False), ("0", False), ("1", True)):
        monkeypatch.setenv("VISTA_SCENE_RANKS", text)
        assert SU.scene_ranks() is want
    for text in ("2", "yes", "true", "01"):
        monkeypatch.setenv("VISTA_SCENE_RANKS", text)
        with pytest.raises(ValueError) as e:
            SU.scene_ranks()
        assert str(e.value) == f"Bad value {text} (environment hook VISTA_SCENE_RANKS): 0 or 1"


@pytest.mark.parametrize("module,compare", [(d, False) for d in DOORS] + [("evaluate", True)],
                         ids=list(DOORS) + ["evaluate_compare"])
def test_the_hook_at_a_front_door(module, compare, monkeypatch, tmp_path):
    from vista_amd import frontdoor
    door = importlib.import_module(f"vista_amd.{module}")
    joined = []
    monkeypatch.setattr(frontdoor, "build_model", lambda *a, **k: (_ for _ in ()).throw(_Reached(f"after {len(joined)} joins")))
    monkeypatch.setattr(torch.distributed, "init_process_group", lambda backend, **k: joined.append((backend, k["rank"], k["world_size"])))
    monkeypatch.setattr(torch.distributed, "destroy_process_group", lambda: None)
    monkeypatch.setenv("VISTA_DIST_BACKEND", "nccl")   # (the group is gloo whatever this says: no tensor on a device enters it)
    out = tmp_path / "out"
    flags = ["--compare", str(out)] if compare else ["--rand_gen", "--save", str(out)]
    _clean_env(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    for text in (None, "0"):   # without the hook the refusal stands, word for word
        if text is not None:
            monkeypatch.setenv("VISTA_SCENE_RANKS", text)
        with pytest.raises(ValueError) as e:
            door.main(flags)
        assert str(e.value) == WORLD_MESSAGES[module]
    for text in ("2", "yes"):   # a bad value is refused by name, with and without a job around it
        monkeypatch.setenv("VISTA_SCENE_RANKS", text)
        for world in ("2", None):
            monkeypatch.setenv("WORLD_SIZE", world) if world else monkeypatch.delenv("WORLD_SIZE")
            with pytest.raises(ValueError) as e:
                door.main(flags)
            assert str(e.value) == f"Bad value {text} (environment hook VISTA_SCENE_RANKS): 0 or 1"
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("VISTA_SCENE_RANKS", "1")
    if compare:   # past the refusal: the next thing --compare wants is the pictures
        with pytest.raises(FileNotFoundError, match="does not exist"):
            door.main(flags)
    else:
        with pytest.raises(ValueError) as e:   # a rank would have nothing to do
            door.main(flags + ["--n_scenes", "1"])
        assert str(e.value).startswith("--n_scenes 1 with WORLD_SIZE 2 (environment hook VISTA_SCENE_RANKS=1)") and "nothing to do" in str(e.value)
        for more in ([], ["--n_scenes", "2"]):
            with pytest.raises(_Reached, match="after 1 joins"):   # the rank joins after the refusals and before the model
                door.main(flags + more)
            assert joined.pop() == ("gloo", 1, 2) and not joined
        monkeypatch.setenv("WORLD_SIZE", "1")   # the single-process run: nothing is joined
        with pytest.raises(_Reached, match="after 0 joins"):
            door.main(flags)
        monkeypatch.delenv("WORLD_SIZE")
        with pytest.raises(_Reached, match="after 0 joins"):
            door.main(flags + ["--n_scenes", "1"])
    assert not joined and not out.exists(), "a refused run writes nothing"


def test_ranks_are_plain_values(monkeypatch):
    from vista_amd import frontdoor
    one = frontdoor.SceneRanks()
    assert (one.rank, one.world, one.split, one.prefix, one.launched) == (0, 1, False, "", False) and all(one.owns(k) for k in range(5))
    r = frontdoor.SceneRanks(1, 2)
    assert r.split and r.prefix == "[rank 1] " and [k for k in range(6) if r.owns(k)] == [1, 3, 5]
    assert r.join() is r and not r.joined, "a rank made by hand joins no group"
    r.barrier()
    r.leave()
    assert not torch.distributed.is_initialized()
    for bad in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError):
            frontdoor.SceneRanks(*bad)
    _clean_env(monkeypatch)
    monkeypatch.setenv("VISTA_SCENE_RANKS", "1")
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "3")
    got = frontdoor.scene_ranks("evaluate", "x", 0)
    assert (got.rank, got.world, got.launched) == (3, 4, True)


# ---- 2. the partition -------------------------------------------------------------------------------------------------------------------------------
def _opt(random_walk):
    return argparse.Namespace(seed=23, dataset="NUSCENES", n_frames=4, action="traj", data_root="root", anno_file="anno.json", rand_gen=random_walk)


def _single_walk(random_walk, n_scenes, draw=lambda: None):
    from vista_amd import frontdoor
    seen = []
    for k, scene in enumerate(frontdoor.walk(_opt(random_walk), get_scene, n_scenes=n_scenes)):
        seen.append((k, scene[1]))
        draw()
    return seen


def _ranked_walk(tmp_path, rank, world, random_walk, n_scenes, draw=lambda: None):
    from vista_amd import frontdoor
    run = frontdoor.RankedRun(frontdoor.SceneRanks(rank, world), str(tmp_path / f"w{world}"), RECORDS_NAME, SUMMARY_NAME, len)
    seen = []
    for k, scene in run.scenes(_opt(random_walk), get_scene, n_scenes):
        seen.append((k, scene[1]))
        draw()
    return seen, run.count


@pytest.mark.parametrize("random_walk,n_scenes", [(False, 0), (True, 5)], ids=["sequential_to_the_end", "random_5"])
def test_the_ranks_partition_the_walk(random_walk, n_scenes, tmp_path):
    def draws():
        torch.rand(3), np.random.rand(2)
    single = _single_walk(random_walk, n_scenes)
    assert len(single) == (n_scenes or DATASET_LENGTH) and [k for k, _ in single] == list(range(len(single)))
    if random_walk:
        assert len({i for _, i in single}) > 1 and [i for _, i in single] != list(range(len(single))), "a walk with steps of its own"
    assert _single_walk(random_walk, n_scenes, draws) == single, "torch's and numpy's generators are free to the body"
    for world in (1, 2, 3, 4):
        parts = [_ranked_walk(tmp_path, rank, world, random_walk, n_scenes, draws) for rank in range(world)]
        for rank, (seen, count) in enumerate(parts):
            assert [k for k, _ in seen] == [k for k in range(len(single)) if k % world == rank], (world, rank)
            assert count == len(single), "every rank walks every scene"
        assert sorted(pair for seen, _ in parts for pair in seen) == single, world


def test_a_body_that_draws_from_random_changes_the_walk(tmp_path):
    """The rule the partition rests on: between the walk's seed_everything and its randint no body draws from Python's `random`. A body that
    does moves the single-process walk; a rank that skips that body walks elsewhere, and the ranks' union is no longer the single walk."""
    def draw():   # (two draws: after random.seed(23) a single one happens to leave the next randint(1, 6) where it was)
        random.random(), random.random()
    quiet = _single_walk(True, 5)
    noisy = _single_walk(True, 5, draw)
    assert noisy != quiet
    parts = [_ranked_walk(tmp_path, rank, 2, True, 5, draw)[0] for rank in (0, 1)]
    assert sorted(parts[0] + parts[1]) != noisy


def test_no_front_door_body_draws_from_random_on_the_way_from_the_cli():
    """The only random.* call of the package outside the walk and its seeding sits in StandardDiffusionLoss behind cond_frames_choices,
    and denoise_loss builds its loss with one empty choice, which draws nothing that could move the walk: pinned by source."""
    import re
    hits = []
    for top, _dirs, files in os.walk(os.path.join(ROOT, "vista_amd")):
        for name in files:
            if name.endswith(".py"):
                text = open(os.path.join(top, name)).read()
                for m in re.finditer(r"\brandom\.(?!seed\b)(\w+)\(", text):
                    if re.search(r"(np|numpy|torch)\.$", text[:m.start()]) is None:
                        hits.append((os.path.relpath(os.path.join(top, name), ROOT), m.group(1)))
    assert sorted(hits) == [("vista_amd/frontdoor.py", "randint"), ("vista_amd/modules/diffusionmodules/loss.py", "choices")], hits
    from vista_amd import frontdoor
    assert frontdoor.RankedRun.scenes.__doc__ and "random" in frontdoor.RankedRun.scenes.__doc__


# ---- 3. the merge -----------------------------------------------------------------------------------------------------------------------------------
def _part_lines(records, world):
    return {rank: [json.dumps({"k": k, "record": rec}) for k, rec in enumerate(records) if k % world == rank] for rank in range(world)}


def _hand_written(tmp_path, lines_of_rank, count=5, world=3):
    """Rank 0 of `world` at its finish, over part files written by hand."""
    from vista_amd import frontdoor
    save = str(tmp_path / "merge")
    run = frontdoor.RankedRun(frontdoor.SceneRanks(0, world), save, RECORDS_NAME, SUMMARY_NAME, lambda records: {"scenes": len(records)})
    for rank, lines in lines_of_rank.items():
        with open(os.path.join(save, f"{RECORDS_NAME}.rank{rank}"), "w") as f:
            f.write("".join(line + "\n" for line in lines))
    run.count = count
    return save, run


RECORDS = [{"index": 3 * k, "v": [0.1 * k, None, 1e-17, -0.0], "name": f"scène {k}", "timings": {"load": 0.5}} for k in range(5)]


def test_merge_of_hand_written_parts(tmp_path):
    save, run = _hand_written(tmp_path, _part_lines(RECORDS, 3))
    assert sorted(os.listdir(save)) == [f"{RECORDS_NAME}.rank{r}" for r in range(3)]
    run.finish()
    assert sorted(os.listdir(save)) == [RECORDS_NAME, SUMMARY_NAME], "the part files are gone after a good merge"
    assert open(os.path.join(save, RECORDS_NAME)).read() == "".join(json.dumps(rec) + "\n" for rec in RECORDS), "walk order, each line unchanged"
    text = open(os.path.join(save, SUMMARY_NAME)).read()
    assert text == json.dumps({"scenes": 5, "ranks": 3}, indent=1) + "\n"


@pytest.mark.parametrize("case", ["no_part_file", "no_position", "twice", "held_by_two", "not_its_own", "past_the_end"])
def test_an_incomplete_run_is_not_merged(case, tmp_path):
    lines = _part_lines(RECORDS, 3)
    if case == "no_part_file":
        del lines[2]
        error, words = FileNotFoundError, ("rank 2 ", "position 2 ")
    elif case == "no_position":
        del lines[1][1]
        error, words = ValueError, ("rank 1 ", "position 4 ")
    elif case == "twice":
        lines[1].append(lines[1][0])
        error, words = ValueError, ("rank 1 ", "position 1 ")
    elif case == "held_by_two":
        lines[2].append(lines[0][1])
        error, words = ValueError, ("rank 2 ", "position 3 ", "rank 0 ")
    elif case == "not_its_own":
        lines[1][0] = json.dumps({"k": 5, "record": RECORDS[1]})
        error, words = ValueError, ("rank 1 ", "position 5 ")
    else:
        lines[0].append(json.dumps({"k": 6, "record": RECORDS[0]}))
        error, words = ValueError, ("rank 0 ", "position 6 ")
    save, run = _hand_written(tmp_path, lines)
    before = {n: open(os.path.join(save, n)).read() for n in os.listdir(save)}
    with pytest.raises(error) as e:
        run.finish()
    assert all(w in str(e.value) for w in words), str(e.value)
    assert {n: open(os.path.join(save, n)).read() for n in os.listdir(save)} == before, "no records, no summary, and the part files stay"


def _door_records(module):
    """Five records with the keys the door's summary reads, scene by scene different."""
    if module == "evaluate":
        return [{"index": k, "frames_scored": 4 + k % 2, "cond": [0], "psnr": [None] + [20.0 + k + 0.1 * i for i in range(3 + k % 2)],
                 "ssim": [1.0] + [0.5 + 0.01 * k + 0.001 * i for i in range(3 + k % 2)], "mean_psnr": 20.1 + k, "mean_ssim": 0.5 + 0.01 * k,
                 "timings": {"load": 0.1 * k}} for k in range(5)]
    if module == "denoise_loss":
        return [{"index": k, "sigmas": [0.5, 4.0], "loss": [0.1 + k, 0.2 + k], "mse": [0.3 * k, 0.4], "dynamics": [0.5, 0.6 * k],
                 "structure": [0.7, 0.8 + k], "frame_mse": [[0.0, 0.1 * k, 0.2], [0.0, 0.3, 0.4 * k]], "cond": [0], "timings": {}} for k in range(5)]
    return [{"index": k, "cond": [0], "ref_sampler": "DPMPP2MSampler", "ref_steps": 4, "ref_gap": 1e-3 * (k + 1),
             "runs": [{"sampler": s, "steps": n, "latent_err": 0.1 / n + 0.01 * k + e, "frame_err": [0.0, 0.1 / n + 0.01 * k + e, 0.1 / n + 0.01 * k + e],
                       "mean_psnr": 30.0 + n - k, "mean_ssim": 0.9, "seconds": 0.1 * n}
                      for s, e in (("EulerEDMSampler", 0.02), ("DPMPP2MSampler", 0.0)) for n in (2, 3)]} for k in range(5)]


@pytest.mark.parametrize("module,name", [("evaluate", "summarize"), ("denoise_loss", "summarize"), ("step_sweep", "summarise")])
def test_a_summary_over_merged_records_is_the_summary_plus_ranks(module, name, tmp_path):
    from vista_amd import frontdoor
    door = importlib.import_module(f"vista_amd.{module}")
    summarize, records = getattr(door, name), _door_records(module)
    saves = {}
    for world in (1, 3):
        saves[world] = str(tmp_path / f"w{world}")
        runs = [frontdoor.RankedRun(frontdoor.SceneRanks(r, world), saves[world], door.RECORDS_NAME, door.SUMMARY_NAME, summarize) for r in range(world)]
        for run in runs:
            for k, rec in run.own(records):
                run.add(k, rec)
        for run in reversed(runs):   # (rank 0 last: no group, no barrier)
            run.finish()
        assert sorted(os.listdir(saves[world])) == [door.RECORDS_NAME, door.SUMMARY_NAME]
    one, three = (open(os.path.join(saves[w], door.RECORDS_NAME)).read() for w in (1, 3))
    assert one == three == "".join(json.dumps(rec) + "\n" for rec in records)
    one, three = (json.load(open(os.path.join(saves[w], door.SUMMARY_NAME))) for w in (1, 3))
    assert one == summarize(records) and "ranks" not in one
    assert list(three) == list(one) + ["ranks"] and three == {**one, "ranks": 3}
    assert open(os.path.join(saves[3], door.SUMMARY_NAME)).read() == json.dumps({**one, "ranks": 3}, indent=1) + "\n"


# ---- 4. three real gloo processes ---------------------------------------------------------------------------------------------------------------------
def _child(cmd, env_extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "VISTA_SCENE_RANKS")}
    env.update(env_extra)
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-6000:]
    return res


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_three_gloo_processes_write_what_one_process_writes(tmp_path):
    one, three = str(tmp_path / "one"), str(tmp_path / "three")
    args = ["5", "--random_walk"]
    single = _child([sys.executable, WORKER, one, *args], {"VISTA_SCENE_RANKS": "1"}, timeout=120)
    job = _child([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
                  "--master-port", str(_free_port()), WORKER, three, *args],
                 {"VISTA_SCENE_RANKS": "1", "VISTA_DIST_BACKEND": "nccl", "OMP_NUM_THREADS": "1"}, timeout=240)   # (gloo whatever the backend hook says)
    records = open(os.path.join(one, RECORDS_NAME)).read()
    assert records.count("\n") == 5 and open(os.path.join(three, RECORDS_NAME)).read() == records
    assert [json.loads(line) for line in records.splitlines()] == [_seeded_body(i) for _, i in _single_walk(True, 5)]
    summary = json.load(open(os.path.join(one, SUMMARY_NAME)))
    assert json.load(open(os.path.join(three, SUMMARY_NAME))) == {**summary, "ranks": 3}
    assert sorted(os.listdir(one)) == sorted([RECORDS_NAME, SUMMARY_NAME, "summarized_by_rank0"])
    assert sorted(os.listdir(three)) == sorted([RECORDS_NAME, SUMMARY_NAME, "summarized_by_rank0"]), "rank 0 alone summarised; no part file is left"
    lines = single.stdout.splitlines()
    assert len(lines) == 5 and all(line.startswith("thing ") for line in lines), "a single process prints no prefix"
    for rank in range(3):
        own = [line for line in job.stdout.splitlines() if line.startswith(f"[rank {rank}] thing ")]
        assert [line.split("] ", 1)[1] for line in own] == [line for k, line in enumerate(lines) if k % 3 == rank]


def _seeded_body(index):
    from vista_amd import frontdoor
    frontdoor.seed_everything(23)
    return body(get_scene(index, "NUSCENES", 4, "traj")[0], index)
