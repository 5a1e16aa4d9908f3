"""What the command-line front doors share (vista_amd/frontdoor.py): the walk over a dataset against a transcription of the loop every front
door used to carry, the records files, the WORLD_SIZE refusals word for word, and the first window's value dict with its one draw.
No GPU, no model. Every comparison is exact."""
import argparse
import json
import math
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DATASET_LENGTH = 5


def _opt(rand_gen):
    return argparse.Namespace(seed=23, dataset="NUSCENES", n_frames=4, action="traj", data_root="root", anno_file="anno.json", rand_gen=rand_gen)


class _Scenes:
    """A get_scene that records its arguments and draws nothing."""

    def __init__(self):
        self.calls = []

    def __call__(self, index, dataset, n_frames, action, data_root=None, anno_file=None):
        self.calls.append((index, dataset, n_frames, action, data_root, anno_file))
        return [f"scene{index}/f0.jpg"], index, DATASET_LENGTH, {"index": index}


def _body_draws():
    return random.random(), float(torch.rand(1))


def _transcribed_loop(opt, get_scene, n_scenes):
    """The loop as sample / evaluate / drive / denoise_loss / step_sweep each spelled it out: seed, get, body, the stop, randint or + 1, -1."""
    from vista_amd import sample
    seen = []
    sample_index = 0
    while sample_index >= 0:
        sample.seed_everything(opt.seed)
        frame_list, sample_index, dataset_length, action = get_scene(sample_index, opt.dataset, opt.n_frames, opt.action,
                                                                     data_root=opt.data_root, anno_file=opt.anno_file)
        seen.append((frame_list, sample_index, dataset_length, action) + _body_draws())

        if n_scenes and len(seen) >= n_scenes:
            break
        if opt.rand_gen:
            sample_index += random.randint(1, max(1, dataset_length - 1))
        else:
            sample_index += 1
            if dataset_length <= sample_index:
                sample_index = -1
    return seen


@pytest.mark.parametrize("rand_gen,n_scenes", [(False, 0), (False, 2), (True, 2), (True, 3)],
                         ids=["sequential_to_the_end", "sequential_counted", "random_counted_2", "random_counted_3"])
def test_the_walk_is_the_loop_every_front_door_carried(rand_gen, n_scenes):
    from vista_amd import frontdoor
    opt = _opt(rand_gen)
    want_scenes = _Scenes()
    want = _transcribed_loop(opt, want_scenes, n_scenes)
    scenes, got = _Scenes(), []
    for scene in frontdoor.walk(opt, scenes, n_scenes=n_scenes):
        got.append(tuple(scene) + _body_draws())
    assert got == want and scenes.calls == want_scenes.calls
    assert len(got) == (n_scenes or DATASET_LENGTH)
    assert all(call[1:] == ("NUSCENES", 4, "traj", "root", "anno.json") for call in scenes.calls)
    if not rand_gen:
        assert [g[1] for g in got] == list(range(len(got)))
    else:   # (every scene starts from the same seed and the body draws the same: the walk's step is one number)
        random.seed(opt.seed)
        random.random()
        step = random.randint(1, DATASET_LENGTH - 1)
        assert [g[1] for g in got] == [i * step for i in range(len(got))]


def test_the_walk_looks_get_sample_up_when_it_is_called(monkeypatch):
    from vista_amd import frontdoor
    from vista_amd import sample_utils as SU
    walk = frontdoor.walk(_opt(False))
    scenes = _Scenes()
    monkeypatch.setattr(SU, "get_sample", scenes)
    assert [s[1] for s in walk] == list(range(DATASET_LENGTH)) and len(scenes.calls) == DATASET_LENGTH


def test_a_body_that_raises_ends_the_walk():
    from vista_amd import frontdoor
    scenes, seen = _Scenes(), []
    with pytest.raises(RuntimeError, match="scene 1"):
        for _frames, index, _length, _action in frontdoor.walk(_opt(False), scenes):
            seen.append(index)
            if index == 1:
                raise RuntimeError("scene 1 failed")
    assert seen == [0, 1] and [c[0] for c in scenes.calls] == [0, 1], "no third scene is looked up"


# ---- records --------------------------------------------------------------------------------------------------------------------------------------
def test_records_start_empty_and_grow_by_one_line(tmp_path):
    from vista_amd import frontdoor
    save = str(tmp_path / "deep" / "out")
    path = frontdoor.start_records(save, "things.jsonl")
    assert path == os.path.join(save, "things.jsonl") and open(path).read() == "", "a missing directory is created"
    for n, record in enumerate(({"index": 0, "v": [1.5, None]}, {"index": 4, "v": []}), 1):
        assert frontdoor.append_record(save, "things.jsonl", record) == path
        assert open(path).read().count("\n") == n
    lines = open(path).read().splitlines()
    assert [json.loads(line) for line in lines] == [{"index": 0, "v": [1.5, None]}, {"index": 4, "v": []}]
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            frontdoor.append_record(save, "things.jsonl", {"index": 5, "v": [bad]})
        assert open(path).read().splitlines() == lines, "a refused record leaves the file as it was"
    assert frontdoor.start_records(save, "things.jsonl") == path and open(path).read() == "", "the file describes one run"
    other = str(tmp_path / "fresh")
    assert frontdoor.append_record(other, "things.jsonl", {"index": 0}) == os.path.join(other, "things.jsonl"), "append creates the directory too"


def test_summary_round_trips_and_ends_in_a_newline(tmp_path):
    from vista_amd import frontdoor
    summary = {"scenes": 2, "mean": 0.1, "curve": [None, 1.0, -0.0], "nested": {"a": [1, 2]}}
    path = frontdoor.write_summary(str(tmp_path / "out"), "summary.json", summary)
    text = open(path).read()
    assert path == str(tmp_path / "out" / "summary.json") and text.endswith("}\n") and json.loads(text) == summary
    assert text == json.dumps(summary, indent=1) + "\n"
    with pytest.raises(ValueError):
        frontdoor.write_summary(str(tmp_path / "out"), "summary.json", {"mean": float("nan")})


def test_json_number_and_mean():
    from vista_amd import frontdoor
    assert frontdoor.json_number(float("nan")) is None and frontdoor.json_number(math.inf) is None and frontdoor.json_number(-math.inf) is None
    assert frontdoor.json_number(0.0) == 0.0 and math.copysign(1.0, frontdoor.json_number(0.0)) == 1.0
    assert frontdoor.json_number(-0.0) == 0.0 and math.copysign(1.0, frontdoor.json_number(-0.0)) == -1.0
    assert frontdoor.json_number(torch.tensor(2.5, dtype=torch.float64)) == 2.5 and type(frontdoor.json_number(3)) is float
    assert math.isnan(frontdoor.mean([]))
    assert frontdoor.mean([1e16, 1.0, -1e16]) == 1 / 3, "fsum: the sum is exact, the mean has one rounding"
    assert frontdoor.mean([0.1] * 10) == math.fsum([0.1] * 10) / 10
    assert frontdoor.rounded_timings({"load": 0.12345678, "sample": 2}) == {"load": 0.1235, "sample": 2.0} and frontdoor.rounded_timings(None) == {}
    assert frontdoor.timings_text({"load": 0.126, "sample": 2}) == "load 0.13 s, sample 2.00 s"


# ---- start-up -------------------------------------------------------------------------------------------------------------------------------------
WORLD_MESSAGES = {
    "evaluate": "WORLD_SIZE 2: vista_amd.evaluate runs on one GPU (scene-per-rank evaluation with a merge of "
                "the records is not built); start it without torch.distributed.run",
    "drive": "WORLD_SIZE 2: vista_amd.drive runs on one GPU (a frame-sharded session is not built); start it "
             "without torch.distributed.run",
    "plan": "WORLD_SIZE 2: vista_amd.plan runs on one GPU (neither a frame-sharded session nor members "
            "over ranks are built); start it without torch.distributed.run",
    "denoise_loss": "WORLD_SIZE 2: vista_amd.denoise_loss runs on one GPU (scene-per-rank scoring with a merge of "
                    "the records is not built); start it without torch.distributed.run",
    "step_sweep": "WORLD_SIZE 2: vista_amd.step_sweep runs on one GPU (scene-per-rank sweeping with a merge of "
                  "the records is not built); start it without torch.distributed.run",
}


@pytest.mark.parametrize("module", list(WORLD_MESSAGES))
def test_every_one_gpu_front_door_refuses_a_job_in_its_own_words(module, monkeypatch, tmp_path):
    import importlib
    from vista_amd import sample_utils as SU
    door = importlib.import_module(f"vista_amd.{module}")
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused run"))
    candidates = tmp_path / "c.json"
    candidates.write_text(json.dumps({"candidates": [{}]}))
    flags = ["--rand_gen", "--save", str(tmp_path / "out")] + (["--candidates", str(candidates)] if module == "plan" else [])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError) as e:
        door.main(flags)
    assert str(e.value) == WORLD_MESSAGES[module]
    assert not (tmp_path / "out").exists(), "a refused run writes nothing"


def test_low_vram_is_announced_by_rank_zero_only(monkeypatch, capsys):
    from vista_amd import frontdoor, sample
    from vista_amd import sample_utils as SU
    specs = []
    monkeypatch.setattr(SU, "init_model", lambda spec: specs.append(spec) or "model")
    opt = sample.parse_args().parse_args(["--low_vram", "--config", "c.yaml", "--ckpt", "w.safetensors"])
    assert frontdoor.build_model(opt, rank=1) == "model" and capsys.readouterr().out == ""
    assert frontdoor.build_model(opt) == "model"
    assert capsys.readouterr().out == "--low_vram: accepted, no effect (every stage stays resident in HBM)\n"
    assert specs[0] == specs[1] == dict(SU.VERSION2SPECS["vwm"], config="c.yaml", ckpt="w.safetensors")
    assert frontdoor.build_model(sample.parse_args().parse_args([])) == "model" and specs[2] == SU.VERSION2SPECS["vwm"]
    assert capsys.readouterr().out == ""


# ---- the first window -----------------------------------------------------------------------------------------------------------------------------
SHIPPED_INPUT_KEYS = ("cond_frames_without_noise", "fps_id", "motion_bucket_id", "cond_frames", "cond_aug", "command", "trajectory", "speed",
                      "angle", "goal")   # configs/inference/vista_mi355x.yaml


class _Embedder:
    def __init__(self, input_key):
        self.input_key = input_key


class _Model:
    class conditioner:
        embedders = [_Embedder(k) for k in SHIPPED_INPUT_KEYS]


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key, value in a.items():
        if isinstance(value, torch.Tensor):
            assert torch.equal(value, b[key]), key
        else:
            assert value == b[key] and type(value) is type(b[key]), key


def test_first_window_values_are_the_five_lines_with_their_one_draw():
    from vista_amd import frontdoor
    from vista_amd import sample_utils as SU
    images = torch.linspace(-1.0, 1.0, 3 * 3 * 6 * 10).reshape(3, 3, 6, 10)
    cond_aug = 0.02

    torch.manual_seed(7)   # the five lines every run() carried
    unique_keys = set(e.input_key for e in _Model.conditioner.embedders)
    want = SU.init_embedder_options(unique_keys)
    cond_img = images[:1]
    want["cond_frames_without_noise"] = cond_img
    want["cond_aug"] = cond_aug
    want["cond_frames"] = cond_img + cond_aug * torch.randn_like(cond_img)
    assert want["fps_id"] == 9 and want["motion_bucket_id"] == 127 and not torch.equal(want["cond_frames"], cond_img)

    torch.manual_seed(7)
    got = frontdoor.first_window_values(_Model, images, cond_aug)
    state = torch.get_rng_state()
    _same(got, want)
    torch.manual_seed(7)
    torch.randn_like(images[:1])
    assert torch.equal(state, torch.get_rng_state()), "exactly one randn_like of the conditioning frame's shape"

    command = torch.tensor(2)
    torch.manual_seed(7)
    with_action = frontdoor.first_window_values(_Model, images, cond_aug, action_dict={"command": command})
    assert with_action["command"] is command
    _same({k: v for k, v in with_action.items() if k != "command"}, want)
    torch.manual_seed(7)
    _same(frontdoor.first_window_values(_Model, images, cond_aug, action_dict={}), want)
