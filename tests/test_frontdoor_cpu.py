"""Host side of the sampling front door (vista_amd/pipeline.py, vista_amd/sample.py, vista_amd/image_io.py): sampler factories, CLI flags,
dataset lookup, crop boxes and Lanczos tables, file names, the size rule. No GPU. Every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("wide", "tall", "exact", "cols")

# the reference's literal guider dicts (sample_utils.py:167-207) for cfg_scale s and num_frames t
GUIDERS = {
    "IdentityGuider": lambda s, t: None,
    "VanillaCFG": lambda s, t: {"scale": s},
    "LinearPredictionGuider": lambda s, t: {"max_scale": s, "min_scale": 1.0, "num_frames": t},
    "TrianglePredictionGuider": lambda s, t: {"max_scale": s, "min_scale": 1.0, "num_frames": t},
}


@pytest.mark.parametrize("steps", [5, 50])
@pytest.mark.parametrize("guider", sorted(GUIDERS))
def test_init_sampling_known_answers(guider, steps):
    from vista_amd import config
    from vista_amd import sample_utils as SU
    from vista_amd.modules.diffusionmodules import discretizer, guiders, sampling
    from vista_amd.util import instantiate_from_config
    s = SU.init_sampling(guider=guider, steps=steps, cfg_scale=3.0, num_frames=7)
    assert type(s) is sampling.EulerEDMSampler and type(s.discretization) is discretizer.EDMDiscretization
    assert type(s.guider) is getattr(guiders, guider)
    assert (s.s_churn, s.s_tmin, s.s_tmax, s.s_noise, s.verbose, s.num_steps) == (0.0, 0.0, 999.0, 1.0, False, steps)
    assert s.graph is None and s.cfg_streams is None, "the environment decides unless a caller says otherwise"
    shipped = config.load_config()["sampler"]
    shipped["params"]["num_steps"] = steps
    assert torch.equal(s.host_sigmas(), instantiate_from_config(shipped).host_sigmas())
    assert (s.discretization.sigma_min, s.discretization.sigma_max, s.discretization.rho) == (0.002, 700.0, 7.0)
    assert abs(float(s.host_sigmas()[0]) - 700.0) < 1e-3 and float(s.host_sigmas()[-1]) == 0.0 and len(s.host_sigmas()) == steps + 1
    want = GUIDERS[guider](3.0, 7)
    cfg = SU.get_guider(guider, 3.0, 7)
    assert cfg["target"] == "vwm.modules.diffusionmodules.guiders." + guider and cfg.get("params") == want
    assert SU.get_discretization("EDMDiscretization") == {"target": "vwm.modules.diffusionmodules.discretizer.EDMDiscretization",
                                                          "params": {"sigma_min": 0.002, "sigma_max": 700.0, "rho": 7.0}}


def test_init_sampling_defaults_and_refusals():
    import inspect
    from vista_amd import sample_utils as SU
    sig = inspect.signature(SU.init_sampling)
    assert {k: v.default for k, v in sig.parameters.items()} == {"sampler": "EulerEDMSampler", "guider": "VanillaCFG", "discretization": "EDMDiscretization",
                                                                 "steps": 50, "cfg_scale": 2.5, "num_frames": 25}
    assert {k: v.default for k, v in inspect.signature(SU.get_guider).parameters.items()} == {"guider": "LinearPredictionGuider", "cfg_scale": 2.5,
                                                                                              "num_frames": 25}
    with pytest.raises(NotImplementedError, match="LegacyDDPMDiscretization"):
        SU.init_sampling(discretization="LegacyDDPMDiscretization")
    with pytest.raises(NotImplementedError):
        SU.get_guider("NoSuchGuider")
    with pytest.raises(ValueError, match="HeunEDMSampler"):
        SU.init_sampling(sampler="HeunEDMSampler")
    assert SU.init_embedder_options(["fps_id", "motion_bucket_id", "cond_aug", "cond_frames"]) == {"fps": 10, "fps_id": 9, "motion_bucket_id": 127}
    assert SU.init_embedder_options(["cond_frames"]) == {}


def test_cli_flags_equal_the_reference_fixture():
    from vista_amd import sample
    parser = sample.parse_args()
    golden = json.load(open(os.path.join(GOLD, "sample_cli_flags.json")))["flags"]
    actions = {a.dest: a for a in parser._actions if a.dest != "help"}
    kinds = {"str": str, "int": int, "float": float}
    for flag in golden:
        a = actions.pop(flag["name"])
        assert a.option_strings == ["--" + flag["name"]] and a.default == flag["default"] and type(a.default) is type(flag["default"]), flag
        if flag["kind"] in kinds:
            assert a.type is kinds[flag["kind"]] and a.nargs is None, flag
        else:
            assert a.nargs == 0 and a.const is (flag["kind"] == "store_true"), flag
    assert sorted(actions) == ["anno_file", "ckpt", "config", "data_root", "eager"], "what this package adds to the reference's flags"
    assert all(actions[k].default is None for k in ("anno_file", "ckpt", "config", "data_root")) and actions["eager"].default is False
    opt = parser.parse_args(["--rand_gen", "--low_vram", "--eager", "--n_rounds", "3"])
    assert opt.rand_gen is False and opt.low_vram is True and opt.eager is True and opt.n_rounds == 3


def _dataset(tmp_path):
    root = tmp_path / "nuscenes"
    root.mkdir()
    names = [f"cam/f{i}.jpg" for i in range(4)]
    (root / "cam").mkdir()
    for n in names:
        (root / n).write_bytes(b"x")
    scenes = [
        {"frames": names, "traj": [0.0, 0.0, 1.0, 0.5, 2.0, 1.0, 3.0, 1.5, 4.0, 2.0], "cmd": 2, "speed": [1.0, 2.0, 3.0, 4.0, 5.0],
         "angle": [0.0, 78.0, -390.0, 780.0, 39.0], "z": 1.5, "goal": [800.0, 450.0]},
        {"frames": names[::-1], "traj": [0.0] * 10, "cmd": 0, "speed": [], "angle": [], "z": -1.0, "goal": [800.0, 450.0]},
        {"frames": names, "traj": [0.0] * 10, "cmd": 1, "speed": [0.0] * 5, "angle": [0.0] * 5, "z": 2.0, "goal": [1600.0, 450.0]},
    ]
    anno = tmp_path / "anno.json"
    anno.write_text(json.dumps(scenes))
    return str(root), str(anno), names


def test_get_sample_nuscenes_actions_wraparound_and_validity(tmp_path):
    from vista_amd import sample_utils as SU
    root, anno, names = _dataset(tmp_path)
    kw = dict(data_root=root, anno_file=anno)
    paths, idx, total, action = SU.get_sample(0, "NUSCENES", 3, "free", **kw)
    assert paths == [os.path.join(root, n) for n in names[:3]] and (idx, total, action) == (0, 3, None)
    assert SU.get_sample(7, "NUSCENES", 2, "free", **kw)[:3] == ([os.path.join(root, n) for n in names[::-1][:2]], 1, 3)   # 7 -> 4 -> 1
    assert SU.get_sample(3, "NUSCENES", 2, "free", **kw)[1] == 0

    def act(i, mode):
        return SU.get_sample(i, "NUSCENES", 2, mode, **kw)[3]
    for mode in ("traj", "trajectory"):
        assert list(act(0, mode)) == ["trajectory"] and torch.equal(act(0, mode)["trajectory"], torch.tensor([1.0, 0.5, 2.0, 1.0, 3.0, 1.5, 4.0, 2.0]))
    for mode in ("cmd", "command"):
        assert torch.equal(act(0, mode)["command"], torch.tensor(2))
    steer = act(0, "steer")
    assert torch.equal(steer["speed"], torch.tensor([2.0, 3.0, 4.0, 5.0])) and torch.equal(steer["angle"], torch.tensor([78.0, -390.0, 780.0, 39.0]) / 780)
    assert act(1, "steer") == {}, "a scene without CAN bus data gives an empty action dict, not an error"
    assert torch.equal(act(0, "goal")["goal"], torch.tensor([800.0 / 1600, 450.0 / 900]))
    assert act(1, "goal") == {} and act(2, "goal") == {}, "z <= 0, or a goal on / outside the frame border, is no goal"
    with pytest.raises(ValueError, match="Unsupported action mode"):
        act(0, "fly")
    with pytest.raises(ValueError, match="Invalid dataset"):
        SU.get_sample(0, "KITTI", 2, "free", **kw)
    os.remove(os.path.join(root, names[1]))
    with pytest.raises(FileNotFoundError):
        SU.get_sample(0, "NUSCENES", 3, "free", **kw)
    assert SU.DATASET2SOURCES == {"NUSCENES": {"data_root": "data/nuscenes", "anno_file": "annos/nuScenes_val.json"}, "IMG": {"data_root": "image_folder"}}


def test_get_sample_image_folder(tmp_path):
    from vista_amd import sample_utils as SU
    for n in ("a.png", "b.png", "c.png"):
        (tmp_path / n).write_bytes(b"x")
    listing = os.listdir(tmp_path)
    paths, idx, total, action = SU.get_sample(4, "IMG", 5, "traj", data_root=str(tmp_path))
    assert (idx, total, action) == (1, 3, None) and paths == [os.path.join(str(tmp_path), listing[1])] * 5


def test_crop_boxes_follow_load_img():
    from vista_amd.image_io import crop_box
    assert crop_box(1600, 900, 576, 1024) == (0, 0, 1600, 900)            # nuScenes: exact 16:9
    assert crop_box(400, 120, 128, 256) == (80, 0, 240, 120)              # too wide: columns go
    assert crop_box(401, 121, 128, 256) == (79, 0, 242, 121)              # int(2.0 * 121) = 242; left (401 - 242) // 2, right (401 + 242) // 2
    assert crop_box(100, 100, 128, 256) == (0, 25, 100, 50)               # too tall: rows go
    assert crop_box(400, 225, 128, 256) == (0, 12, 400, 200)              # 12 = (225 - 200) // 2, bottom (225 + 200) // 2 = 212
    assert crop_box(1920, 1080, 576, 1024) == (0, 0, 1920, 1080)
    assert crop_box(1001, 300, 128, 256) == (200, 0, 600, 300)
    assert crop_box(300, 1001, 256, 128) == (0, 200, 300, 600)


def test_lanczos_tables_reproduce_the_golden_and_pillow():
    from vista_amd import image_io as I
    g = np.load(os.path.join(GOLD, "image_io.npz"))
    th, tw = (int(v) for v in g["target"])
    for name in CASES:
        src, box = g[name + "_src"], tuple(int(v) for v in g[name + "_box"])
        assert box == I.crop_box(src.shape[1], src.shape[0], th, tw)
        got = I.resize_u8_reference(src, box, th, tw)
        assert got.dtype == np.uint8 and np.array_equal(got, g[name + "_u8"]), name
        f32 = I.unit_range_table()[got].transpose(2, 0, 1)
        assert f32.dtype == np.float32 and np.array_equal(f32, g[name + "_f32"]), name
    assert torch.equal(torch.from_numpy(I.unit_range_table()), torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255) * 2.0 - 1.0)
    bounds, coef, ksize = I.lanczos_tables(1600, 1024)
    assert ksize == 11 and bounds.shape == (1024, 2) and coef.shape == (1024, 11) and bounds.dtype == coef.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 1600).all() and (bounds[:, 1] <= ksize).all()
    assert (np.abs(coef.sum(1) - (1 << 22)) <= ksize).all(), "weights are normalised before they are rounded"
    PIL = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for h, w, oh, ow in ((900, 1600, 576, 1024), (97, 131, 64, 128), (200, 300, 576, 1024), (450, 800, 128, 256)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        left, top, cw, ch = I.crop_box(w, h, oh, ow)
        want = np.asarray(PIL.fromarray(img).crop((left, top, left + cw, top + ch)).resize((ow, oh), resample=PIL.LANCZOS))
        assert np.array_equal(I.resize_u8_reference(img, (left, top, cw, ch), oh, ow), want), (h, w, oh, ow)


def test_grid_geometry_is_make_grid():
    from vista_amd.image_io import grid_geometry
    assert grid_geometry(25, 576, 1024) == (5, 5, 5 * 578 + 2, 5 * 1026 + 2, 2)
    assert grid_geometry(47, 8, 12) == (6, 8, 8 * 10 + 2, 6 * 14 + 2, 2)
    assert grid_geometry(5, 8, 12) == (2, 3, 32, 30, 2)
    assert grid_geometry(1, 8, 12) == (1, 1, 8, 12, 0)     # make_grid hands a single image back as it is


def test_perform_save_locally_names_and_the_real_rule(tmp_path, monkeypatch):
    from PIL import Image
    from vista_amd import pipeline
    from vista_amd import sample_utils as SU
    seen = []

    def numpy_u8(samples, real, grid=False):   # the reference's numpy expressions (sample_utils.py:104-131) in place of the kernel
        seen.append((real, grid))
        x = samples.numpy().transpose(0, 2, 3, 1)
        x = 255.0 * (x + 1.0) / 2.0 if real else 255.0 * x
        return x.astype(np.uint8)[0] if grid else x.astype(np.uint8)
    monkeypatch.setattr(pipeline, "_to_u8", numpy_u8)
    g = torch.Generator().manual_seed(0)
    samples = torch.rand(3, 3, 4, 6, generator=g)
    virtual, real = str(tmp_path / "virtual"), str(tmp_path / "real")
    for path, x in ((virtual, samples), (real, samples * 2 - 1)):
        for mode in ("videos", "grids", "images"):
            SU.perform_save_locally(path, x, mode, "NUSCENES", 12)
    assert seen == [(False, False), (False, True), (False, False), (True, False), (True, True), (True, False)]
    for path in (virtual, real):
        assert sorted(os.listdir(path)) == ["grids", "images", "videos"]
        assert sorted(os.listdir(os.path.join(path, "images"))) == [f"NUSCENES_000012_{i:04}.png" for i in range(3)]
        assert os.listdir(os.path.join(path, "grids")) == ["NUSCENES_000012.png"]
        video = os.listdir(os.path.join(path, "videos"))
        assert video in (["NUSCENES_000012.apng"], ["NUSCENES_000012.mp4"])
    want = (255.0 * samples.numpy().transpose(0, 2, 3, 1)).astype(np.uint8)
    for i in range(3):
        assert np.array_equal(np.asarray(Image.open(os.path.join(virtual, "images", f"NUSCENES_000012_{i:04}.png"))), want[i])
    if video == ["NUSCENES_000012.apng"]:
        assert np.array_equal(SU.read_video_frames(os.path.join(virtual, "videos", video[0])), want)
        with Image.open(os.path.join(virtual, "videos", video[0])) as im:
            assert im.n_frames == 3 and im.info["duration"] == 100.0
        # a still video (the IMG dataset repeats one picture): every frame must stay a frame of its own
        still = np.repeat(want[:1], 4, 0)
        path = SU.save_video(str(tmp_path / "still"), still)
        assert np.array_equal(SU.read_video_frames(path), still)
    with pytest.raises(AssertionError):
        SU.perform_save_locally(virtual, samples, "gifs", "NUSCENES", 0)


def test_size_rule_names_the_constraint():
    from vista_amd import sample_utils as SU
    SU.check_sizes(576, 1024, 25)
    SU.check_sizes(576, 1024, 25, n_rounds=4, n_conds=3)
    SU.check_sizes(128, 256, 5)
    with pytest.raises(ValueError, match=r"attention level 2 has S = 18 x 34 = 612 .*S % 8 == 0"):
        SU.check_sizes(576, 1088, 25)
    with pytest.raises(ValueError, match=r"attention level 3 has S = 2 x 3 = 6 "):   # the middle block's level
        SU.check_sizes(128, 192, 25)
    with pytest.raises(ValueError, match="vk_attn_temporal_bf16"):
        SU.check_sizes(576, 1024, 33)
    with pytest.raises(ValueError, match="multiples of 8"):
        SU.check_sizes(580, 1024, 25)
    with pytest.raises(ValueError, match="multiples of 8 "):
        SU.check_sizes(576 + 32, 1024, 25)
    with pytest.raises(ValueError, match="carries 3 frames"):
        SU.check_sizes(576, 1024, 3, n_rounds=2)
    with pytest.raises(ValueError, match="n_conds"):
        SU.check_sizes(576, 1024, 5, n_conds=6)


def test_cli_refuses_a_bad_size_before_building_anything(monkeypatch):
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused size"))
    with pytest.raises(ValueError, match="attention level"):
        sample.main(["--height", "576", "--width", "1088"])
    with pytest.raises(ValueError, match="n_frames 40"):
        sample.main(["--n_frames", "40"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the refusal of a process without a GPU")
def test_init_model_refuses_a_cpu_only_process():
    from vista_amd import sample_utils as SU
    from vista_amd._lib import VistaHipError
    with pytest.raises(VistaHipError, match="no GPU"):
        SU.init_model({"config": None, "ckpt": "does-not-exist.safetensors"})
    from vista_amd import ops
    with pytest.raises(VistaHipError):
        ops.load_img_batch(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 8, 8)
    with pytest.raises(VistaHipError):
        ops.frames_to_u8(torch.zeros(1, 3, 8, 8))


def test_load_into_routes_encoder_and_conditioner_slices():
    """checkpoint.load_into(encoder=, conditioner=): `first_stage_model.encoder.*` and `conditioner.*` reach their modules with the prefixes
    stripped, missing / unexpected keys are reported per component, and without the new arguments the report is what it was."""
    import torch.nn as nn
    from vista_amd import checkpoint

    class Box(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Linear(2, 2)
    unet, dec, enc, cond = Box(), Box(), Box(), Box()
    sd = {}
    for prefix, fill in (("model.diffusion_model.", 1.0), ("first_stage_model.decoder.", 2.0), ("first_stage_model.encoder.", 3.0), ("conditioner.", 4.0)):
        sd[prefix + "a.weight"] = torch.full((2, 2), fill)
    sd["conditioner.extra"] = torch.zeros(1)
    rep = checkpoint.load_into(sd, unet=unet, decoder=dec, encoder=enc, conditioner=cond, verbose=False)
    assert [float(m.a.weight.detach()[0, 0]) for m in (unet, dec, enc, cond)] == [1.0, 2.0, 3.0, 4.0]
    assert rep == {"unet": (["a.bias"], []), "decoder": (["a.bias"], []), "encoder": (["a.bias"], []), "conditioner": (["a.bias"], ["extra"])}
    assert sorted(checkpoint.load_into(sd, unet=unet, decoder=dec, verbose=False)) == ["decoder", "unet"]


def test_first_stage_entry_of_the_overlay_and_the_reference_config_build_the_same_module():
    import yaml
    from vista_amd import config
    from vista_amd.models.autoencoder import AutoencodingEngine, DiagonalGaussianRegularizer
    from vista_amd.util import instantiate_from_config
    cfg = config.load_config()
    assert "first_stage_config" not in cfg["model"]["params"], "the overlay's model: entry stays what the reference file is merged under"
    ours = instantiate_from_config(cfg["first_stage"])
    ref_cfg = yaml.safe_load(open(os.path.join(GOLD, "vista_inference.yaml")))["model"]["params"]
    theirs = instantiate_from_config(ref_cfg["first_stage_config"])
    assert type(ours) is type(theirs) is AutoencodingEngine and type(theirs.regularization) is DiagonalGaussianRegularizer
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}  # noqa: E731
    assert shapes(ours) == shapes(theirs) and any(k.startswith("encoder.") for k in shapes(ours)) and any(k.startswith("decoder.") for k in shapes(ours))
    assert cfg["pipeline"] == {"scale_factor": ref_cfg["scale_factor"], "en_and_decode_n_samples_a_time": ref_cfg["en_and_decode_n_samples_a_time"]}
    assert cfg["first_stage"]["params"]["encoder_config"]["params"] == {k: v for k, v in ref_cfg["first_stage_config"]["params"]["encoder_config"]["params"].items()}
