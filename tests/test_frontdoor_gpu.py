"""The sampling front door on the MI355X: the two image I/O kernels (csrc/image_io.hip), the pipeline factory and the CLI.

No tolerance anywhere: the resize is compared with Pillow's integers (tests/golden/image_io.npz, made by tools/make_golden_image_io.py, and live
Pillow where it imports), the 8-bit conversion with numpy's float32 expressions of the reference's perform_save_locally, the grid with a numpy
restatement of torchvision.utils.make_grid (torchvision itself is not installed here: parity with the real make_grid is unpinned), and the
pipeline with a second route through the same deterministic kernels."""
import copy
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
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("wide", "tall", "exact", "cols")
UC_KEYS = ["cond_frames", "cond_frames_without_noise", "command", "trajectory", "speed", "angle", "goal"]


# ---- kernel (a): crop + Lanczos resize + normalise --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_load_img_batch_equals_pillow_golden(name):
    from vista_amd import ops
    g = np.load(os.path.join(GOLD, "image_io.npz"))
    th, tw = (int(v) for v in g["target"])
    got = ops.load_img_batch(torch.from_numpy(g[name + "_src"]).cuda()[None], th, tw)
    assert got.dtype == torch.float32 and got.shape == (1, 3, th, tw)
    assert torch.equal(got[0].cpu(), torch.from_numpy(g[name + "_f32"])), name
    # the same through an explicit box, and the bytes behind the values
    box = tuple(int(v) for v in g[name + "_box"])
    again = ops.load_img_batch(torch.from_numpy(g[name + "_src"]).cuda(), th, tw, box=box)
    assert torch.equal(again, got)
    assert np.array_equal(np.rint((got[0].cpu().numpy() + 1.0) * 127.5).astype(np.uint8).transpose(1, 2, 0), g[name + "_u8"])


def test_load_img_batch_full_size_and_odd_widths_equal_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    from vista_amd import ops
    from vista_amd.image_io import crop_box
    rng = np.random.default_rng(11)
    for h, w, oh, ow in ((900, 1600, 576, 1024), (200, 300, 576, 1024), (97, 131, 63, 125), (131, 97, 50, 70), (64, 64, 64, 64)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        left, top, cw, ch = crop_box(w, h, oh, ow)
        pil = Image.fromarray(img).crop((left, top, left + cw, top + ch)).resize((ow, oh), resample=Image.LANCZOS)
        want = torch.from_numpy(np.asarray(pil)).permute(2, 0, 1).to(torch.float32).div(255) * 2.0 - 1.0   # ToTensor, then x * 2.0 - 1.0
        got = ops.load_img_batch(torch.from_numpy(img).cuda(), oh, ow)[0].cpu()
        assert torch.equal(got, want), (h, w, oh, ow, int((got != want).sum()))


def test_load_img_batch_of_five_equals_five_single_calls_and_bad_boxes_are_refused():
    from vista_amd import ops
    from vista_amd._lib import VistaHipError
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (5, 90, 170, 3), generator=g, dtype=torch.uint8).cuda()
    batch = ops.load_img_batch(frames, 64, 128)
    for i in range(5):
        assert torch.equal(batch[i], ops.load_img_batch(frames[i], 64, 128)[0])
    assert not torch.equal(batch[0], batch[1])
    for box in ((0, 0, 0, 90), (0, 0, 170, 0), (10, 0, 170, 90), (0, 1, 170, 90), (-1, 0, 100, 90)):
        with pytest.raises(VistaHipError, match="-22"):
            ops.load_img_batch(frames, 64, 128, box=box)
    with pytest.raises(TypeError):
        ops.load_img_batch(frames.float(), 64, 128)
    with pytest.raises(ValueError):
        ops.load_img_batch(frames[..., :2], 64, 128)


def test_load_img_reads_files_like_the_reference(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from vista_amd import sample_utils as SU
    from vista_amd.image_io import crop_box
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (120, 400, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    Image.fromarray(rgb[..., 0]).save(tmp_path / "gray.png")     # mode "L": converted to RGB like the reference does
    Image.fromarray(rgb[:100, :100]).save(tmp_path / "small.png")

    def reference(path):
        image = Image.open(path).convert("RGB")
        w, h = image.size
        left, top, cw, ch = crop_box(w, h, 128, 256)
        image = image.crop((left, top, left + cw, top + ch)).resize((256, 128), resample=Image.LANCZOS)
        return torch.from_numpy(np.asarray(image)).permute(2, 0, 1).to(torch.float32).div(255) * 2.0 - 1.0
    names = [str(tmp_path / n) for n in ("rgb.png", "gray.png", "small.png", "rgb.png")]
    one = SU.load_img(names[0], 128, 256)
    assert one.is_cuda and one.shape == (3, 128, 256) and torch.equal(one.cpu(), reference(names[0]))
    seq = SU.load_img_seq(names, 128, 256)
    assert seq.shape == (4, 3, 128, 256)
    for i, n in enumerate(names):
        assert torch.equal(seq[i].cpu(), reference(n)), n


# ---- kernel (b): frames / grid to 8 bit ---------------------------------------------------------------------------------------------------
def _unit_samples(n, H, W, seed):
    """[0, 1] values that include exact 0, 1 and every k/255 (and its float32 neighbours, where the truncation decides)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, H, W, generator=g)
    flat = x.view(-1)
    k = torch.arange(256, dtype=torch.float32) / 255
    special = torch.cat([k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-1.0)).clamp_(0, 1), torch.tensor([0.0, 1.0, 0.5])])
    special = special[torch.randperm(special.numel(), generator=g)][:flat.numel()]   # (a small tensor takes as many as fit)
    flat[torch.randperm(flat.numel(), generator=g)[:special.numel()]] = special
    return x


def _numpy_u8(x, real):
    a = x.numpy()
    a = 255.0 * (a + 1.0) / 2.0 if real else 255.0 * a     # the reference's expressions (sample_utils.py:106-109), float32 throughout
    assert a.dtype == np.float32
    return a.astype(np.uint8)


def _numpy_make_grid(x, padding=2):
    """torchvision.utils.make_grid(x, nrow=int(n ** 0.5)) restated (defaults: padding 2, pad_value 0; one image is returned as it is)."""
    n, c, H, W = x.shape
    if n == 1:
        return x[0]
    xmaps = min(int(n ** 0.5), n)
    ymaps = -(-n // xmaps)
    grid = np.zeros((c, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), dtype=x.dtype)
    for k in range(n):
        y0, x0 = k // xmaps * (H + padding) + padding, k % xmaps * (W + padding) + padding
        grid[:, y0:y0 + H, x0:x0 + W] = x[k]
    return grid


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("n,H,W", [(3, 16, 32), (4, 9, 13), (1, 72, 128)])
def test_frames_to_u8_equals_numpy_float32(n, H, W, real):
    from vista_amd import ops
    x = _unit_samples(n, H, W, seed=n * H + W)
    if real:
        x = x * 2.0 - 1.0
        x.view(-1)[:2] = torch.tensor([-1.0, 1.0])
    got = ops.frames_to_u8(x.cuda(), real=real)
    assert got.dtype == torch.uint8 and got.shape == (n, H, W, 3)
    want = _numpy_u8(x, real).transpose(0, 2, 3, 1)
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    assert want.min() == 0 and want.max() == 255


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("n", [1, 5, 25, 47])
def test_grid_equals_numpy_make_grid(n, real):
    from vista_amd import ops
    from vista_amd.image_io import grid_geometry
    for H, W in ((8, 12), (9, 14)):          # canvas widths that are / are not multiples of 4 for some n
        x = _unit_samples(n, H, W, seed=n + H)
        if real:
            x = x * 2.0 - 1.0
        got = ops.frames_to_u8(x.cuda(), real=real, grid=True).cpu().numpy()
        want = _numpy_u8(torch.from_numpy(_numpy_make_grid(x.numpy())), real).transpose(1, 2, 0)
        assert got.shape == want.shape == grid_geometry(n, H, W)[2:4] + (3,)
        assert np.array_equal(got, want), (n, H, W)
    if n > 1:
        assert (got[0, 0] == (127 if real else 0)).all(), "the border is the map of make_grid's pad value 0"


def test_frames_to_u8_refuses_what_it_cannot_take():
    from vista_amd import _lib, ops
    with pytest.raises(TypeError):
        ops.frames_to_u8(torch.zeros(1, 3, 4, 4, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        ops.frames_to_u8(torch.zeros(1, 4, 4, 4).cuda())
    x, out = torch.zeros(2, 3, 4, 4).cuda(), torch.zeros(2, 4, 4, 3, dtype=torch.uint8).cuda()
    lib, p = _lib.load(), ops._p
    assert lib.vk_frames_to_u8(p(x), p(out), 2, 4, 4, 1, 0, 2, ops._stream()) == -22      # real must be 0 / 1
    assert lib.vk_frames_to_u8(p(x), p(out), 2, 4, 4, 3, 2, 0, ops._stream()) == -22      # more columns than images
    assert lib.vk_frames_to_u8(p(x), None, 2, 4, 4, 1, 0, 0, ops._stream()) == -22
    assert lib.vk_frames_to_u8(p(x), p(out), 0, 4, 4, 1, 0, 0, ops._stream()) == -22


# ---- the pipeline: one config + one checkpoint -> VistaPipeline ----------------------------------------------------------------------------
T, H, W, STEPS = 5, 128, 256, 3
TINY_CLIP = dict(width=320, layers=2, heads=4, mlp=1280, patch=14, image=224, embed=1024)   # the tiny tower of the goldens, 1024-d output for the UNet


def _tiny_config():
    """The shipped config at the shapes of the tiny goldens: model_channels 64, the 64-channel first stage, a 2-layer image tower, 5 frames."""
    from oracle.make_golden_vae import TINY
    from vista_amd import config
    cfg = copy.deepcopy(config.load_config())
    mp = cfg["model"]["params"]
    mp["num_frames"] = mp["denoiser_config"]["params"]["num_frames"] = T
    mp["network_config"]["params"]["model_channels"] = 64
    embs = mp["conditioner_config"]["params"]["emb_models"]
    embs[0]["params"]["open_clip_embedding_config"]["params"]["arch"] = dict(TINY_CLIP)
    embs[3]["params"]["encoder_config"]["params"]["ddconfig"]["ch"] = TINY["ch"]
    fs = cfg["first_stage"]["params"]
    fs["encoder_config"]["params"] = dict(TINY)
    fs["decoder_config"]["params"] = dict(TINY, video_kernel_size=[3, 1, 1])
    return cfg


def _seeded(module, seed):
    from vista_amd import synth
    return synth.seeded_state_dict({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed)


@pytest.fixture(scope="module", autouse=True)
def _process_wide_graph_state_as_found():
    """Graph replay with concurrent halves registers per-process state: a second split-K workspace (slot 1), the warm-up stream and the side
    stream of half 1. Other modules of the suite count those entries from their own runs, so this module leaves the registries as it found
    them. A captured graph holds its own reference to its workspace, so dropping the registry entry frees nothing a live graph needs."""
    from vista_amd import ops
    from vista_amd.modules.diffusionmodules.sampling import FusedLoop
    held = [(d, dict(d)) for d in (ops._GRAPH_TLS.ws, FusedLoop._WARM_STREAMS, FusedLoop._CFG_STREAMS)]
    yield
    torch.cuda.synchronize()
    for d, before in held:
        d.clear()
        d.update(before)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A tiny config, a seeded checkpoint, five pictures and an annotation file on disk + the same modules assembled by hand."""
    import yaml
    from PIL import Image
    from safetensors.torch import save_file
    from vista_amd.models.diffusion import encode_first_stage
    from vista_amd.modules.diffusionmodules.wrappers import OpenAIWrapper
    from vista_amd.sample_utils import VistaPipeline
    from vista_amd.util import instantiate_from_config
    d = tmp_path_factory.mktemp("frontdoor")
    cfg = _tiny_config()
    cfg_path = str(d / "tiny.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    mp = cfg["model"]["params"]
    net, den = instantiate_from_config(mp["network_config"]), instantiate_from_config(mp["denoiser_config"])
    cond, fs = instantiate_from_config(mp["conditioner_config"]), instantiate_from_config(cfg["first_stage"])
    sd = {}
    for prefix, module, seed in (("model.diffusion_model.", net, 0), ("conditioner.", cond, 1), ("first_stage_model.", fs, 2)):
        part = _seeded(module, seed)
        module.load_state_dict(part, strict=True)
        sd.update({prefix + k: v.contiguous() for k, v in part.items()})
    ckpt = str(d / "tiny.safetensors")
    save_file(sd, ckpt)
    for m in (net, cond, fs):
        m.cuda().eval()
    sf, n_a_time = cfg["pipeline"]["scale_factor"], cfg["pipeline"]["en_and_decode_n_samples_a_time"]
    hand = VistaPipeline(OpenAIWrapper(net), den, decoder=fs.decoder, conditioner=cond, scale_factor=sf, en_and_decode_n_samples_a_time=n_a_time,
                         encode_fn=lambda x: encode_first_stage(fs, x, sf, n_a_time))
    rng = np.random.default_rng(4)
    (d / "data" / "cam").mkdir(parents=True)
    names = []
    for i in range(T):
        yy, xx = np.mgrid[0:180, 0:320]
        img = np.stack([127 + 120 * np.sin(xx / (9.0 + i) + c) * np.cos(yy / (7.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (180, 320, 3))
        names.append(f"cam/frame{i}.png")
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(d / "data" / names[-1])
    anno = str(d / "anno.json")
    with open(anno, "w") as f:
        json.dump([{"frames": names, "traj": [0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2], "cmd": 1, "speed": [], "angle": [], "z": 1.0,
                    "goal": [800.0, 450.0]}], f)
    return {"dir": d, "config": cfg_path, "ckpt": ckpt, "hand": hand, "data_root": str(d / "data"), "anno": anno,
            "frames": [str(d / "data" / n) for n in names]}


@pytest.fixture(scope="module")
def model(world):
    from vista_amd import sample_utils as SU
    return SU.init_model({"config": world["config"], "ckpt": world["ckpt"]})


def _hand_run(world, n_rounds, eager, seed, action=None):
    """What sample.run does, spelled out over the hand-assembled pipeline."""
    from vista_amd import ops
    from vista_amd import sample_utils as SU
    from vista_amd.modules.diffusionmodules.sampling import EulerEDMSampler
    from PIL import Image
    torch.manual_seed(seed)
    frames = torch.from_numpy(np.stack([np.asarray(Image.open(p).convert("RGB")) for p in world["frames"]])).cuda()
    images = ops.load_img_batch(frames, H, W)
    vd = {"fps": 10, "fps_id": 9, "motion_bucket_id": 127, "cond_frames_without_noise": images[:1], "cond_aug": 0.02,
          "cond_frames": images[:1] + 0.02 * torch.randn_like(images[:1])}
    vd.update(action or {})
    P = "vwm.modules.diffusionmodules."
    guider = ({"target": P + "guiders.TrianglePredictionGuider", "params": {"max_scale": 2.5, "min_scale": 1.0, "num_frames": T}} if n_rounds > 1
              else {"target": P + "guiders.VanillaCFG", "params": {"scale": 2.5}})
    sampler = EulerEDMSampler(num_steps=STEPS, discretization_config={"target": P + "discretizer.EDMDiscretization",
                                                                      "params": {"sigma_min": 0.002, "sigma_max": 700.0, "rho": 7.0}},
                              guider_config=guider, s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0, verbose=False, device="cuda")
    sampler.graph = sampler.cfg_streams = not eager
    return SU.do_sample(images, world["hand"], sampler, vd, num_rounds=n_rounds, num_frames=T, force_uc_zero_embeddings=UC_KEYS,
                        initial_cond_indices=[0])


def _run(model, world, n_rounds, eager, seed, action=None, **kw):
    from vista_amd import sample
    torch.manual_seed(seed)
    return sample.run(model, world["frames"], action, height=H, width=W, n_frames=T, n_rounds=n_rounds, n_steps=STEPS, cond_aug=0.02, eager=eager, **kw)


def test_init_model_builds_the_pipeline_and_reports_clean_loads(world, model, capsys):
    from vista_amd import checkpoint
    from vista_amd import sample_utils as SU
    from vista_amd.models.autoencoder import AutoencodingEngine
    from vista_amd.modules.diffusionmodules.denoiser import Denoiser
    from vista_amd.modules.diffusionmodules.wrappers import OpenAIWrapper
    from vista_amd.modules.encoders.modules import GeneralConditioner
    assert isinstance(model, SU.VistaPipeline) and isinstance(model.model, OpenAIWrapper) and isinstance(model.denoiser, Denoiser)
    assert isinstance(model.conditioner, GeneralConditioner) and isinstance(model.first_stage_model, AutoencodingEngine)
    assert model.scale_factor == 0.18215 and model.en_and_decode_n_samples_a_time == 14 and model.denoiser.num_frames == T
    assert all(p.is_cuda for p in model.model.parameters()) and all(p.is_cuda for p in model.conditioner.parameters())
    hand = world["hand"]
    for a, b in ((model.model, hand.model), (model.conditioner, hand.conditioner), (model.decoder, hand.decoder)):
        sa, sb = a.state_dict(), b.state_dict()
        assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    sd = checkpoint.load_checkpoint(world["ckpt"])
    rep = checkpoint.load_into(sd, unet=model.model.diffusion_model, decoder=model.decoder, encoder=model.first_stage_model.encoder,
                               conditioner=model.conditioner, verbose=True)
    assert rep == {k: ([], []) for k in ("unet", "decoder", "encoder", "conditioner")} and "keys" not in capsys.readouterr().out
    sd.pop("conditioner.embedders.0.open_clip.model.visual.proj")
    sd["first_stage_model.encoder.stray"] = torch.zeros(1)
    rep = checkpoint.load_into(sd, encoder=model.first_stage_model.encoder, conditioner=model.conditioner)
    out = capsys.readouterr().out
    assert rep["conditioner"] == (["embedders.0.open_clip.model.visual.proj"], []) and rep["encoder"] == ([], ["stray"])
    assert "Missing keys: ['embedders.0.open_clip.model.visual.proj']" in out and "Unexpected keys: ['stray']" in out

@pytest.mark.parametrize("n_rounds", [1, 2], ids=["one_round_vanilla_cfg", "two_rounds_triangle"])
def test_run_equals_the_hand_assembled_pipeline_bitwise(world, model, n_rounds):
    action = {"trajectory": torch.tensor([0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2])}
    got = _run(model, world, n_rounds, eager=False, seed=7, action=action)
    want = _hand_run(world, n_rounds, eager=False, seed=7, action=action)
    frames = n_rounds * (T - 3) + 3
    assert got[0].shape == (frames, 3, H, W) and got[1].shape == (frames, 4, H // 8, W // 8) and got[2].shape == (T, 3, H, W)
    assert torch.isfinite(got[0]).all() and 0.0 <= float(got[0].min()) and float(got[0].max()) <= 1.0 and float(got[0].std()) > 0
    for name, a, b in zip(("samples", "samples_z", "inputs"), got, want):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    other = _run(model, world, n_rounds, eager=False, seed=8, action=action)
    assert not torch.equal(other[1], got[1]), "another seed, another sample"


@pytest.mark.parametrize("n_rounds", [1, 2])
def test_graph_replay_with_concurrent_halves_equals_eager_bitwise(world, model, n_rounds):
    timings = {}
    fast = _run(model, world, n_rounds, eager=False, seed=5, timings=timings)
    slow = _run(model, world, n_rounds, eager=True, seed=5)
    for name, a, b in zip(("samples", "samples_z", "inputs"), fast, slow):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert sorted(timings) == ["condition", "decode", "encode", "load", "sample"] and all(v >= 0 for v in timings.values())


def test_cli_writes_what_run_returns(world, model):
    """`python -m vista_amd.sample` once, as a fresh child process: its files against run() in this process (same seed, same kernels)."""
    from PIL import Image
    from vista_amd import ops, sample
    from vista_amd import sample_utils as SU
    from vista_amd.image_io import grid_geometry
    save = str(world["dir"] / "out")
    cmd = [sys.executable, "-m", "vista_amd.sample", "--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES",
           "--data_root", world["data_root"], "--anno_file", world["anno"], "--action", "traj", "--n_frames", str(T), "--height", str(H),
           "--width", str(W), "--n_steps", str(STEPS), "--cond_aug", "0.02", "--rand_gen", "--low_vram", "--save", save]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "--low_vram: accepted, no effect" in res.stdout and "Loading model from" in res.stdout and "Missing keys" not in res.stdout

    sample.seed_everything(23)   # the CLI's default --seed
    frame_list, index, total, action = SU.get_sample(0, "NUSCENES", T, "traj", data_root=world["data_root"], anno_file=world["anno"])
    assert (index, total) == (0, 1) and list(action) == ["trajectory"]
    samples, _, inputs = sample.run(model, frame_list, action, height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02)
    for sub, x, real in (("virtual", samples, False), ("real", inputs, True)):
        want = ops.frames_to_u8(x, real=real).cpu().numpy()
        files = sorted(os.listdir(os.path.join(save, sub, "images")))
        assert files == [f"NUSCENES_000000_{i:04}.png" for i in range(T)]
        for i, f in enumerate(files):
            assert np.array_equal(np.asarray(Image.open(os.path.join(save, sub, "images", f))), want[i]), (sub, f)
        grid = np.asarray(Image.open(os.path.join(save, sub, "grids", "NUSCENES_000000.png")))
        assert grid.shape == grid_geometry(T, H, W)[2:4] + (3,) == (3 * (H + 2) + 2, 2 * (W + 2) + 2, 3)
        assert np.array_equal(grid, ops.frames_to_u8(x, real=real, grid=True).cpu().numpy())
        videos = os.listdir(os.path.join(save, sub, "videos"))
        assert videos in (["NUSCENES_000000.apng"], ["NUSCENES_000000.mp4"])
        if videos[0].endswith(".apng"):
            assert np.array_equal(SU.read_video_frames(os.path.join(save, sub, "videos", videos[0])), want)
    # the inputs are the files themselves through load_img
    assert torch.equal(inputs, SU.load_img_seq(world["frames"], H, W))
