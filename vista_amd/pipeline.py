"""The standalone front door: everything between a checkpoint plus a folder of pictures and saved frames that the reference keeps in
sample.py / sample_utils.py:20-229 and this package lacked -- model and sampler factories, dataset lookup, image loading and saving.
Exported from vista_amd.sample_utils (where the reference's users look); `python -m vista_amd.sample` is the CLI over it.

Same names, arguments and defaults as the reference. Differences, all stated where they occur: the pictures are cropped, resized and normalised
on the GPU (ops.load_img_batch, Pillow's LANCZOS byte for byte), frames are converted to 8 bit on the GPU (ops.frames_to_u8), nothing is
shuffled between host and device (`--low_vram` is a no-op: 288 GB of HBM keep every stage resident), and without `imageio` a video is written as
an animated PNG instead of an mp4 (or, with VISTA_VIDEO=mjpeg, as Motion-JPEG in AVI whose frames are encoded on the GPU: video_format, README
"Videos"). With VISTA_PNG=hip every PNG stream -- images, grids, the animated PNG -- is filtered and deflated on the GPU (png_format, README "Pictures").
"""
import json
import math
import os

import torch

from . import checkpoint, config, image_io, ops
from ._lib import VistaHipError
from .util import instantiate_from_config

VERSION2SPECS = {"vwm": {"config": config.CONFIG_PATH, "ckpt": "ckpts/vista.safetensors"}}
DATASET2SOURCES = {"NUSCENES": {"data_root": "data/nuscenes", "anno_file": "annos/nuScenes_val.json"}, "IMG": {"data_root": "image_folder"}}
_P = "vwm.modules.diffusionmodules."   # (reference target strings: vista_amd.util.instantiate_from_config maps them onto this package)


# ---- sampler factories (sample_utils.py:140-229) ----------------------------------------------------------------------------------------
def get_discretization(discretization):
    if discretization == "EDMDiscretization":
        return {"target": _P + "discretizer.EDMDiscretization", "params": {"sigma_min": 0.002, "sigma_max": 700.0, "rho": 7.0}}
    if discretization == "LegacyDDPMDiscretization":
        raise NotImplementedError("LegacyDDPMDiscretization is not built in vista_amd: Vista samples with EDMDiscretization "
                                  "(sigma_min 0.002, sigma_max 700, rho 7)")
    raise NotImplementedError(f"unknown discretization {discretization!r}")


def get_guider(guider="LinearPredictionGuider", cfg_scale=2.5, num_frames=25):
    if guider == "IdentityGuider":
        return {"target": _P + "guiders.IdentityGuider"}
    if guider == "VanillaCFG":
        return {"target": _P + "guiders.VanillaCFG", "params": {"scale": cfg_scale}}
    if guider in ("LinearPredictionGuider", "TrianglePredictionGuider"):
        return {"target": _P + "guiders." + guider, "params": {"max_scale": cfg_scale, "min_scale": 1.0, "num_frames": num_frames}}
    raise NotImplementedError(f"unknown guider {guider!r}")


SAMPLERS = ("EulerEDMSampler", "DPMPP2MSampler")   # the reference ships the first; the second (DPM-Solver++(2M)) is this package's


def sampler_name(sampler=None):
    """The sampler a front door builds: `sampler` if given, else the environment hook VISTA_SAMPLER, else EulerEDMSampler (the reference's).
    The one place the hook is read. A name that is not built is refused here, by name, before a model is built."""
    name = sampler if sampler is not None else (os.environ.get("VISTA_SAMPLER") or "EulerEDMSampler")
    if name not in SAMPLERS:
        where = " (environment hook VISTA_SAMPLER)" if sampler is None else ""
        raise ValueError(f"Unknown sampler {name}{where}: one of {', '.join(SAMPLERS)}")
    return name


VIDEO_FORMATS = ("apng", "mjpeg")


def video_format():
    """-> (format, quality): how the front doors write videos. The one place the environment hooks VISTA_VIDEO and VISTA_VIDEO_QUALITY are read.
    VISTA_VIDEO unset or `apng`: an mp4 through imageio where it is importable, else an animated PNG -- what was written before the hook existed,
    byte for byte. `mjpeg`: `<stem>.avi`, Motion-JPEG frames encoded on the GPU (video.py) at VISTA_VIDEO_QUALITY (1 .. 100, default 90).
    An unknown format or a bad quality is refused here, by name, before a model is built."""
    name = os.environ.get("VISTA_VIDEO") or "apng"
    if name not in VIDEO_FORMATS:
        raise ValueError(f"Unknown video format {name} (environment hook VISTA_VIDEO): one of {', '.join(VIDEO_FORMATS)}")
    text = os.environ.get("VISTA_VIDEO_QUALITY") or "90"
    try:
        quality = int(text)
    except ValueError:
        quality = 0
    if not 1 <= quality <= 100:
        raise ValueError(f"Bad JPEG quality {text} (environment hook VISTA_VIDEO_QUALITY): a whole number from 1 to 100")
    return name, quality


PNG_FORMATS = ("pillow", "hip")


def png_format():
    """-> how the package codes the PNG streams it writes. The one place the environment hook VISTA_PNG is read. Unset or `pillow`: Pillow on the
    host, every file byte for byte what was written before the hook existed. `hip`: the rows are filtered and deflated on the GPU (png.py,
    csrc/png.hip) -- the per-frame images, the grids and the animated PNG. An unknown value is refused here, by name, before a model is built."""
    name = os.environ.get("VISTA_PNG") or "pillow"
    if name not in PNG_FORMATS:
        raise ValueError(f"Unknown PNG coder {name} (environment hook VISTA_PNG): one of {', '.join(PNG_FORMATS)}")
    return name


def eval_clip():
    """-> whether `evaluate` adds the CLIP-space scores of perceptual.py to its records. The one place the environment hook VISTA_EVAL_CLIP is
    read. Unset or `0`: no, and every record, summary, printed line and file is what was written before the hook existed. `1`: yes. Any other
    value is refused here, by name, before a model is built."""
    text = os.environ.get("VISTA_EVAL_CLIP") or "0"
    if text not in ("0", "1"):
        raise ValueError(f"Bad value {text} (environment hook VISTA_EVAL_CLIP): 0 or 1")
    return text == "1"


def eval_motion():
    """-> whether `evaluate` adds the motion scores of motion.py (block-matching optical flow) to its records. The one place the environment
    hook VISTA_EVAL_MOTION is read. Unset or `0`: no, and every record, summary, printed line and file is what was written before the hook
    existed. `1`: yes. Any other value is refused here, by name, before a model is built."""
    text = os.environ.get("VISTA_EVAL_MOTION") or "0"
    if text not in ("0", "1"):
        raise ValueError(f"Bad value {text} (environment hook VISTA_EVAL_MOTION): 0 or 1")
    return text == "1"


def scene_ranks():
    """-> whether `evaluate`, `denoise_loss` and `step_sweep` run scene-per-rank under torch.distributed.run (frontdoor.SceneRanks: the k-th
    scene of the walk on rank k mod WORLD_SIZE, the records merged by rank 0). The one place the environment hook VISTA_SCENE_RANKS is read.
    Unset or `0`: no, and WORLD_SIZE > 1 is refused as it was before the hook existed. `1`: yes; with WORLD_SIZE unset or 1 the run is the
    single-process run. Any other value is refused here, by name, before a model is built."""
    text = os.environ.get("VISTA_SCENE_RANKS") or "0"
    if text not in ("0", "1"):
        raise ValueError(f"Bad value {text} (environment hook VISTA_SCENE_RANKS): 0 or 1")
    return text == "1"


def get_sampler(sampler, steps, discretization_config, guider_config):
    if sampler == "DPMPP2MSampler":
        from .modules.diffusionmodules.sampling import DPMPP2MSampler
        return DPMPP2MSampler(num_steps=steps, discretization_config=discretization_config, guider_config=guider_config, verbose=False)
    if sampler != "EulerEDMSampler":
        raise ValueError(f"Unknown sampler {sampler}")
    from .modules.diffusionmodules.sampling import EulerEDMSampler
    return EulerEDMSampler(num_steps=steps, discretization_config=discretization_config, guider_config=guider_config,
                           s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0, verbose=False)


def init_sampling(sampler="EulerEDMSampler", guider="VanillaCFG", discretization="EDMDiscretization", steps=50, cfg_scale=2.5, num_frames=25):
    return get_sampler(sampler, steps, get_discretization(discretization), get_guider(guider, cfg_scale, num_frames))


def init_embedder_options(keys):
    """The demo's fixed conditioning scalars (sample_utils.py:83-93): 10 fps -> fps_id 9, motion bucket 127."""
    value_dict = {}
    for key in keys:
        if key in ("fps_id", "fps"):
            value_dict["fps"] = 10
            value_dict["fps_id"] = 10 - 1
        elif key == "motion_bucket_id":
            value_dict["motion_bucket_id"] = 127
    return value_dict


# ---- sizes the kernels take ---------------------------------------------------------------------------------------------------------------
def check_sizes(height, width, n_frames, n_rounds=1, n_conds=1, unet_params=None):
    """Refuses, by naming the constraint, a frame size or window length the kernels cannot take -- before any model is built. Derived from the
    argument checks of the entry points a run goes through (include/vista_hip.h):
      * first stage: three stride-2 convolutions down, three x2 upsamples back: height and width multiples of 8; its mid-block attention
        (modules/diffusionmodules/model.py AttnBlock) takes token counts that are multiples of 64
      * UNet: len(channel_mult) - 1 stride-2 convolutions whose skip tensors must meet the x2 upsampled ones again: latent height and width
        multiples of 2 ** (levels - 1); attn_spatial_launch (vk_attn_spatial_*) takes S % 8 == 0 at every level that holds a transformer
        (attention_resolutions, and the middle block at the deepest level)
      * vk_attn_temporal_bf16: 1 <= T <= 32 frames per window
      * the rollout carries 3 frames from one window to the next: more than 3 frames per window when n_rounds > 1."""
    p = config.vista_unet_kwargs() if unet_params is None else unet_params
    if n_frames < 1 or n_frames > 32:
        raise ValueError(f"--n_frames {n_frames}: the temporal attention kernel (vk_attn_temporal_bf16) takes 1 <= T <= 32 frames per window")
    if n_rounds > 1 and n_frames <= 3:
        raise ValueError(f"--n_frames {n_frames}: a multi-round rollout carries 3 frames between windows and needs more than 3 per window")
    if not 1 <= n_conds <= n_frames:
        raise ValueError(f"--n_conds {n_conds}: between 1 and n_frames ({n_frames}) condition frames")
    if height <= 0 or width <= 0 or height % 8 or width % 8:
        raise ValueError(f"--height {height} --width {width}: the first stage maps 8 x 8 pixels to one latent; both must be positive multiples of 8")
    h, w = height // 8, width // 8
    if (h * w) % 64:
        raise ValueError(f"--height {height} --width {width}: the first stage's mid-block attention takes H/8 * W/8 = {h} x {w} = {h * w} tokens, "
                         "which must be a multiple of 64")
    levels = len(p["channel_mult"])
    step = 2 ** (levels - 1)
    if h % step or w % step:
        raise ValueError(f"--height {height} --width {width}: the UNet halves the {h} x {w} latent {levels - 1} times and doubles it back onto its skip "
                         f"tensors; H/8 and W/8 must be multiples of {step} (height and width of {8 * step})")
    for level in range(levels):
        ds = 2 ** level
        if ds in p["attention_resolutions"] or level == levels - 1:
            S = (h // ds) * (w // ds)
            if S % 8:
                raise ValueError(f"--height {height} --width {width}: attention level {level} has S = {h // ds} x {w // ds} = {S} tokens per frame; "
                                 "the spatial attention kernels (attn_spatial_launch) take S % 8 == 0 at every level")


# ---- model factory (sample_utils.py:20-80) ------------------------------------------------------------------------------------------------
def _plain(cfg):
    """OmegaConf containers (if a caller hands one in) -> plain dicts / lists."""
    try:
        from omegaconf import OmegaConf
        if OmegaConf.is_config(cfg):
            return OmegaConf.to_container(cfg, resolve=True)
    except ImportError:
        pass
    return cfg


def load_model_from_config(cfg, ckpt=None, verbose=True):
    """A ready `VistaPipeline` on the GPU from one config and one checkpoint. `cfg` is the shipped overlay (its top-level `first_stage:` /
    `pipeline:` entries carry what the overlay's `model:` does not) or the reference's full vista.yaml, unmodified (`model.params.first_stage_config`,
    `scale_factor`, `en_and_decode_n_samples_a_time`). Weights are loaded per component from `model.diffusion_model.*`, `first_stage_model.*` and
    `conditioner.*` with strict=False; missing and unexpected keys are printed the way the reference prints them."""
    if not torch.cuda.is_available():
        raise VistaHipError("init_model: no GPU is visible; vista_amd runs on the MI355X only (no CPU / eager fallback)")
    from .models.diffusion import encode_first_stage
    from .modules.diffusionmodules.wrappers import OpenAIWrapper
    from .sample_utils import VistaPipeline
    cfg = _plain(cfg)
    mp = cfg["model"]["params"]
    extra = cfg.get("pipeline", {})
    fs_cfg = mp.get("first_stage_config", cfg.get("first_stage"))
    if fs_cfg is None:
        raise KeyError("config has neither model.params.first_stage_config (the reference's vista.yaml) nor a top-level first_stage entry")
    scale_factor = mp.get("scale_factor", extra.get("scale_factor", 0.18215))
    n_a_time = mp.get("en_and_decode_n_samples_a_time", extra.get("en_and_decode_n_samples_a_time", 14))
    net = instantiate_from_config(mp["network_config"])
    denoiser = instantiate_from_config(mp["denoiser_config"])
    conditioner = instantiate_from_config(mp["conditioner_config"])
    first_stage = instantiate_from_config(fs_cfg)
    if ckpt is not None:
        if verbose:
            print(f"Loading model from {ckpt}")
        if ckpt.endswith(".bin"):   # a DeepSpeed training dump: what the reference's bin_to_st.py does to it, in memory
            sd = checkpoint.convert_training_checkpoint(torch.load(ckpt, map_location="cpu", weights_only=True))
        else:
            sd = checkpoint.load_checkpoint(ckpt)
        checkpoint.load_into(sd, unet=net, decoder=first_stage.decoder, encoder=first_stage.encoder, conditioner=conditioner, verbose=verbose)
    for m in (net, conditioner, first_stage):
        m.cuda().eval()
    pipe = VistaPipeline(OpenAIWrapper(net), denoiser, decoder=first_stage.decoder, conditioner=conditioner, scale_factor=scale_factor,
                         en_and_decode_n_samples_a_time=n_a_time,
                         encode_fn=lambda x: encode_first_stage(first_stage, x, scale_factor, n_a_time))
    pipe.first_stage_model = first_stage
    return pipe


def init_model(version_dict, load_ckpt=True):
    """version_dict = {"config": path of a YAML (default: the shipped overlay), "ckpt": path of vista.safetensors / a Lightning .ckpt}.
    A DeepSpeed `pytorch_model.bin` is converted first (checkpoint.convert_training_checkpoint, what the reference's bin_to_st.py does)."""
    if not torch.cuda.is_available():
        raise VistaHipError("init_model: no GPU is visible; vista_amd runs on the MI355X only (no CPU / eager fallback)")
    cfg = config.load_config(version_dict.get("config") or config.CONFIG_PATH)
    return load_model_from_config(cfg, version_dict.get("ckpt") if load_ckpt else None)


# ---- dataset lookup (sample.py:122-171) ---------------------------------------------------------------------------------------------------
def get_sample(selected_index=0, dataset_name="NUSCENES", num_frames=25, action_mode="free", data_root=None, anno_file=None):
    """-> (path_list, selected_index, total_length, action_dict). IMG: one picture of the folder, repeated; NUSCENES: the frames of one annotated
    scene plus, for an action mode, its trajectory / command / speed + steering angle / goal point, scaled as the reference scales them.
    `data_root` / `anno_file` default to the reference's DATASET2SOURCES."""
    if dataset_name not in DATASET2SOURCES:
        raise ValueError(f"Invalid dataset {dataset_name}")
    src = DATASET2SOURCES[dataset_name]
    data_root = src["data_root"] if data_root is None else data_root
    if dataset_name == "IMG":
        names = os.listdir(data_root)
        total = len(names)
        selected_index %= total
        return [os.path.join(data_root, names[selected_index])] * num_frames, selected_index, total, None
    anno_file = src["anno_file"] if anno_file is None else anno_file
    with open(anno_file, "r") as f:
        scenes = json.load(f)
    total = len(scenes)
    selected_index %= total
    scene = scenes[selected_index]
    paths = [os.path.join(data_root, scene["frames"][i]) for i in range(num_frames)]
    for path in paths:
        if not os.path.exists(path):
            raise FileNotFoundError(path)
    if action_mode == "free":
        return paths, selected_index, total, None
    action = {}
    if action_mode in ("traj", "trajectory"):
        action["trajectory"] = torch.tensor(scene["traj"][2:])
    elif action_mode in ("cmd", "command"):
        action["command"] = torch.tensor(scene["cmd"])
    elif action_mode == "steer":
        if scene["speed"]:       # a scene may carry no CAN bus record
            action["speed"] = torch.tensor(scene["speed"][1:])
        if scene["angle"]:
            action["angle"] = torch.tensor(scene["angle"][1:]) / 780
    elif action_mode == "goal":
        gx, gy = scene["goal"][0], scene["goal"][1]
        if scene["z"] > 0 and 0 < gx < 1600 and 0 < gy < 900:   # the goal point must project into the 1600 x 900 camera frame
            action["goal"] = torch.tensor([gx / 1600, gy / 900])
    else:
        raise ValueError(f"Unsupported action mode {action_mode}")
    return paths, selected_index, total, action


# ---- pictures in (sample.py:174-201) ------------------------------------------------------------------------------------------------------
def _decode_rgb(file_name):
    """PIL only decodes: (h, w, 3) uint8."""
    import numpy as np
    from PIL import Image
    if file_name is None:
        raise ValueError(f"Invalid image file {file_name}")
    with Image.open(file_name) as image:
        return np.array(image if image.mode == "RGB" else image.convert("RGB"), dtype=np.uint8)


def load_img_seq(file_names, target_height=320, target_width=576, device="cuda"):
    """The batched `load_img`: a list of files -> (n, 3, target_height, target_width) fp32 in [-1, 1] on `device`. A file that occurs several times
    (the IMG dataset repeats one picture) is decoded and resized once; frames of one size go through one kernel launch."""
    import numpy as np
    first, groups = {}, {}
    for name in file_names:
        if name not in first:
            first[name] = _decode_rgb(name)
            groups.setdefault(first[name].shape, []).append(name)
    done = {}
    for names in groups.values():
        stack = torch.from_numpy(np.stack([first[n] for n in names])).to(device)
        out = ops.load_img_batch(stack, target_height, target_width)
        for i, n in enumerate(names):
            done[n] = out[i]
    return torch.stack([done[n] for n in file_names])


def load_img(file_name, target_height=320, target_width=576, device="cuda"):
    """-> (3, target_height, target_width) fp32 in [-1, 1]: centre crop to the target ratio, PIL's LANCZOS resize, ToTensor, x * 2 - 1 -- the crop,
    the resize and the normalisation in vk_lanczos_resize_u8, every value bitwise the reference's."""
    return load_img_seq([file_name], target_height, target_width, device)[0]


# ---- frames out (sample_utils.py:96-137) --------------------------------------------------------------------------------------------------
def _to_u8(samples, real, grid=False):
    """(n, 3, H, W) fp32 -> uint8 numpy, HWC: the one place perform_save_locally converts (tests stub it with the numpy expression)."""
    return ops.frames_to_u8(samples.float(), real=real, grid=grid).cpu().numpy()


def save_video(path_stem, frames_u8, fps=10):
    """(t, H, W, 3) uint8 -> `<stem>.mp4` through imageio where it is importable (the reference's writer); otherwise `<stem>.apng`, an animated
    PNG at 1000 / fps ms per frame (lossless, so the frames read back exactly). With VISTA_VIDEO=mjpeg (video_format): `<stem>.avi`, Motion-JPEG;
    the frames may then be a uint8 GPU tensor, which is encoded where it lies, or numpy, which is uploaded. With VISTA_PNG=hip (png_format) the
    `.apng` is written by png.write_apng, its streams coded on the GPU, from a GPU tensor or numpy alike. Returns the path written."""
    fmt, quality = video_format()
    if fmt == "mjpeg":
        from . import video
        H, W = int(frames_u8.shape[1]), int(frames_u8.shape[2])
        return video.write_avi(path_stem + ".avi", video.encode_jpeg(frames_u8, quality), W, H, fps)
    try:
        import imageio
    except ImportError:
        imageio = None
    if imageio is None and png_format() == "hip":
        from . import png
        return png.write_apng(path_stem + ".apng", frames_u8, fps)
    if torch.is_tensor(frames_u8):
        frames_u8 = frames_u8.cpu().numpy()
    if imageio is not None:
        path = path_stem + ".mp4"
        writer = imageio.get_writer(path, fps=fps)
        for frame in frames_u8:
            writer.append_data(frame)
        writer.close()
        return path
    from PIL import Image
    path = path_stem + ".apng"
    images = [Image.fromarray(f) for f in frames_u8]
    # (Pillow folds a frame that equals its predecessor under the same disposal into the predecessor's duration -- a still video would come back
    # as one frame. Alternating the disposal between "leave" and "clear" keeps every frame a frame of its own, 1000 / fps ms each.)
    images[0].save(path, format="PNG", save_all=True, append_images=images[1:], duration=int(round(1000 / fps)), loop=0,
                   disposal=[i & 1 for i in range(len(images))], blend=0)
    return path


def read_video_frames(path):
    """The frames of an `.apng` or an `.avi` (Motion-JPEG, every chunk decoded by Pillow) written by save_video -> (t, H, W, 3) uint8."""
    import numpy as np
    from PIL import Image, ImageSequence
    if path.lower().endswith(".avi"):
        import io
        from . import video
        frames = []
        for j in video.read_avi(path):
            with Image.open(io.BytesIO(j)) as im:
                frames.append(np.array(im.convert("RGB"), dtype=np.uint8))
        return np.stack(frames)
    with Image.open(path) as im:
        return np.stack([np.array(frame.convert("RGB"), dtype=np.uint8) for frame in ImageSequence.Iterator(im)])


def perform_save_locally(save_path, samples, mode, dataset_name, sample_index):
    """Writes `samples` (n, 3, H, W) under save_path/mode with the reference's file names: images `<dataset>_<index:06>_<frame:04>.png`, grids
    `<dataset>_<index:06>.png`, videos `<dataset>_<index:06>.mp4` at 10 fps. A save_path containing "real" holds inputs in [-1, 1], any other
    samples in [0, 1]. The 8-bit conversion (and the make_grid layout) runs in vk_frames_to_u8. Deviation: without imageio the video is an
    animated PNG (`.apng`, 100 ms per frame) instead of an mp4; with VISTA_VIDEO=mjpeg it is `<stem>.avi` (README "Videos"), and the 8-bit frames
    go from vk_frames_to_u8 to the JPEG kernels without leaving the GPU. With VISTA_PNG=hip (README "Pictures") the images, the grid and the
    animated PNG are coded on the GPU (png.encode_png / png.write_apng) under the same file names: the 8-bit frames never make the host round trip."""
    from PIL import Image
    if mode not in ("images", "grids", "videos"):
        raise AssertionError(mode)
    merged_path = os.path.join(save_path, mode)
    os.makedirs(merged_path, exist_ok=True)
    real = "real" in save_path
    stem = os.path.join(merged_path, f"{dataset_name}_{sample_index:06}")
    if png_format() == "hip" and mode != "videos":
        from . import png
        names = [f"{stem}_{count:04}.png" for count in range(samples.shape[0])] if mode == "images" else [stem + ".png"]
        for name, data in zip(names, png.encode_png(ops.frames_to_u8(samples.float(), real=real, grid=mode == "grids"))):
            with open(name, "wb") as f:
                f.write(data)
    elif mode == "images":
        for count, frame in enumerate(_to_u8(samples, real)):
            Image.fromarray(frame).save(f"{stem}_{count:04}.png")
    elif mode == "grids":
        Image.fromarray(_to_u8(samples, real, grid=True)).save(stem + ".png")
    elif video_format()[0] == "mjpeg" or png_format() == "hip":
        save_video(stem, ops.frames_to_u8(samples.float(), real=real), 10)
    else:
        save_video(stem, _to_u8(samples, real), 10)
