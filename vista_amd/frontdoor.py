"""What the command-line front doors share: the walk over a dataset, model construction and the start-up refusals, the records files, the
first window's value dict and the picture tree. vista_amd.sample, reward, evaluate, drive, plan, denoise_loss and step_sweep keep what is their
own: flags, refusals, `run`, record contents, summary arithmetic and the scene line.

The walk's order of draws decides which scenes a --rand_gen run visits and what every scene's noise is: seed, scene lookup, the body's draws
(the cond_aug noise first), then the walk's own randint. It is written down once, in `walk`.
"""
import json
import math
import os
import random

import torch

from . import config
from . import sample_utils as SU


def seed_everything(seed):
    """What pytorch_lightning.seed_everything seeds: Python's, numpy's and torch's generators (CPU and every GPU)."""
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------------
def walk(opt, get_scene=None, n_scenes=0):
    """The reference's walk over a dataset (sample.py:204-274) as a generator -> (frame_list, sample_index, dataset_length, action) per scene.
    Before every scene: seed_everything(opt.seed), then get_scene(index, opt.dataset, opt.n_frames, opt.action, data_root=, anno_file=)
    (default: SU.get_sample, looked up at call time). After the caller's body: stop once `n_scenes` scenes were yielded (0 = no stop), else
    advance by a random step of 1 .. dataset_length - 1 (the random walk, which never ends by itself) or by one to the dataset's end.
    Every rank of a job walks the same indices: the walk is a function of the seed."""
    sample_index, yielded = 0, 0
    while sample_index >= 0:
        seed_everything(opt.seed)
        frame_list, sample_index, dataset_length, action = (get_scene or SU.get_sample)(
            sample_index, opt.dataset, opt.n_frames, opt.action, data_root=opt.data_root, anno_file=opt.anno_file)
        yield frame_list, sample_index, dataset_length, action
        yielded += 1
        if n_scenes and yielded >= n_scenes:
            return
        if opt.rand_gen:
            sample_index += random.randint(1, max(1, dataset_length - 1))
        else:
            sample_index += 1
            if dataset_length <= sample_index:
                sample_index = -1


# ---- model and start-up ---------------------------------------------------------------------------------------------------------------------------
def net_params(opt):
    """network_config.params of --config, for SU.check_sizes; None = the shipped configuration."""
    return config.load_config(opt.config)["model"]["params"]["network_config"]["params"] if opt.config else None


def build_model(opt, rank=0):
    """The model of --version with the --config / --ckpt overrides (SU.init_model, looked up at call time)."""
    if opt.low_vram and rank == 0:
        print("--low_vram: accepted, no effect (every stage stays resident in HBM)")
    spec = dict(SU.VERSION2SPECS[opt.version])
    if opt.config:
        spec["config"] = opt.config
    if opt.ckpt:
        spec["ckpt"] = opt.ckpt
    return SU.init_model(spec)


def check_world(module, not_built):
    """Refuses WORLD_SIZE > 1 for a front door that runs on one GPU; `not_built` names the multi-GPU form it lacks."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError(f"WORLD_SIZE {os.environ['WORLD_SIZE']}: vista_amd.{module} runs on one GPU ({not_built}); start it without "
                         "torch.distributed.run")


def check_scene_count(opt):
    if opt.n_scenes < 0:
        raise ValueError(f"--n_scenes {opt.n_scenes}: a count of scenes, or 0 for the whole dataset")
    if opt.n_scenes == 0 and opt.rand_gen:
        raise ValueError("--n_scenes 0 (to the end of the dataset) with the random walk: the reference's random walk never ends by itself; "
                         "give --n_scenes N, or --rand_gen for the sequential walk")


def n_rounds_given(parse_args, argv):
    """Whether the command line names --n_rounds (under any abbreviation argparse accepts), and its value."""
    parser = parse_args()
    parser.set_defaults(n_rounds=None)
    return parser.parse_known_args(argv)[0].n_rounds


def join_process_group():
    """This process as one rank of a torch.distributed.run job: picks the GPU (VISTA_FORCE_DEVICE, else LOCAL_RANK) and joins the process group
    (VISTA_DIST_BACKEND, default "nccl" = RCCL) -> (global rank, world, device index). The caller owns the group (destroy_process_group)."""
    import torch.distributed as dist
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ.get("RANK", "0"))
    backend = os.environ.get("VISTA_DIST_BACKEND", "nccl")
    dev = int(os.environ.get("VISTA_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev))   # "nccl" is RCCL on ROCm
    else:
        dist.init_process_group(backend)
    return rank, world, dev


# ---- records --------------------------------------------------------------------------------------------------------------------------------------
def start_records(save_dir, name):
    """An empty <save_dir>/<name>: the file describes one run, as the summary does. Returns its path."""
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, name)
    open(path, "w").close()
    return path


def append_record(save_dir, name, record):
    """One line per scene at the end of <save_dir>/<name>, strict JSON (a non-finite number is a ValueError, nothing is written). Returns the
    file's path."""
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, name)
    line = json.dumps(record, allow_nan=False)
    with open(path, "a") as f:
        f.write(line + "\n")
    return path


def write_summary(save_dir, name, summary):
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, name)
    with open(path, "w") as f:
        json.dump(summary, f, allow_nan=False, indent=1)
        f.write("\n")
    return path


def json_number(v):
    """A float for strict JSON: None where it is not finite (an infinite PSNR, a mean over nothing)."""
    v = float(v)
    return v if math.isfinite(v) else None


def mean(values):
    """The mean of a list of floats in float64 (fsum: exact sum, one rounding); nan for an empty list."""
    return math.fsum(values) / len(values) if values else float("nan")


def rounded_timings(timings):
    return {k: round(float(v), 4) for k, v in (timings or {}).items()}


def timings_text(timings):
    return ", ".join(f"{k} {v:.2f} s" for k, v in timings.items())


# ---- the first window -----------------------------------------------------------------------------------------------------------------------------
def first_window_values(model, images, cond_aug, action_dict=None):
    """The value dict of a scene's first window (sample.py:226-236): the embedders' options, the conditioning frame with and without its
    augmentation noise -- ONE torch.randn_like draw -- and the action's entries."""
    value_dict = SU.init_embedder_options(set(e.input_key for e in model.conditioner.embedders))
    cond_img = images[:1]
    value_dict["cond_frames_without_noise"] = cond_img
    value_dict["cond_aug"] = cond_aug
    value_dict["cond_frames"] = cond_img + cond_aug * torch.randn_like(cond_img)
    value_dict.update(action_dict or {})
    return value_dict


def save_pictures(save_dir, dataset, index, virtual=None, real=None):
    """<save_dir>/{virtual,real}/{videos,grids,images} under perform_save_locally's names, for the stacks given."""
    for side, frames in (("virtual", virtual), ("real", real)):
        if frames is None:
            continue
        for mode in ("videos", "grids", "images"):
            SU.perform_save_locally(os.path.join(save_dir, side), frames, mode, dataset, index)
