"""`python -m vista_amd.sample`: pictures in, frames out -- the reference's sample.py on the MI355X.

Every flag of the reference (sample.py:29-119) under its name with its default; on top: --config / --ckpt (one config, one checkpoint),
--data_root / --anno_file (where the dataset lives) and --eager. On one GPU the sampler replays the UNet of a step from a captured hipGraph, the
two guidance halves concurrently (sampler.graph = sampler.cfg_streams = True: the form bench.py measures, bitwise the eager result); --eager
launches every kernel of every step from the host instead.

    python -m vista_amd.sample --ckpt ckpts/vista.safetensors --dataset IMG --data_root image_folder --save outputs

Several GPUs: start one process per GPU with `python -m torch.distributed.run --nproc-per-node=N -m vista_amd.sample ...` (same flags). With
WORLD_SIZE > 1 in the environment `main` runs as one rank of the job: the denoising steps are frame-sharded over the ranks
(vista_amd/parallel.py; VISTA_SHARD = hybrid | frames, VISTA_DIST_BACKEND = nccl | gloo), everything around them is replicated, and
rank 0 writes the files.

`run(...)` is the loop body as a function (returns the tensors instead of writing files), `main(argv)` the loop of sample.py:204-274.
"""
import argparse
import os
import sys
import time

import torch

from . import frontdoor
from . import sample_utils as SU
from .frontdoor import seed_everything   # noqa: F401  (where the reference's users, and the other front doors, look for it)

UC_KEYS = ["cond_frames", "cond_frames_without_noise", "command", "trajectory", "speed", "angle", "goal"]


def parse_args(**parser_kwargs):
    parser = argparse.ArgumentParser(**parser_kwargs)
    add = parser.add_argument
    add("--version", type=str, default="vwm", help="model version")
    add("--dataset", type=str, default="NUSCENES", help="dataset name")
    add("--save", type=str, default="outputs", help="directory to save samples")
    add("--action", type=str, default="free", help="action mode for control, such as traj, cmd, steer, goal")
    add("--n_rounds", type=int, default=1, help="number of sampling rounds")
    add("--n_frames", type=int, default=25, help="number of frames for each round")
    add("--n_conds", type=int, default=1, help="number of initial condition frames for the first round")
    add("--seed", type=int, default=23, help="random seed for seed_everything")
    add("--height", type=int, default=576, help="target height of the generated video")
    add("--width", type=int, default=1024, help="target width of the generated video")
    add("--cfg_scale", type=float, default=2.5, help="scale of the classifier-free guidance")
    add("--cond_aug", type=float, default=0.0, help="strength of the noise augmentation")
    add("--n_steps", type=int, default=50, help="number of sampling steps")
    add("--rand_gen", action="store_false", help="whether to generate samples randomly or sequentially")
    add("--low_vram", action="store_true", help="accepted for compatibility; a no-op here (every stage stays resident in HBM)")
    # not in the reference
    add("--config", type=str, default=None, help="model config (default: the shipped configs/inference/vista_mi355x.yaml)")
    add("--ckpt", type=str, default=None, help="checkpoint (default: ckpts/vista.safetensors)")
    add("--data_root", type=str, default=None, help="dataset root (default: the reference's, data/nuscenes or image_folder)")
    add("--anno_file", type=str, default=None, help="annotation JSON of the NUSCENES dataset (default: annos/nuScenes_val.json)")
    add("--eager", action="store_true", help="launch every step's kernels from the host instead of replaying captured graphs")
    return parser


class _StageClock:
    """Adds the wall time of the pipeline's condition / encode / decode calls to `timings` while it is active (a device sync on either side of
    each call: a handful per run)."""
    STAGES = (("condition_fn", "condition"), ("encode_first_stage", "encode"), ("decode_first_stage", "decode"))

    def __init__(self, model, timings):
        self.model, self.timings = model, timings

    def _wrap(self, fn, stage):
        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            self.timings[stage] = self.timings.get(stage, 0.0) + time.perf_counter() - t0
            return out
        return timed

    def __enter__(self):
        self.saved = {}
        for attr, stage in self.STAGES:
            self.saved[attr] = self.model.__dict__.get(attr)
            setattr(self.model, attr, self._wrap(getattr(self.model, attr), stage))

    def __exit__(self, *exc):
        for attr, old in self.saved.items():
            if old is None:
                delattr(self.model, attr)
            else:
                setattr(self.model, attr, old)
        return False


def run(model, frame_list, action_dict=None, *, height=576, width=1024, n_frames=25, n_rounds=1, n_conds=1, n_steps=50, cfg_scale=2.5,
        cond_aug=0.0, eager=False, timings=None, shard=None, sampler=None):
    """One sample of the reference's loop (sample.py:222-254) without the files -> (samples in [0, 1], samples_z, inputs in [-1, 1]): load and
    resize the frames, build the value dict, pick the guider (TrianglePredictionGuider for a rollout, VanillaCFG for one round), do_sample.
    The caller seeds. `timings` (a dict) receives the wall time in seconds of load, condition, encode, decode and sample (= the rest of do_sample:
    the denoising loops).
    `shard` (a vista_amd.parallel.FrameShard, one per rank, every rank calling with the same arguments and the same seed): the denoising steps
    run frame-sharded over the shard's ranks, eagerly on one stream whatever `eager` says (a captured graph cannot hold the collectives: DESIGN
    section 6). Conditioner, encoder, decoder and the noise are replicated: every rank returns the same tensors.
    `sampler`: "EulerEDMSampler" | "DPMPP2MSampler"; None = the environment hook VISTA_SAMPLER, unset = EulerEDMSampler (SU.sampler_name)."""
    t0 = time.perf_counter()
    images = SU.load_img_seq(frame_list, height, width, "cuda")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    value_dict = frontdoor.first_window_values(model, images, cond_aug, action_dict)
    sampler = SU.init_sampling(sampler=SU.sampler_name(sampler), guider="TrianglePredictionGuider" if n_rounds > 1 else "VanillaCFG", steps=n_steps,
                               cfg_scale=cfg_scale, num_frames=n_frames)
    sampler.graph = sampler.cfg_streams = not eager and shard is None   # (graph replay: one GPU, no frame shard)
    if shard is not None:
        sampler.shard = shard
    import contextlib
    stages = {}
    with (_StageClock(model, stages) if timings is not None else contextlib.nullcontext()):
        out = SU.do_sample(images, model, sampler, value_dict, num_rounds=n_rounds, num_frames=n_frames, force_uc_zero_embeddings=UC_KEYS,
                           initial_cond_indices=list(range(n_conds)))
        torch.cuda.synchronize()
    if timings is not None:
        timings["load"] = t1 - t0
        timings.update(stages)
        timings["sample"] = time.perf_counter() - t1 - sum(stages.values())
    return out


def init_distributed(n_frames):
    """This process as one rank of a torch.distributed.run job (WORLD_SIZE > 1): picks the GPU (VISTA_FORCE_DEVICE, else LOCAL_RANK), joins the
    process group (VISTA_DIST_BACKEND, default "nccl" = RCCL), builds this rank's FrameShard (VISTA_SHARD = "hybrid" (default) | "frames") and
    runs its plumbing check -- every collective signature of a sharded step on tiny tensors -- before any model is built.
    -> (global rank, shard). The caller owns the process group (destroy_process_group)."""
    import torch.distributed as dist
    from .parallel import DistComm, make_shard
    world = int(os.environ["WORLD_SIZE"])
    mode = os.environ.get("VISTA_SHARD") or "hybrid"
    if mode not in ("hybrid", "frames"):
        raise ValueError(f"VISTA_SHARD must be 'hybrid' or 'frames', not {mode!r}")
    group_size = world // 2 if (mode == "hybrid" and world % 2 == 0) else world
    if group_size > n_frames:
        raise ValueError(f"WORLD_SIZE {world} (VISTA_SHARD={mode}) puts {group_size} ranks into one frame-shard group, but --n_frames is "
                         f"{n_frames}: a rank needs at least one frame")
    rank, world, dev = frontdoor.join_process_group()
    try:
        def make_group(ranks):   # collective: every rank creates every group, members get a communicator
            g = dist.new_group(ranks=ranks)
            return DistComm(g) if rank in ranks else None
        shard = make_shard(n_frames, world, rank, mode=mode, make_group=make_group)
        try:
            shard.selfcheck(torch.device("cuda", dev))
        except Exception as e:  # noqa: BLE001
            raise RuntimeError(f"[rank {rank}/{world}] multi-GPU plumbing check failed (VISTA_SHARD={mode}, backend "
                               f"{dist.get_backend()}, device cuda:{dev}): {e}") from e
    except BaseException:
        dist.destroy_process_group()
        raise
    return rank, shard


def main(argv=None):
    opt, _unknown = parse_args(prog="python -m vista_amd.sample").parse_known_args(argv)
    # sizes the kernels cannot take are refused here, before 2.5 billion parameters are built
    SU.check_sizes(opt.height, opt.width, opt.n_frames, opt.n_rounds, opt.n_conds, frontdoor.net_params(opt))
    SU.sampler_name()   # (a bad VISTA_SAMPLER is refused by name, here)
    SU.video_format()   # (and a bad VISTA_VIDEO or VISTA_VIDEO_QUALITY)
    SU.png_format()     # (and a bad VISTA_PNG)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:   # one rank of a torch.distributed.run job
        rank, shard = init_distributed(opt.n_frames)
        try:
            return _sample_loop(opt, shard, rank)
        finally:
            import torch.distributed as dist
            dist.destroy_process_group()
    return _sample_loop(opt, None, 0)


def _sample_loop(opt, shard, rank):
    """The loop of sample.py:204-274. Every rank of a job walks the same sample indices (the walk is a function of the seed); rank 0 writes."""
    model = frontdoor.build_model(opt, rank)
    for frame_list, sample_index, _dataset_length, action_dict in frontdoor.walk(opt):
        timings = {}
        samples, samples_z, inputs = run(model, frame_list, action_dict, height=opt.height, width=opt.width, n_frames=opt.n_frames,
                                         n_rounds=opt.n_rounds, n_conds=opt.n_conds, n_steps=opt.n_steps, cfg_scale=opt.cfg_scale,
                                         cond_aug=opt.cond_aug, eager=opt.eager, timings=timings, shard=shard)
        if rank == 0:
            t0 = time.perf_counter()
            frontdoor.save_pictures(opt.save, opt.dataset, sample_index, virtual=samples, real=inputs)
            timings["save"] = time.perf_counter() - t0
            print(f"sample {sample_index}: " + frontdoor.timings_text(timings), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
