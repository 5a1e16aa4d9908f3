"""`python -m vista_amd.reward`: pictures and candidate actions in, rewards out -- the reference's reward.py on the MI355X.

Every flag of the reference (reward.py:29-119) under its name with its default (note --n_steps 10, --ens_size 5, --action traj); on top, as in
vista_amd.sample: --config / --ckpt, --data_root / --anno_file, --eager; and --save_maps / --heat_max for the disagreement overlays. The
reference computes the reward and drops it; here every scene appends one JSON line to <save>/rewards.jsonl and prints the same numbers:

    python -m vista_amd.reward --ckpt ckpts/vista.safetensors --action traj,cmd,free --save outputs --save_maps

--action takes a comma-separated list: the scene is scored under every candidate with the SAME ensemble noise (common random numbers), so
the rewards of two actions differ by the actions, not by the draws. A candidate the scene's annotation cannot supply (no CAN bus record for
`steer`, a goal point outside the frame) is reported with "reward": null and the reason; the run goes on.

Several GPUs: `python -m torch.distributed.run --nproc-per-node=N -m vista_amd.reward ...` (same flags, N <= --ens_size). With WORLD_SIZE > 1
`main` runs as one rank: ensemble member e is sampled by rank e % N, whole, on that rank's GPU (no frame shard: graph replay stays on), one
all_reduce per candidate completes the ensemble on every rank, and rank 0 writes.

`run(...)` is the loop body as a function (returns the reports instead of writing files), `main(argv)` the loop of reward.py:212-266.
"""
import contextlib
import os
import sys
import time

import torch

from . import frontdoor, ops, reward_utils
from . import sample_utils as SU
from .sample import UC_KEYS, _StageClock, seed_everything   # noqa: F401  (seed_everything: for the callers of run)

ACTION_MODES = ("free", "traj", "trajectory", "cmd", "command", "steer", "goal")
HEAT_CELL = 8       # the first stage maps 8 x 8 pixels to one latent pixel
HEAT_ALPHA = 0.6
RECORDS_NAME = "rewards.jsonl"
_WHY_EMPTY = {"steer": "the scene's annotation has no speed / angle record", "goal": "the scene's goal point does not project into the camera frame"}


def parse_args(**parser_kwargs):
    import argparse
    parser = argparse.ArgumentParser(**parser_kwargs)
    add = parser.add_argument
    add("--version", type=str, default="vwm", help="model version")
    add("--dataset", type=str, default="NUSCENES", help="dataset name")
    add("--save", type=str, default="outputs", help="directory to save samples")
    add("--action", type=str, default="traj", help="action mode for control, such as traj, cmd, steer, goal; a comma-separated list scores "
        "the scene under every one of them (free = no action)")
    add("--n_frames", type=int, default=25, help="number of frames for each round")
    add("--n_conds", type=int, default=1, help="number of initial condition frames for the first round")
    add("--ens_size", type=int, default=5, help="number of samples per case")
    add("--seed", type=int, default=23, help="random seed for seed_everything")
    add("--height", type=int, default=576, help="target height of the generated video")
    add("--width", type=int, default=1024, help="target width of the generated video")
    add("--cfg_scale", type=float, default=2.5, help="scale of the classifier-free guidance")
    add("--cond_aug", type=float, default=0.0, help="strength of the noise augmentation")
    add("--n_steps", type=int, default=10, help="number of sampling steps")
    add("--rand_gen", action="store_false", help="whether to generate samples randomly or sequentially")
    add("--low_vram", action="store_true", help="accepted for compatibility; a no-op here (every stage stays resident in HBM)")
    # not in the reference
    add("--config", type=str, default=None, help="model config (default: the shipped configs/inference/vista_mi355x.yaml)")
    add("--ckpt", type=str, default=None, help="checkpoint (default: ckpts/vista.safetensors)")
    add("--data_root", type=str, default=None, help="dataset root (default: the reference's, data/nuscenes or image_folder)")
    add("--anno_file", type=str, default=None, help="annotation JSON of the NUSCENES dataset (default: annos/nuScenes_val.json)")
    add("--eager", action="store_true", help="launch every step's kernels from the host instead of replaying captured graphs")
    add("--save_maps", action="store_true", help="write the input frames with every candidate's disagreement map laid over them (heat/<action>/videos)")
    add("--heat_max", type=float, default=None, help="map value drawn at full heat (default: the maximum of the scene's maps)")
    return parser


def parse_actions(text):
    """"traj,cmd,free" -> ["traj", "cmd", "free"]: the candidate actions of --action, in the order given, each one once."""
    names = [n.strip() for n in str(text).split(",")]
    if not names or any(not n for n in names):
        raise ValueError(f"--action {text!r}: expected an action mode or a comma-separated list of them ({', '.join(ACTION_MODES)})")
    for n in names:
        if n not in ACTION_MODES:
            raise ValueError(f"Unsupported action mode {n} (--action takes {', '.join(ACTION_MODES)})")
    if len(set(names)) != len(names):
        raise ValueError(f"--action {text!r}: every candidate once")
    return names


def scene_candidates(selected_index, dataset, n_frames, names, data_root=None, anno_file=None):
    """The scene at `selected_index` under every candidate action -> (frame_list, index, dataset_length, [(name, action_dict, reason)]).
    Each name is resolved through SU.get_sample; `free` is the empty action dict. A dataset without annotations (IMG) has no actions: every
    candidate runs action-free, as the reference runs it. action_dict None + a reason = the scene's annotation cannot supply this action."""
    frame_list = index = total = None
    out = []
    for name in names:
        frame_list, index, total, action = SU.get_sample(selected_index, dataset, n_frames, name, data_root=data_root, anno_file=anno_file)
        if name == "free" or action is None:
            out.append((name, {}, None))
        elif not action:
            out.append((name, None, _WHY_EMPTY.get(name, "the scene's annotation does not supply this action")))
        else:
            out.append((name, action, None))
    return frame_list, index, total, out


def run(model, frame_list, action_dicts, *, height=576, width=1024, n_frames=25, n_conds=1, n_steps=10, cfg_scale=2.5, cond_aug=0.0,
        ens_size=5, eager=False, want_map=False, members=None, comm=None, timings=None, inputs_out=None, sampler=None):
    """One scene of the reference's loop (reward.py:214-250) under every candidate of `action_dicts` (a list of action dicts; {} or None = no
    action) -> [RewardReport], one per candidate. Mirrors sample.run: load and resize the frames, one value dict per candidate (the
    conditioning frame and its augmentation noise are shared), VanillaCFG, reward_utils.estimate. The sampler replays the UNet of a step from a
    captured hipGraph, the guidance halves concurrently, unless `eager`: the graphs captured for the first member are the ones every later
    member and candidate replays. The caller seeds. `members` / `comm`: see reward_utils.estimate. `timings` (a dict) receives the wall time
    in seconds of load, condition, encode and sample (= the rest: ens_size x n_steps denoising steps per candidate and the statistics).
    `inputs_out` (a list) receives the loaded frames, (n_frames, 3, height, width) in [-1, 1]. `sampler`: as in sample.run (None = VISTA_SAMPLER)."""
    t0 = time.perf_counter()
    images = SU.load_img_seq(frame_list, height, width, "cuda")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    base = frontdoor.first_window_values(model, images, cond_aug)
    value_dicts = []
    for action in action_dicts:
        value_dict = dict(base)
        value_dict.update(action or {})
        value_dicts.append(value_dict)
    sampler = SU.init_sampling(sampler=SU.sampler_name(sampler), guider="VanillaCFG", steps=n_steps, cfg_scale=cfg_scale, num_frames=n_frames)
    sampler.graph = sampler.cfg_streams = not eager
    stages = {}
    with (_StageClock(model, stages) if timings is not None else contextlib.nullcontext()):
        reports = reward_utils.estimate(images, model, sampler, value_dicts, num_frames=n_frames, ensemble_size=ens_size,
                                        force_uc_zero_embeddings=UC_KEYS, initial_cond_indices=list(range(n_conds)), want_map=want_map,
                                        members=members, comm=comm)
        torch.cuda.synchronize()
    if timings is not None:
        timings["load"] = t1 - t0
        timings.update(stages)
        timings["sample"] = time.perf_counter() - t1 - sum(stages.values())
    if inputs_out is not None:
        inputs_out.append(images)
    return reports


def make_record(index, frame_list, seed, ens_size, n_steps, candidates, reports, timings):
    """The JSON record of one scene. `candidates` as scene_candidates returns them; `reports` holds one RewardReport per candidate that ran (in
    order), a candidate without an action dict gets "reward": null and its reason."""
    reports = iter(reports)
    actions = []
    for name, action, reason in candidates:
        if action is None:
            actions.append({"action": name, "reward": None, "reason": reason})
            continue
        rep = next(reports)
        actions.append({"action": name, "reward": float(rep.reward), "mean_variance": float(rep.mean_variance),
                        "frame_variance": [float(v) for v in rep.frame_variance]})
    return {"index": int(index), "frames": [frame_list[0]], "seed": int(seed), "ens_size": int(ens_size), "n_steps": int(n_steps),
            "actions": actions, "timings": frontdoor.rounded_timings(timings)}


def save_heat_videos(save_dir, inputs, candidates, reports, dataset, sample_index, heat_max=None):
    """<save_dir>/heat/<action>/videos/<dataset>_<index:06>: the input frames under every candidate's map (vk_heat_overlay_u8, 8 x 8 pixels per
    latent pixel). One colour scale per scene: `heat_max`, or the maximum over the scene's maps. Returns the paths written."""
    ran = [name for name, action, _ in candidates if action is not None]
    maps = [rep.map for rep in reports]
    if any(m is None for m in maps):
        raise ValueError("save_heat_videos: the reports carry no maps (run(..., want_map=True))")
    vmax = float(heat_max) if heat_max is not None else max((float(m.max()) for m in maps), default=0.0)
    if not vmax > 0.0:
        vmax = 1.0   # (members that agree everywhere: nothing to draw, any scale will do)
    paths = []
    for name, fmap in zip(ran, maps):
        if tuple(inputs.shape[-2:]) != (HEAT_CELL * fmap.shape[-2], HEAT_CELL * fmap.shape[-1]):
            raise ValueError(f"save_heat_videos: a {tuple(fmap.shape[-2:])} map does not belong to {tuple(inputs.shape[-2:])} frames")
        frames = ops.heat_overlay_u8(inputs.float(), fmap, vmax, alpha=HEAT_ALPHA)   # (stays on the GPU: save_video moves it only for the PNG path)
        folder = os.path.join(save_dir, "heat", name, "videos")
        os.makedirs(folder, exist_ok=True)
        paths.append(SU.save_video(os.path.join(folder, f"{dataset}_{sample_index:06}"), frames, 10))
    return paths


def init_distributed(ens_size):
    """This process as one rank of a torch.distributed.run job (WORLD_SIZE > 1): picks the GPU the way sample.init_distributed does
    (VISTA_FORCE_DEVICE, else LOCAL_RANK) and joins the process group (VISTA_DIST_BACKEND, default "nccl" = RCCL). No FrameShard: a member runs
    whole on its rank. -> (global rank, world, communicator). The caller owns the process group (destroy_process_group)."""
    import torch.distributed as dist
    from .parallel import DistComm
    reward_utils.member_slots(ens_size, int(os.environ["WORLD_SIZE"]))   # refuses world > ens_size by name, before anything is joined
    rank, world, _dev = frontdoor.join_process_group()
    try:
        comm = DistComm(None, name="ensemble")
    except BaseException:
        dist.destroy_process_group()
        raise
    return rank, world, comm


def main(argv=None):
    opt, _unknown = parse_args(prog="python -m vista_amd.reward").parse_known_args(argv)
    # what cannot run is refused here, before 2.5 billion parameters are built
    SU.check_sizes(opt.height, opt.width, opt.n_frames, 1, opt.n_conds, frontdoor.net_params(opt))
    SU.sampler_name()   # (a bad VISTA_SAMPLER is refused by name, here)
    SU.video_format()   # (and a bad VISTA_VIDEO or VISTA_VIDEO_QUALITY)
    SU.png_format()     # (and a bad VISTA_PNG)
    if opt.ens_size < 2:
        raise ValueError(f"--ens_size {opt.ens_size}: reward estimation needs at least two ensemble members (unbiased variance)")
    if opt.heat_max is not None and not opt.heat_max > 0.0:
        raise ValueError(f"--heat_max {opt.heat_max}: must be positive")
    names = parse_actions(opt.action)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:   # one rank of a torch.distributed.run job
        rank, world, comm = init_distributed(opt.ens_size)
        try:
            return _reward_loop(opt, names, rank, (rank, world), comm)
        finally:
            import torch.distributed as dist
            dist.destroy_process_group()
    return _reward_loop(opt, names, 0, None, None)


def _reward_loop(opt, names, rank, members, comm):
    """The loop of reward.py:212-266. Every rank of a job walks the same sample indices (the walk is a function of the seed); rank 0 writes."""
    model = frontdoor.build_model(opt, rank)

    def get_scene(index, dataset, n_frames, _action, **where):   # (the candidates of --action in place of its one action)
        return scene_candidates(index, dataset, n_frames, names, **where)
    for frame_list, sample_index, _dataset_length, candidates in frontdoor.walk(opt, get_scene):
        timings, inputs = {}, []
        action_dicts = [action for _, action, _ in candidates if action is not None]
        reports = []
        if action_dicts:
            reports = run(model, frame_list, action_dicts, height=opt.height, width=opt.width, n_frames=opt.n_frames, n_conds=opt.n_conds,
                          n_steps=opt.n_steps, cfg_scale=opt.cfg_scale, cond_aug=opt.cond_aug, ens_size=opt.ens_size, eager=opt.eager,
                          want_map=opt.save_maps, members=members, comm=comm, timings=timings, inputs_out=inputs)
        if rank == 0:
            t0 = time.perf_counter()
            images = inputs[0] if inputs else SU.load_img_seq(frame_list, opt.height, opt.width, "cuda")
            frontdoor.save_pictures(opt.save, opt.dataset, sample_index, real=images)
            if opt.save_maps and reports:
                save_heat_videos(opt.save, images, candidates, reports, opt.dataset, sample_index, opt.heat_max)
            timings["save"] = time.perf_counter() - t0
            record = make_record(sample_index, frame_list, opt.seed, opt.ens_size, opt.n_steps, candidates, reports, timings)
            frontdoor.append_record(opt.save, RECORDS_NAME, record)
            shown = ", ".join(f"{a['action']} " + ("null" if a["reward"] is None else f"{a['reward']:.6f}") for a in record["actions"])
            print(f"reward {sample_index}: {shown} | " + frontdoor.timings_text(timings), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
