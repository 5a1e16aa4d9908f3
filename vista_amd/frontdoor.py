"""What the command-line front doors share: the walk over a dataset, model construction and the start-up refusals, the records files, the
scene-per-rank form of a run that walks scenes (SceneRanks, RankedRun), the first window's value dict and the picture tree. vista_amd.sample,
reward, evaluate, drive, plan, denoise_loss and step_sweep keep what is their own: flags, refusals, `run`, record contents, summary arithmetic
and the scene line.

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


# ---- scene-per-rank -------------------------------------------------------------------------------------------------------------------------------
BARRIER_HOURS = 24   # a rank that is done waits at the barrier for the slowest one: the group's timeout is a run's length, not a collective's


class SceneRanks:
    """This process's place in a scene-per-rank run of evaluate / denoise_loss / step_sweep: the k-th scene the walk yields (k = 0, 1, ...)
    belongs to rank k % world. `rank` and `world` are plain values: SceneRanks(1, 2) is "rank 1 of 2" with no process group -- join() does
    nothing and the barrier returns at once, so the caller runs the ranks one after the other and finishes rank 0 last. Only scene_ranks()
    makes one that is `launched`, from torch.distributed.run's environment, and that one joins a group. world 1 is the single-process run."""

    def __init__(self, rank=0, world=1, launched=False):
        if not 0 <= rank < world:
            raise ValueError(f"SceneRanks: rank {rank} of {world}")
        self.rank, self.world, self.launched, self.joined = int(rank), int(world), bool(launched), False

    @property
    def split(self):
        return self.world > 1

    @property
    def prefix(self):
        """What a rank puts before its scene lines; nothing for a single process."""
        return f"[rank {self.rank}] " if self.split else ""

    def owns(self, k):
        return k % self.world == self.rank

    def join(self):
        """One rank of a torch.distributed.run job: picks the GPU as join_process_group does (VISTA_FORCE_DEVICE, else LOCAL_RANK) and joins
        a gloo group, whatever VISTA_DIST_BACKEND says: the group exists for one barrier before the merge, no tensor on a device ever enters
        it, and RCCL refuses two ranks on one device. A single process joins nothing, nor does a rank that was not launched as one."""
        if not (self.split and self.launched) or self.joined:
            return self
        import datetime
        import torch.distributed as dist
        dev = int(os.environ.get("VISTA_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if torch.cuda.is_available():   # (a front door without a GPU is refused where it builds its model)
            torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=self.rank, world_size=self.world, timeout=datetime.timedelta(hours=BARRIER_HOURS))
        self.joined = True
        return self

    def barrier(self):
        if self.joined:
            import torch.distributed as dist
            dist.barrier()

    def leave(self):
        if self.joined:
            import torch.distributed as dist
            dist.destroy_process_group()
            self.joined = False


def scene_ranks(module, not_built, n_scenes=0):
    """The start-up check of a front door that walks scenes -> its SceneRanks (not joined yet). Without the hook VISTA_SCENE_RANKS this is
    check_world, word for word. With it: WORLD_SIZE unset or 1 is the single-process run; a larger one is rank RANK of WORLD_SIZE, and a
    count of scenes below WORLD_SIZE is refused because a rank would have nothing to do."""
    if not SU.scene_ranks():   # (a bad value is refused by name, here)
        check_world(module, not_built)
        return SceneRanks()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return SceneRanks()
    if 0 < n_scenes < world:
        raise ValueError(f"--n_scenes {n_scenes} with WORLD_SIZE {world} (environment hook VISTA_SCENE_RANKS=1): scene k runs on rank k mod "
                         f"{world}, so ranks {n_scenes} .. {world - 1} would have nothing to do; give --n_scenes {world} or more, or fewer ranks")
    return SceneRanks(int(os.environ.get("RANK", "0")), world, launched=True)


def part_name(name, rank):
    return f"{name}.rank{rank}"


def read_parts(save_dir, name, world, count):
    """The part files <name>.rank<r> of `world` ranks -> the `count` records in walk order. Every line holds {"k": walk position, "record": ...};
    position k must occur exactly once, in the file of rank k % world. Anything else is an error that names the rank and the position."""
    found = {}
    for rank in range(world):
        path = os.path.join(save_dir, part_name(name, rank))
        first = f"position {rank}" if rank < count else "no position"
        if not os.path.isfile(path):
            raise FileNotFoundError(f"scene-per-rank merge: rank {rank} left no part file {path} (it holds {first} onwards): the run is "
                                    "incomplete, nothing is merged")
        with open(path) as f:
            for line in f.read().splitlines():
                entry = json.loads(line)
                k = int(entry["k"])
                if k in found:
                    raise ValueError(f"scene-per-rank merge: rank {rank} holds position {k} a second time in {path}" if found[k][0] == rank else
                                     f"scene-per-rank merge: rank {rank} holds position {k} in {path}, which rank {found[k][0]} holds too")
                if not (0 <= k < count and k % world == rank):
                    raise ValueError(f"scene-per-rank merge: rank {rank} holds position {k} in {path}; of {count} positions its own are "
                                     f"{rank}, {rank + world}, ...")
                found[k] = (rank, entry["record"])
    for k in range(count):
        if k not in found:
            raise ValueError(f"scene-per-rank merge: rank {k % world} holds no record of position {k} in "
                             f"{os.path.join(save_dir, part_name(name, k % world))}: the run is incomplete, nothing is merged")
    return [found[k][1] for k in range(count)]


class RankedRun:
    """The records and the summary of one run of a front door that walks scenes, for a single process and for one rank of several.

    A single process (ranks.world == 1) writes what the front doors always wrote: <records_name> started anew, one line per scene, then
    <summary_name> from summarize(records). One rank of several starts <records_name>.rank<r> anew and appends {"k": position, "record":
    record} per scene of its own; finish() waits at the barrier, and rank 0 then reads every part file, starts <records_name> anew with the
    records in walk order, writes summarize(records) with a last key "ranks", and removes the part files. An incomplete run (read_parts)
    raises before <records_name> is touched: no summary is written and the part files stay.

    extra: what the summary needs beyond the records (evaluate's CLIP embeddings), as an object with save_part(path) -- called by every
    rank before the barrier -- and load_parts(paths, in rank order) -- called by rank 0 after it; its files are <records_name>.<extra_name>.rank<r>."""

    def __init__(self, ranks, save_dir, records_name, summary_name, summarize, extra=None, extra_name="extra"):
        self.ranks, self.save_dir, self.records_name, self.summary_name, self.summarize = ranks, save_dir, records_name, summary_name, summarize
        self.extra, self.extra_name = extra, f"{records_name}.{extra_name}"
        self.records, self.count = [], 0
        self.own_name = part_name(records_name, ranks.rank) if ranks.split else records_name
        start_records(save_dir, self.own_name)

    def own(self, items):
        """(k, item) for the items at this rank's positions; every rank consumes the whole iterable, and counts it."""
        for k, item in enumerate(items):
            self.count = k + 1
            if self.ranks.owns(k):
                yield k, item

    def scenes(self, opt, get_scene=None, n_scenes=0):
        """(k, scene) for this rank's scenes of walk(). Every rank runs the whole walk -- the seeding, the lookup, the advance -- and the
        caller's body for its own scenes only: the ranks visit the single-process walk's scenes as long as no body draws from Python's
        `random` between the walk's seed_everything and its randint (torch's and numpy's generators are free: the walk draws from neither)."""
        return self.own(walk(opt, get_scene, n_scenes))

    def add(self, k, record):
        append_record(self.save_dir, self.own_name, {"k": int(k), "record": record} if self.ranks.split else record)
        self.records.append(record)

    def _extra_paths(self):
        return [os.path.join(self.save_dir, part_name(self.extra_name, r)) for r in range(self.ranks.world)]

    def finish(self):
        ranks = self.ranks
        if not ranks.split:
            write_summary(self.save_dir, self.summary_name, self.summarize(self.records))
            return
        if self.extra is not None:
            self.extra.save_part(self._extra_paths()[ranks.rank])
        ranks.barrier()
        if ranks.rank != 0:
            return
        records = read_parts(self.save_dir, self.records_name, ranks.world, self.count)
        if self.extra is not None:
            self.extra.load_parts(self._extra_paths())
        summary = self.summarize(records)
        summary["ranks"] = ranks.world
        start_records(self.save_dir, self.records_name)
        for record in records:
            append_record(self.save_dir, self.records_name, record)
        write_summary(self.save_dir, self.summary_name, summary)
        for r in range(ranks.world):
            os.remove(os.path.join(self.save_dir, part_name(self.records_name, r)))
        for path in self._extra_paths() if self.extra is not None else []:
            os.remove(path)


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
