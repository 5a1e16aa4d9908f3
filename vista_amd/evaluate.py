"""`python -m vista_amd.evaluate`: sample scenes as `vista_amd.sample` does and score every predicted frame against the real one.

Every flag of `vista_amd.sample` under its name with its default (the parser is built from sample.parse_args); on top: --n_scenes (how many
scenes to score; 0 = to the end of the dataset, for the sequential walk only), --no_pictures (write the metrics files only) and --compare DIR
(score the pictures an earlier run wrote under DIR; no model is built).

    python -m vista_amd.evaluate --ckpt ckpts/vista.safetensors --action traj --rand_gen --n_scenes 50 --save outputs
    python -m vista_amd.evaluate --compare outputs --n_conds 1

Per scene: sample.run with the sampling CLI's seeding, ops.frames_to_u8 on both stacks (the bytes of the saved pictures), PSNR and SSIM from
vk_frame_fidelity_u8 (vista_amd/fidelity.py). A rollout predicts n_rounds * (n_frames - 3) + 3 frames while the sampler loads n_frames: where
the scene's annotation lists more, the additional real frames are loaded here at the same size, and as many frames are scored as have ground
truth. One JSON line per scene goes to <save>/metrics.jsonl, the means over scenes and the horizon curve (mean PSNR / SSIM at each frame index)
to <save>/metrics_summary.json; both files describe this run only. The first --n_conds frames are conditioning frames: listed, and excluded from
every mean. A mean over frames of which one is identical to its ground truth (infinite PSNR) is infinite, and written as null.

Not built: the IMG dataset (one picture repeated has no future to compare against) is refused by name, and so is WORLD_SIZE > 1 without the
hook below. LPIPS and FVD are not built: their weights are in no checkpoint.

Several GPUs: with the environment hook VISTA_SCENE_RANKS=1 under torch.distributed.run the k-th scene of the walk (for --compare: of
picture_pairs) is sampled and scored by rank k mod WORLD_SIZE, every rank appends its records to <save>/metrics.jsonl.rank<r>, and after one
barrier rank 0 writes metrics.jsonl in walk order and the summary, with a last key "ranks" (frontdoor.SceneRanks / RankedRun; README "Evaluate
on several GPUs"). Every line is the single-process run's apart from the timings. Separate processes on one GPU have run; several devices have
not, and no speed-up has been measured. Unset (or 0), nothing here changes.

With the environment hook VISTA_EVAL_CLIP=1 the records also hold CLIP-space scores from the checkpoint's own image tower (vista_amd/perceptual.py;
README "CLIP-space scores"): per scored frame `clip_sim`, `clip_step`, `clip_step_real`, their means over the predicted frames, the scene's
`clip_mmd`, and in the summary the means over scenes, the horizon curves and the run-level `clip_mmd`. --compare then loads the tower alone from
--config / --ckpt. Unset (or 0), nothing here changes.

With the environment hook VISTA_EVAL_MOTION=1 the records also hold motion scores from block-matching optical flow on the same bytes
(vista_amd/motion.py; README "Motion scores"): per scored frame `flow_rms`, `flow_rms_real`, `flow_epe`, `flow_moving`, `warp_err`,
`warp_err_real` (the step from the frame before; entry 0 is null), their means over the predicted frames, a `mean_flow_epe` per round, and in
the summary the means over scenes and the horizon curves of the first three. --compare needs nothing more for it: no model, no checkpoint; pictures
whose sides are not multiples of 32 are refused by name. Unset (or 0), nothing here changes.
"""
import json
import os
import re
import sys
import time

from . import fidelity, frontdoor, motion, perceptual, sample
from .frontdoor import json_number, mean
from ._lib import VistaHipError
from . import sample_utils as SU

PICTURE_NAME = re.compile(r"^(?P<dataset>.+)_(?P<index>\d{6})_(?P<frame>\d{4})\.png$")   # perform_save_locally's image names
RECORDS_NAME, SUMMARY_NAME = "metrics.jsonl", "metrics_summary.json"


def parse_args(**parser_kwargs):
    parser = sample.parse_args(**parser_kwargs)
    add = parser.add_argument
    add("--n_scenes", type=int, default=0, help="number of scenes to score (0: to the end of the dataset; needs the sequential walk, --rand_gen)")
    add("--no_pictures", action="store_true", help="write metrics.jsonl and metrics_summary.json only, no pictures")
    add("--compare", type=str, default=None, metavar="DIR",
        help="score DIR/virtual/images against DIR/real/images (an earlier run's pictures) and write the metrics files into DIR; no model is built")
    return parser


def check_run(opt, net_params=None):
    """Refuses, by name and before any model is built, what an evaluation run cannot do."""
    SU.check_sizes(opt.height, opt.width, opt.n_frames, opt.n_rounds, opt.n_conds, net_params)
    SU.sampler_name()   # (a bad VISTA_SAMPLER is refused by name, here)
    SU.video_format()   # (and a bad VISTA_VIDEO or VISTA_VIDEO_QUALITY)
    SU.png_format()     # (and a bad VISTA_PNG)
    SU.eval_clip()      # (and a bad VISTA_EVAL_CLIP)
    if SU.eval_motion():   # (and a bad VISTA_EVAL_MOTION; check_sizes left multiples of 64 only)
        motion.check_size(opt.height, opt.width, f"--height {opt.height} --width {opt.width} with VISTA_EVAL_MOTION=1")
    if opt.height < fidelity.TAPS or opt.width < fidelity.TAPS:
        raise ValueError(f"--height {opt.height} --width {opt.width}: SSIM takes an {fidelity.TAPS} x {fidelity.TAPS} window")
    if opt.dataset == "IMG":
        raise ValueError("--dataset IMG: one picture repeated has no future frames to score a prediction against; evaluate needs a dataset "
                         "of annotated scenes (NUSCENES)")
    frontdoor.check_scene_count(opt)


def check_world(n_scenes=0):
    """-> this process's frontdoor.SceneRanks: a single process, unless the hook VISTA_SCENE_RANKS=1 allows WORLD_SIZE > 1."""
    return frontdoor.scene_ranks("evaluate", "scene-per-rank evaluation with a merge of the records is not built", n_scenes)


def rollout_length(n_frames, n_rounds):
    return n_rounds * (n_frames - 3) + 3 if n_rounds > 1 else n_frames


def future_frames(index, n_frames, upto, dataset="NUSCENES", data_root=None, anno_file=None):
    """The paths of the scene's real frames n_frames .. upto - 1, as far as its annotation lists them and the files exist."""
    src = SU.DATASET2SOURCES[dataset]
    data_root = src["data_root"] if data_root is None else data_root
    anno_file = src["anno_file"] if anno_file is None else anno_file
    with open(anno_file, "r") as f:
        scenes = json.load(f)
    names = scenes[index % len(scenes)]["frames"][n_frames:upto]
    paths = []
    for name in names:
        path = os.path.join(data_root, name)
        if not os.path.exists(path):
            break
        paths.append(path)
    return paths


# ---- records ------------------------------------------------------------------------------------------------------------------------------
def frame_round(i, n_frames):
    """The sampling round that produced frame i of a rollout: the first window holds n_frames, every later one adds n_frames - 3."""
    return 0 if i < n_frames else 1 + (i - n_frames) // (n_frames - 3)


# record key -> MotionReport attribute, in the order the keys are written
MOTION_KEYS = {"flow_rms": "rms", "flow_rms_real": "rms_real", "flow_epe": "epe", "flow_moving": "moving", "warp_err": "warp_err",
               "warp_err_real": "warp_err_real"}


def make_record(index, frame_list, report, *, seed, action, n_conds, n_rounds, n_frames, timings=None, clip=None, motion=None):
    """The JSON record of one scene from its FidelityReport (one entry per scored frame). clip: the scene's perceptual.PerceptualReport, which
    adds the clip_* keys (a NaN score is null, and so is a mean that holds one); None adds nothing. motion: the scene's motion.MotionReport of
    both stacks, which adds the MOTION_KEYS after them (entry 0, which has no predecessor, is null); None adds nothing."""
    scored = len(report.psnr)
    psnr, ssim = [float(v) for v in report.psnr], [float(v) for v in report.ssim]
    cond = [i for i in range(scored) if i < n_conds]
    pred = [i for i in range(scored) if i >= n_conds]
    rounds = []
    for r in range(max(1, n_rounds)):
        members = [i for i in pred if frame_round(i, n_frames) == r]
        if members:
            rounds.append({"round": r, "frames": len(members), "mean_psnr": json_number(mean([psnr[i] for i in members])),
                           "mean_ssim": json_number(mean([ssim[i] for i in members]))})
    record = {"index": int(index), "frames": [frame_list[0]], "seed": int(seed), "action": str(action), "n_conds": int(n_conds),
              "n_rounds": int(n_rounds), "frames_scored": scored,
              "psnr": [json_number(v) for v in psnr], "ssim": [json_number(v) for v in ssim], "sse": [[int(c) for c in row] for row in report.sse],
              "cond": cond, "mean_psnr": json_number(mean([psnr[i] for i in pred])), "mean_ssim": json_number(mean([ssim[i] for i in pred])),
              "rounds": rounds, "timings": frontdoor.rounded_timings(timings)}
    if clip is None and motion is None:
        return record
    timings_at = record.pop("timings")   # (stays the last key)
    if clip is not None:
        if not len(clip.sim) == len(clip.step) == len(clip.step_real) == scored:
            raise ValueError(f"make_record: the CLIP-space report holds {len(clip.sim)} frames, the fidelity report {scored}")
        scores = {"clip_sim": [float(v) for v in clip.sim], "clip_step": [float(v) for v in clip.step], "clip_step_real": [float(v) for v in clip.step_real]}
        for key, values in scores.items():
            record[key] = [json_number(v) for v in values]
        for key, values in scores.items():   # (a first predicted frame steps from the last conditioning frame)
            record["mean_" + key] = json_number(mean([values[i] for i in pred]))
        record["clip_mmd"] = None if clip.mmd is None else perceptual.mmd_json(clip.mmd)
        for r in rounds:
            members = [i for i in pred if frame_round(i, n_frames) == r["round"]]
            r["mean_clip_sim"] = json_number(mean([float(clip.sim[i]) for i in members]))
    if motion is not None:
        columns = {key: getattr(motion, attr) for key, attr in MOTION_KEYS.items()}
        if any(v is None for v in columns.values()) or not all(len(v) == scored for v in columns.values()):
            held = "no real stack" if motion.epe is None else f"{len(motion.rms)} frames"
            raise ValueError(f"make_record: the motion report holds {held}, the fidelity report {scored} frames of both stacks")
        scores = {key: [float(v) for v in values] for key, values in columns.items()}
        for key, values in scores.items():   # (entry 0 has no predecessor: null)
            record[key] = [json_number(v) for v in values]
        for key, values in scores.items():   # (a first predicted frame steps from the last conditioning frame)
            record["mean_" + key] = json_number(mean([values[i] for i in pred]))
        for r in rounds:
            members = [i for i in pred if frame_round(i, n_frames) == r["round"]]
            r["mean_flow_epe"] = json_number(mean([scores["flow_epe"][i] for i in members]))
    record["timings"] = timings_at
    return record


def summarize(records, clip=None, motion=None):
    """Means over scenes and the horizon curve: at each frame index the mean PSNR and SSIM over the scenes that scored that index as a predicted
    (not a conditioning) frame. null where no scene did, or where a PSNR in the mean is infinite (written as null in the record).
    clip: {"mmd": perceptual.mmd() over all predicted and real frames of the run (or None), "tower": perceptual.tower_info()} for records made
    with clip=; adds the CLIP-space means, horizon curves and the run-level clip_mmd. None adds nothing.
    motion: motion.motion_info() for records made with motion=; adds the means over scenes of the motion scores, the horizon curves of flow_rms,
    flow_rms_real and flow_epe, and the dict itself under "motion". None adds nothing."""
    def scene_mean(key):
        vals = [r[key] for r in records if r["frames_scored"] > len(r["cond"])]
        return None if not vals or any(v is None for v in vals) else json_number(mean(vals))
    length = max((r["frames_scored"] for r in records), default=0)
    horizon = {"frame": list(range(length)), "scenes": [], "psnr": [], "ssim": []}
    for i in range(length):
        has = [r for r in records if i < r["frames_scored"] and i not in r["cond"]]
        horizon["scenes"].append(len(has))
        for key in ("psnr", "ssim"):
            vals = [r[key][i] for r in has]
            horizon[key].append(None if not vals or any(v is None for v in vals) else json_number(mean(vals)))
    summary = {"scenes": len(records), "mean_psnr": scene_mean("mean_psnr"), "mean_ssim": scene_mean("mean_ssim"), "horizon": horizon}

    def curve(key):
        horizon[key] = []
        for i in range(length):
            vals = [r[key][i] for r in records if i < r["frames_scored"] and i not in r["cond"]]
            horizon[key].append(None if not vals or any(v is None for v in vals) else json_number(mean(vals)))
    if clip is not None:
        for key in ("mean_clip_sim", "mean_clip_step", "mean_clip_step_real"):
            summary[key] = scene_mean(key)
        for key in ("clip_sim", "clip_step"):
            curve(key)
        summary["clip_mmd"] = None if clip["mmd"] is None else perceptual.mmd_json(clip["mmd"])
        summary["clip"] = dict(clip["tower"])
    if motion is not None:
        for key in MOTION_KEYS:
            summary["mean_" + key] = scene_mean("mean_" + key)
        for key in ("flow_rms", "flow_rms_real", "flow_epe"):
            curve(key)
        summary["motion"] = dict(motion)
    return summary


# ---- offline: the pictures of an earlier run ----------------------------------------------------------------------------------------------------
def picture_pairs(directory):
    """DIR/virtual/images and DIR/real/images -> [(dataset, index, [(frame, virtual path, real path)])], scenes and frames in ascending order:
    the pictures both sides hold under the reference's names <dataset>_<index:06>_<frame:04>.png."""
    sides = []
    for sub in ("virtual", "real"):
        folder = os.path.join(directory, sub, "images")
        if not os.path.isdir(folder):
            raise FileNotFoundError(f"--compare {directory}: {folder} does not exist (a run without --no_pictures writes it)")
        sides.append({n: os.path.join(folder, n) for n in os.listdir(folder) if PICTURE_NAME.match(n)})
    scenes = {}
    for name in sorted(set(sides[0]) & set(sides[1])):
        m = PICTURE_NAME.match(name)
        scenes.setdefault((m["dataset"], int(m["index"])), []).append((int(m["frame"]), sides[0][name], sides[1][name]))
    if not scenes:
        raise FileNotFoundError(f"--compare {directory}: no picture occurs under both virtual/images and real/images")
    return [(d, i, sorted(frames)) for (d, i), frames in sorted(scenes.items())]


def compare(opt):
    """--compare DIR: the same records and summary from the saved pictures. The bytes are the ones the online run scored, so are the numbers."""
    ranks = check_world()
    try:
        return _compare(opt, ranks).finish() or 0
    finally:
        ranks.leave()


def _compare(opt, ranks):
    """-> the frontdoor.RankedRun of this rank's scenes of picture_pairs (the k-th scene on rank k mod W), scored and not yet finished."""
    import numpy as np
    import torch
    from PIL import Image
    if not 1 <= opt.n_conds:
        raise ValueError(f"--n_conds {opt.n_conds}: at least one conditioning frame")
    ckpt = None
    if SU.eval_clip():   # the tower alone, from --config / --ckpt: a checkpoint that is not there is refused before anything is read
        ckpt = opt.ckpt or SU.VERSION2SPECS[opt.version]["ckpt"]
        if not os.path.isfile(ckpt):
            raise FileNotFoundError(f"--compare with VISTA_EVAL_CLIP=1: the checkpoint {ckpt} does not exist (--ckpt names the file whose "
                                    "image tower scores the pictures)")
    motion_run = motion.RunScores() if SU.eval_motion() else None   # (a bad VISTA_EVAL_MOTION is refused by name, before anything is read)
    scenes = picture_pairs(opt.compare)
    if motion_run is not None:   # every picture's size from its header, before anything is scored
        for dataset, index, frames in scenes:
            for entry in frames:
                for path in entry[1:]:
                    with Image.open(path) as im:
                        motion.check_size(im.height, im.width, f"--compare {opt.compare} with VISTA_EVAL_MOTION=1: {os.path.basename(path)}")
    if not torch.cuda.is_available():
        raise VistaHipError("evaluate --compare: no GPU is visible; vista_amd runs on the MI355X only (no CPU / eager fallback)")
    ranks.join()
    clip_run = perceptual.RunScores(perceptual.load_tower(opt.config, ckpt)) if ckpt is not None else None
    run = _ranked_run(ranks, opt.compare, clip_run, motion_run)
    for k, (dataset, index, frames) in run.own(scenes):
        t0 = time.perf_counter()
        stacks = []
        for side in (1, 2):
            pictures = []
            for entry in frames:
                with Image.open(entry[side]) as im:
                    pictures.append(np.array(im if im.mode == "RGB" else im.convert("RGB"), dtype=np.uint8))
            if len({p.shape for p in pictures}) != 1:
                raise ValueError(f"--compare {opt.compare}: the pictures of {dataset}_{index:06} differ in size")
            stacks.append(torch.from_numpy(np.stack(pictures)).cuda())
        t1 = time.perf_counter()
        report = fidelity.frame_metrics(stacks[0], stacks[1])
        timings = {"load": t1 - t0, "metrics": time.perf_counter() - t1}
        more = {**_clip_stage(clip_run, stacks[0], stacks[1], opt.n_conds, timings, k), **_motion_stage(motion_run, stacks[0], stacks[1], timings)}
        record = make_record(index, [frames[0][2]], report, seed=opt.seed, action=opt.action, n_conds=opt.n_conds, n_rounds=opt.n_rounds,
                             n_frames=opt.n_frames, timings=timings, **more)
        run.add(k, record)
        print(ranks.prefix + _scene_line(record), flush=True)
    return run


def _ranked_run(ranks, save_dir, clip_run, motion_run):
    """The records and the summary of this run; the CLIP embeddings behind the run-level clip_mmd travel to rank 0 beside the records."""
    return frontdoor.RankedRun(ranks, save_dir, RECORDS_NAME, SUMMARY_NAME, lambda records: _summary(records, clip_run, motion_run),
                               extra=clip_run, extra_name="clip")


def _clip_stage(clip_run, pred_u8, real_u8, n_conds, timings, position=None):
    """The CLIP-space stage behind a scene's metrics -> the clip= keyword of make_record ({} without the hook: the call is the parent's).
    position: the scene's place in the walk, which a scene-per-rank run keeps with the scene's embeddings."""
    if clip_run is None:
        return {}
    t0 = time.perf_counter()
    report = clip_run.scene(pred_u8, real_u8, n_conds, position)   # (its copies to the host end the stage)
    timings["clip"] = time.perf_counter() - t0
    return {"clip": report}


def _motion_stage(motion_run, pred_u8, real_u8, timings):
    """The motion stage behind a scene's metrics -> the motion= keyword of make_record ({} without the hook: the call is the parent's)."""
    if motion_run is None:
        return {}
    t0 = time.perf_counter()
    report = motion_run.scene(pred_u8, real_u8)   # (its copies to the host end the stage)
    timings["motion"] = time.perf_counter() - t0
    return {"motion": report}


def _summary(records, clip_run, motion_run=None):
    more = {} if clip_run is None else {"clip": clip_run.summary()}
    if motion_run is not None:
        more["motion"] = motion_run.summary()
    return summarize(records, **more)


def _scene_line(record):
    keys = ("mean_psnr", "mean_ssim") + (("mean_clip_sim",) if "mean_clip_sim" in record else ())
    keys += ("mean_flow_epe",) if "mean_flow_epe" in record else ()
    shown = ", ".join(f"{k} " + ("null" if record[k] is None else f"{record[k]:.4f}") for k in keys)
    return (f"evaluate {record['index']}: {record['frames_scored']} frames, {shown} | "
            + frontdoor.timings_text(record["timings"]))


# ---- online ---------------------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    opt, _unknown = parse_args(prog="python -m vista_amd.evaluate").parse_known_args(argv)
    if opt.compare is not None:
        return compare(opt)
    # what cannot run is refused here, before 2.5 billion parameters are built
    check_run(opt, frontdoor.net_params(opt))
    ranks = check_world(opt.n_scenes)
    try:
        return _evaluate_loop(opt, ranks.join())
    finally:
        ranks.leave()


def _evaluate_loop(opt, ranks=None):
    """The loop of vista_amd.sample with the metrics stage behind every scene."""
    _evaluate_scenes(opt, ranks or frontdoor.SceneRanks()).finish()
    return 0


def _evaluate_scenes(opt, ranks):
    """-> the frontdoor.RankedRun of this rank's scenes of the walk, sampled, scored and not yet finished."""
    import torch
    from . import ops
    model = frontdoor.build_model(opt, ranks.rank)
    clip_run = perceptual.RunScores(perceptual.find_tower(model)) if SU.eval_clip() else None
    motion_run = motion.RunScores() if SU.eval_motion() else None
    run = _ranked_run(ranks, opt.save, clip_run, motion_run)
    for k, (frame_list, sample_index, _dataset_length, action_dict) in run.scenes(opt, n_scenes=opt.n_scenes):
        timings = {}
        samples, _samples_z, inputs = sample.run(model, frame_list, action_dict, height=opt.height, width=opt.width, n_frames=opt.n_frames,
                                                 n_rounds=opt.n_rounds, n_conds=opt.n_conds, n_steps=opt.n_steps, cfg_scale=opt.cfg_scale,
                                                 cond_aug=opt.cond_aug, eager=opt.eager, timings=timings)
        # ground truth beyond the sampler's window: the scene's own later frames, as far as the annotation lists them
        t0 = time.perf_counter()
        real = inputs
        if samples.shape[0] > inputs.shape[0]:
            more = future_frames(sample_index, opt.n_frames, samples.shape[0], opt.dataset, opt.data_root, opt.anno_file)
            if more:
                real = torch.cat([inputs, SU.load_img_seq(more, opt.height, opt.width, "cuda")])
        scored = min(samples.shape[0], real.shape[0])
        torch.cuda.synchronize()
        timings["load"] = timings.get("load", 0.0) + time.perf_counter() - t0
        t0 = time.perf_counter()
        pred_m, real_m = samples[:scored].float(), real[:scored].float()
        if clip_run is not None or motion_run is not None:   # both stacks to 8 bit once: the same bytes go to every metrics stage
            pred_m, real_m = ops.frames_to_u8(pred_m, real=False), ops.frames_to_u8(real_m, real=True)
        report = fidelity.frame_metrics(pred_m, real_m)   # (its copy to the host ends the stage)
        timings["metrics"] = time.perf_counter() - t0
        more = {**_clip_stage(clip_run, pred_m, real_m, opt.n_conds, timings, k), **_motion_stage(motion_run, pred_m, real_m, timings)}
        if not opt.no_pictures:
            t0 = time.perf_counter()
            frontdoor.save_pictures(opt.save, opt.dataset, sample_index, virtual=samples, real=real)
            timings["save"] = time.perf_counter() - t0
        record = make_record(sample_index, frame_list, report, seed=opt.seed, action=opt.action, n_conds=opt.n_conds, n_rounds=opt.n_rounds,
                             n_frames=opt.n_frames, timings=timings, **more)
        run.add(k, record)
        print(ranks.prefix + _scene_line(record), flush=True)
    return run


if __name__ == "__main__":
    sys.exit(main())
