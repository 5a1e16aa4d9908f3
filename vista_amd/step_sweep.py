"""`python -m vista_amd.step_sweep`: how few sampling steps does this checkpoint need -- every sampler at every step budget against one
converged reference run, scene by scene.

Every flag of `vista_amd.sample` under its name with its default (the parser is built from sample.parse_args); on top: --n_scenes (how many
scenes to sweep; 0 = to the end of the dataset, for the sequential walk only), --samplers and --budgets (comma-separated: the sweep is their
product), --ref_steps / --ref_sampler (the yardstick: one run of that sampler with that many steps).

    python -m vista_amd.step_sweep --ckpt ckpts/vista.safetensors --rand_gen --n_scenes 20 --save outputs

Per scene: load the frames and build the conditioning once, as sample.run does for round 0; draw the noise once, after torch.manual_seed(seed)
under torch.random.fork_rng, and hand every run a clone of it (common random numbers, as in vista_amd.plan: two runs differ by sampler and step
count only). The reference run comes first; then the OTHER sampler at --ref_steps, whose distance to the reference is the record's `ref_gap` --
how converged the yardstick itself is: an error below it says nothing. Then one run per (sampler, budget). Graph replay follows sample's rule (on
unless --eager); the UNet's graphs are keyed by the window's geometry, so the ones the reference run captures serve every run.

Per run: `frame_err[f] = sqrt(sum (z - z_ref)^2 / sum z_ref^2)` over frame f's latent, both sums from vk_loss_stats with T = 1 (its S0-alone form;
fp64, fixed order; the denominators once per scene, z_ref against zeros); `latent_err` is the mean of frame_err over the predicted frames. The
first --n_conds frames are conditioning frames: every run holds them at the encoded input, their error is exactly 0, and they are listed under
`cond` and left out of every mean. `mean_psnr` / `mean_ssim` compare the decoded 8-bit frames with the reference run's (fidelity.frame_metrics,
vk_frame_fidelity_u8); a run whose frames are byte for byte the reference's has an infinite PSNR, written as null. `seconds` is the wall time of
the run's denoising loop (the first run of a geometry includes the graph capture).

One JSON line per scene goes to <save>/steps.jsonl, the means over scenes and the equal-error table to <save>/steps_summary.json; both files
describe this run only. The table names, for each sampler and budget, the smallest budget of every other sampler whose mean latent error is not
larger -- null where none of the budgets swept gets there.

Not measured: quality. The distance to a converged run of the same model says how much of the sampler's own error is left, not how good the
picture is. Not built: rollouts (--n_rounds must be 1), refused by name. The still IMG dataset is allowed. Several GPUs: WORLD_SIZE > 1 is refused
by name unless the environment hook VISTA_SCENE_RANKS=1 is set; then the k-th scene of the walk is swept by rank k mod WORLD_SIZE and rank 0 merges
the records and writes the summary, with a last key "ranks" and every `seconds` its rank's own (frontdoor.SceneRanks / RankedRun; README "Evaluate on
several GPUs": separate processes on one GPU have run, several devices have not, no speed-up has been measured).
"""
import math
import sys
import time

from . import fidelity, frontdoor, sample
from .frontdoor import json_number, mean
from . import sample_utils as SU

DEFAULT_SAMPLERS = "EulerEDMSampler,DPMPP2MSampler"
DEFAULT_BUDGETS = "10,15,20,30,50"
RECORDS_NAME, SUMMARY_NAME = "steps.jsonl", "steps_summary.json"
RUN_FIELDS = ("sampler", "steps", "latent_err", "frame_err", "mean_psnr", "mean_ssim", "seconds")


def parse_args(**parser_kwargs):
    parser = sample.parse_args(**parser_kwargs)
    add = parser.add_argument
    add("--n_scenes", type=int, default=0, help="number of scenes to sweep (0: to the end of the dataset; needs the sequential walk, --rand_gen)")
    add("--samplers", type=str, default=DEFAULT_SAMPLERS, help="comma-separated sampler classes to sweep")
    add("--budgets", type=str, default=DEFAULT_BUDGETS, help="comma-separated step counts to sweep")
    add("--ref_steps", type=int, default=200, help="steps of the reference run every other run is measured against")
    add("--ref_sampler", type=str, default="DPMPP2MSampler", help="sampler of the reference run")
    return parser


def parse_samplers(text):
    """"A,B" -> ["A", "B"]; every name must be a sampler this package builds."""
    names = [s.strip() for s in str(text).split(",") if s.strip()]
    if not names:
        raise ValueError(f"--samplers {text!r}: an empty sampler list; one or more of {', '.join(SU.SAMPLERS)}")
    out = []
    for name in names:
        if name not in SU.SAMPLERS:
            raise ValueError(f"--samplers: Unknown sampler {name}: one of {', '.join(SU.SAMPLERS)}")
        if name not in out:
            out.append(name)
    return out


def parse_budgets(text, ref_steps):
    """"10,20" -> [10, 20]: step counts between 1 and ref_steps."""
    parts = [s.strip() for s in str(text).split(",") if s.strip()]
    if not parts:
        raise ValueError(f"--budgets {text!r}: an empty budget list; give step counts, e.g. {DEFAULT_BUDGETS}")
    out = []
    for part in parts:
        try:
            n = int(part)
        except ValueError:
            raise ValueError(f"--budgets {text!r}: {part!r} is no step count") from None
        if n < 1:
            raise ValueError(f"--budgets {text!r}: a budget of {n} steps; a run takes at least 1 step")
        if n > ref_steps:
            raise ValueError(f"--budgets {text!r}: a budget of {n} steps is above --ref_steps {ref_steps}; the reference run must be the finest")
        if n not in out:
            out.append(n)
    return out


def check_run(opt, net_params=None):
    """Refuses, by name and before any model is built, what a sweep cannot do. -> (samplers, budgets)."""
    SU.check_sizes(opt.height, opt.width, opt.n_frames, opt.n_rounds, opt.n_conds, net_params)
    if opt.height < fidelity.TAPS or opt.width < fidelity.TAPS:
        raise ValueError(f"--height {opt.height} --width {opt.width}: SSIM takes an {fidelity.TAPS} x {fidelity.TAPS} window")
    if opt.ref_sampler not in SU.SAMPLERS:
        raise ValueError(f"--ref_sampler: Unknown sampler {opt.ref_sampler}: one of {', '.join(SU.SAMPLERS)}")
    samplers = parse_samplers(opt.samplers)
    if opt.ref_steps < 1:
        raise ValueError(f"--ref_steps {opt.ref_steps}: the reference run takes at least 1 step")
    budgets = parse_budgets(opt.budgets, opt.ref_steps)
    if opt.n_rounds != 1:
        raise ValueError(f"--n_rounds {opt.n_rounds}: the sweep compares single windows (a rollout's later rounds start from the earlier ones' "
                         "results, so their errors do not separate); give --n_rounds 1")
    if opt.n_conds >= opt.n_frames:
        raise ValueError(f"--n_conds {opt.n_conds} with --n_frames {opt.n_frames}: every frame would be a conditioning frame, nothing is left to compare")
    frontdoor.check_scene_count(opt)
    return samplers, budgets


class SweepReport:
    """What run() returns: ref_sampler, ref_steps, ref_seconds, ref_gap (the other sampler's latent_err at ref_steps), cond (the conditioning
    frames' indices) and runs, one dict per (sampler, budget) with RUN_FIELDS. Python numbers; None for a PSNR that is not finite."""

    def __init__(self, ref_sampler, ref_steps, ref_seconds, ref_gap, cond, runs):
        self.ref_sampler, self.ref_steps, self.ref_seconds, self.ref_gap, self.cond, self.runs = ref_sampler, ref_steps, ref_seconds, ref_gap, cond, runs

    def __repr__(self):
        return f"SweepReport({self.__dict__})"


def clip_error(frame_err, cond):
    """The clip's figure: the mean of the per-frame errors over the frames that are not conditioning frames."""
    return mean([float(v) for i, v in enumerate(frame_err) if i not in set(cond)])


def other_sampler(name):
    """The sampler the reference is cross-checked with: the first one this package builds that is not `name`."""
    return [s for s in SU.SAMPLERS if s != name][0]


def run(model, frame_list, action_dict=None, *, height=576, width=1024, n_frames=25, n_conds=1, cfg_scale=2.5, cond_aug=0.0, eager=False, seed=23,
        samplers=("EulerEDMSampler", "DPMPP2MSampler"), budgets=(10, 15, 20, 30, 50), ref_steps=200, ref_sampler="DPMPP2MSampler"):
    """One scene -> SweepReport. The caller seeds torch's generator (the conditioning frame's augmentation noise, as for sample.run); the
    sampling noise is drawn here from `seed` and shared by every run."""
    import torch
    from . import ops
    samplers, budgets = [str(s) for s in samplers], [int(b) for b in budgets]
    for name in samplers + [ref_sampler]:
        if name not in SU.SAMPLERS:
            raise ValueError(f"Unknown sampler {name}: one of {', '.join(SU.SAMPLERS)}")
    if not budgets or min(budgets) < 1 or max(budgets) > ref_steps:
        raise ValueError(f"budgets {budgets}: one or more step counts between 1 and ref_steps ({ref_steps})")
    if not 0 <= n_conds < n_frames:
        raise ValueError(f"n_conds {n_conds} with n_frames {n_frames}: nothing is left to compare")
    cond = list(range(n_conds))
    with torch.no_grad(), model.ema_scope("Sampling"):
        images = SU.load_img_seq(frame_list, height, width, "cuda")
        value_dict = frontdoor.first_window_values(model, images, cond_aug, action_dict)
        condition = getattr(model, "condition_fn", None) or SU.get_condition
        c, uc = condition(model, value_dict, n_frames, sample.UC_KEYS, "cuda")
        z = model.encode_first_stage(images)
        first_mask, _carry = SU.rollout_masks(n_frames, cond, "cuda")
        denoiser = SU.rollout_denoiser(model)
        with torch.random.fork_rng(devices=[z.device]):
            torch.manual_seed(seed)
            noise = torch.randn_like(z)

        def one(name, steps):
            """-> (latents fp32, decoded frames uint8, seconds of the denoising loop)"""
            sampler = SU.init_sampling(sampler=name, guider="VanillaCFG", steps=steps, cfg_scale=cfg_scale, num_frames=n_frames)
            sampler.graph = sampler.cfg_streams = not eager
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            latents = SU.first_round(sampler, denoiser, c, uc, z, first_mask, lambda like: noise.clone())
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            frames = torch.clamp((model.decode_first_stage(latents) + 1.0) / 2.0, min=0.0, max=1.0)   # (do_sample's expression)
            return latents.float().contiguous(), ops.frames_to_u8(frames.float(), real=False), seconds

        z_ref, u8_ref, ref_seconds = one(ref_sampler, ref_steps)
        norms = [float(v) for v in ops.loss_stats(z_ref, torch.zeros_like(z_ref), 1)[:, 0].cpu()]   # sum z_ref^2 per frame, once per scene

        def measure(name, steps):
            latents, u8, seconds = one(name, steps)
            dist = [float(v) for v in ops.loss_stats(latents, z_ref, 1)[:, 0].cpu()]
            frame_err = [math.sqrt(d / n) if n > 0.0 else (0.0 if d == 0.0 else float("inf")) for d, n in zip(dist, norms)]
            rep = fidelity.frame_metrics(u8, u8_ref)
            pred = [i for i in range(len(frame_err)) if i not in cond]
            return {"sampler": name, "steps": int(steps), "latent_err": clip_error(frame_err, cond), "frame_err": frame_err,
                    "mean_psnr": json_number(mean([float(rep.psnr[i]) for i in pred])), "mean_ssim": json_number(mean([float(rep.ssim[i]) for i in pred])),
                    "seconds": seconds}

        ref_gap = measure(other_sampler(ref_sampler), ref_steps)["latent_err"]
        runs = [measure(name, steps) for name in samplers for steps in budgets]
    return SweepReport(ref_sampler, int(ref_steps), ref_seconds, ref_gap, cond, runs)


# ---- records ------------------------------------------------------------------------------------------------------------------------------
def settings_of(opt):
    return {"seed": opt.seed, "action": opt.action, "n_frames": opt.n_frames, "n_conds": opt.n_conds, "height": opt.height, "width": opt.width,
            "cfg_scale": opt.cfg_scale, "cond_aug": opt.cond_aug, "eager": bool(opt.eager), "samplers": parse_samplers(opt.samplers),
            "budgets": parse_budgets(opt.budgets, opt.ref_steps), "ref_steps": opt.ref_steps, "ref_sampler": opt.ref_sampler}


def make_record(index, frame_list, report, settings):
    return {"index": int(index), "frames": [frame_list[0]], "seed": int(settings["seed"]), "settings": settings, "cond": [int(i) for i in report.cond],
            "ref_sampler": report.ref_sampler, "ref_steps": int(report.ref_steps), "ref_seconds": round(float(report.ref_seconds), 4),
            "ref_gap": json_number(report.ref_gap),
            "runs": [{"sampler": r["sampler"], "steps": int(r["steps"]), "latent_err": json_number(r["latent_err"]),
                      "frame_err": [json_number(v) for v in r["frame_err"]], "mean_psnr": r["mean_psnr"], "mean_ssim": r["mean_ssim"],
                      "seconds": round(float(r["seconds"]), 4)} for r in report.runs]}


def summarise(records):
    """A pure function of the records: the means over scenes per (sampler, steps) and the equal-error table. A run's error is the mean of its
    frame_err over the frames its record does not list under `cond`. equal_error: for each (sampler, steps), `matched_by` maps every OTHER
    sampler to its smallest budget whose mean latent error is not larger (a tie counts), or None where no budget of it gets there."""
    if not records:
        return {"scenes": 0, "ref_gap": None, "runs": [], "equal_error": []}
    keys = []
    for rec in records:
        for r in rec["runs"]:
            if (r["sampler"], r["steps"]) not in keys:
                keys.append((r["sampler"], r["steps"]))
    runs = []
    for name, steps in keys:
        rows = [(rec, r) for rec in records for r in rec["runs"] if (r["sampler"], r["steps"]) == (name, steps)]
        errs = [clip_error(r["frame_err"], rec["cond"]) for rec, r in rows]

        def mean_of(field):
            vals = [r[field] for _rec, r in rows]
            return None if any(v is None for v in vals) else json_number(mean(vals))
        runs.append({"sampler": name, "steps": steps, "scenes": len(rows), "latent_err": json_number(mean(errs)), "mean_psnr": mean_of("mean_psnr"),
                     "mean_ssim": mean_of("mean_ssim"), "seconds": mean_of("seconds")})
    names = []
    for name, _steps in keys:
        if name not in names:
            names.append(name)
    table = []
    for row in runs:
        matched = {}
        for other in names:
            if other == row["sampler"]:
                continue
            reach = [o["steps"] for o in runs if o["sampler"] == other and o["latent_err"] is not None and row["latent_err"] is not None
                     and o["latent_err"] <= row["latent_err"]]
            matched[other] = min(reach) if reach else None
        table.append({"sampler": row["sampler"], "steps": row["steps"], "latent_err": row["latent_err"], "matched_by": matched})
    gaps = [rec.get("ref_gap") for rec in records]
    return {"scenes": len(records), "ref_sampler": records[0].get("ref_sampler"), "ref_steps": records[0].get("ref_steps"),
            "ref_gap": None if any(g is None for g in gaps) else json_number(mean(gaps)), "runs": runs, "equal_error": table}


def _scene_line(record):
    shown = ", ".join(f"{r['sampler'][:5]}@{r['steps']} " + ("null" if r["latent_err"] is None else f"{r['latent_err']:.3e}") for r in record["runs"])
    gap = "null" if record["ref_gap"] is None else f"{record['ref_gap']:.3e}"
    return f"step_sweep {record['index']}: ref {record['ref_sampler']}@{record['ref_steps']} (gap {gap}) | {shown}"


def main(argv=None):
    opt, _unknown = parse_args(prog="python -m vista_amd.step_sweep").parse_known_args(argv)
    # what cannot run is refused here, before 2.5 billion parameters are built
    samplers, budgets = check_run(opt, frontdoor.net_params(opt))
    ranks = frontdoor.scene_ranks("step_sweep", "scene-per-rank sweeping with a merge of the records is not built", opt.n_scenes)
    try:
        return _sweep_loop(opt, samplers, budgets, ranks.join())
    finally:
        ranks.leave()


def _sweep_loop(opt, samplers, budgets, ranks=None):
    """The walk of vista_amd.sample over the dataset with the sweep behind every scene."""
    _sweep_scenes(opt, samplers, budgets, ranks or frontdoor.SceneRanks()).finish()
    return 0


def _sweep_scenes(opt, samplers, budgets, ranks):
    """-> the frontdoor.RankedRun of this rank's scenes of the walk, swept and not yet finished."""
    model = frontdoor.build_model(opt, ranks.rank)
    run_, settings = frontdoor.RankedRun(ranks, opt.save, RECORDS_NAME, SUMMARY_NAME, summarise), settings_of(opt)
    for k, (frame_list, sample_index, _dataset_length, action_dict) in run_.scenes(opt, n_scenes=opt.n_scenes):
        report = run(model, frame_list, action_dict, height=opt.height, width=opt.width, n_frames=opt.n_frames, n_conds=opt.n_conds,
                     cfg_scale=opt.cfg_scale, cond_aug=opt.cond_aug, eager=opt.eager, seed=opt.seed, samplers=samplers, budgets=budgets,
                     ref_steps=opt.ref_steps, ref_sampler=opt.ref_sampler)
        record = make_record(sample_index, frame_list, report, settings)
        run_.add(k, record)
        print(ranks.prefix + _scene_line(record), flush=True)
    return run_


if __name__ == "__main__":
    sys.exit(main())
