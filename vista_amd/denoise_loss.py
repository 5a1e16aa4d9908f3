"""`python -m vista_amd.denoise_loss`: the denoising loss of a checkpoint on real frames -- the number the model was trained on -- per noise level.

Every flag of `vista_amd.sample` under its name with its default (the parser is built from sample.parse_args); on top: --n_scenes (how many
scenes to score; 0 = to the end of the dataset, for the sequential walk only), --n_sigmas / --p_mean / --p_std (the grid of noise levels: the
mid-quantiles of the sigma sampler's log-normal, sigma_i = exp(p_mean + p_std * Phi^-1((i + 0.5) / n)); the same for every scene, checkpoint and
build), --loss_type, --weighting, --no_additional_loss, --additional_loss_weight, --offset_noise_level and --noise_seed.

    python -m vista_amd.denoise_loss --ckpt ckpts/vista.safetensors --rand_gen --n_scenes 50 --save outputs

Per scene: load n_frames real frames and encode all of them; build the conditioning as sample.run builds round 0's; the first --n_conds frames are
conditioning frames (kept clean, excluded from the loss, as the reference's replace_cond_frames does). Per noise level i: the noise is drawn after
torch.manual_seed(noise_seed + i) under torch.random.fork_rng -- the same draw for every scene and run (common random numbers, as in
vista_amd.plan) --, one eager denoiser forward of the whole clip (no guidance, no graph replay), then StandardDiffusionLoss's kernels
(csrc/loss.hip). One JSON line per scene goes to <save>/loss.jsonl, the means over scenes to <save>/loss_summary.json; both files describe this
run only. Forward only: this measures, it does not train.

Per noise level a record holds `loss` (the reference's scalar: the mean over the clip's images of the weighted loss, with the dynamics and
structure terms unless --no_additional_loss) and three unweighted means over the clip's images: `mse` (of e), `dynamics` (of e * aux_w, the
dynamics-enhanced error) and `structure` (of the Fourier high-pass term), so that with --weighting Unit loss = dynamics + additional_loss_weight *
structure. `frame_mse` is the unweighted mean of e per frame. A conditioning frame contributes exactly 0 to every figure, as in the reference's
replace_cond_frames. With --loss_type l1, e is the absolute error.

Several GPUs: WORLD_SIZE > 1 is refused by name unless the environment hook VISTA_SCENE_RANKS=1 is set; then the k-th scene of the walk is scored
by rank k mod WORLD_SIZE and rank 0 merges the records and writes the summary, with a last key "ranks" (frontdoor.SceneRanks / RankedRun; README
"Evaluate on several GPUs": separate processes on one GPU have run, several devices have not, no speed-up has been measured).
The still IMG dataset is allowed: the loss of a still clip is well defined. Random conditioning-frame choices and gradients are not built.
"""
import math
import sys
import time
from statistics import NormalDist

from . import frontdoor, sample
from .frontdoor import mean
from . import sample_utils as SU

WEIGHTINGS = {"V": "VWeighting", "EDM": "EDMWeighting", "Eps": "EpsWeighting", "Unit": "UnitWeighting"}
RECORDS_NAME, SUMMARY_NAME = "loss.jsonl", "loss_summary.json"
FIELDS = ("loss", "mse", "dynamics", "structure")


def parse_args(**parser_kwargs):
    parser = sample.parse_args(**parser_kwargs)
    add = parser.add_argument
    add("--n_scenes", type=int, default=0, help="number of scenes to score (0: to the end of the dataset; needs the sequential walk, --rand_gen)")
    add("--n_sigmas", type=int, default=8, help="number of noise levels: the mid-quantiles of the log-normal sigma sampler")
    add("--p_mean", type=float, default=1.0, help="mean of log sigma (phase 2 training: 1.0)")
    add("--p_std", type=float, default=1.6, help="standard deviation of log sigma (phase 2 training: 1.6)")
    add("--loss_type", type=str, default="l2", choices=["l2", "l1"], help="squared or absolute error")
    add("--weighting", type=str, default="V", choices=list(WEIGHTINGS), help="the loss weight w(sigma)")
    add("--no_additional_loss", action="store_true", help="the plain denoising loss, without the dynamics and structure terms")
    add("--additional_loss_weight", type=float, default=0.1, help="weight of the structure (Fourier high-pass) term")
    add("--offset_noise_level", type=float, default=0.0, help="offset noise per (frame, channel); 0 for evaluation (phase 2 trains with 0.02)")
    add("--noise_seed", type=int, default=0, help="noise level i draws its noise after torch.manual_seed(noise_seed + i)")
    return parser


def sigma_grid(n_sigmas, p_mean=1.0, p_std=1.6):
    """The mid-quantiles of the sigma sampler's log-normal, ascending: exp(p_mean + p_std * Phi^-1((i + 0.5) / n)). Python floats."""
    if n_sigmas < 1:
        raise ValueError(f"--n_sigmas {n_sigmas}: at least one noise level")
    normal = NormalDist()
    return [math.exp(p_mean + p_std * normal.inv_cdf((i + 0.5) / n_sigmas)) for i in range(n_sigmas)]


def check_run(opt, net_params=None):
    """Refuses, by name and before any model is built, what a loss run cannot do."""
    from . import ops
    SU.check_sizes(opt.height, opt.width, opt.n_frames, opt.n_rounds, opt.n_conds, net_params)
    if opt.n_sigmas < 1:
        raise ValueError(f"--n_sigmas {opt.n_sigmas}: at least one noise level")
    if opt.n_conds >= opt.n_frames:
        raise ValueError(f"--n_conds {opt.n_conds} with --n_frames {opt.n_frames}: every frame would be a conditioning frame, nothing is left to score")
    if not opt.no_additional_loss and not ops.fourier_highpass_fits(opt.height // 8, opt.width // 8):
        raise ValueError(f"--height {opt.height} --width {opt.width}: the structure term's Fourier high-pass keeps a latent plane in one workgroup's "
                         f"LDS, and a {opt.height // 8} x {opt.width // 8} plane does not fit (16 h w + 16 (h + w) <= 160 KiB; 72 x 128 does); "
                         "give --no_additional_loss for the plain denoising loss")
    frontdoor.check_scene_count(opt)


class LossReport:
    """What run() returns: sigmas [S], loss / mse / dynamics / structure [S], frame_mse [S][T], cond (the conditioning frames' indices). Python floats."""

    def __init__(self, sigmas, loss, mse, dynamics, structure, frame_mse, cond):
        self.sigmas, self.loss, self.mse, self.dynamics, self.structure = sigmas, loss, mse, dynamics, structure
        self.frame_mse, self.cond = frame_mse, cond

    def __eq__(self, other):
        return isinstance(other, LossReport) and self.__dict__ == other.__dict__

    def __repr__(self):
        return f"LossReport({self.__dict__})"


def make_loss_fn(n_frames, *, p_mean=1.0, p_std=1.6, loss_type="l2", weighting="V", additional=True, additional_loss_weight=0.1,
                 offset_noise_level=0.0):
    from .modules.diffusionmodules.loss import StandardDiffusionLoss
    P = "vwm.modules.diffusionmodules."
    return StandardDiffusionLoss(
        sigma_sampler_config={"target": P + "sigma_sampling.EDMSampling", "params": {"p_mean": p_mean, "p_std": p_std, "num_frames": n_frames}},
        loss_weighting_config={"target": P + "loss_weighting." + WEIGHTINGS[weighting]}, loss_type=loss_type, use_additional_loss=additional,
        offset_noise_level=offset_noise_level, additional_loss_weight=additional_loss_weight, num_frames=n_frames, replace_cond_frames=True,
        cond_frames_choices=[[]])


def run(model, frame_list, action_dict=None, *, height=576, width=1024, n_frames=25, n_conds=1, cond_aug=0.0, n_sigmas=8, p_mean=1.0, p_std=1.6,
        loss_type="l2", weighting="V", additional=True, additional_loss_weight=0.1, offset_noise_level=0.0, noise_seed=0, timings=None):
    """One scene -> LossReport. The caller seeds (the conditioning frame's augmentation noise); the noise of the loss is seeded here."""
    import torch
    if not 0 <= n_conds < n_frames:
        raise ValueError(f"n_conds {n_conds} with n_frames {n_frames}: nothing is left to score")
    sigmas = sigma_grid(n_sigmas, p_mean, p_std)
    loss_fn = make_loss_fn(n_frames, p_mean=p_mean, p_std=p_std, loss_type=loss_type, weighting=weighting, additional=additional,
                           additional_loss_weight=additional_loss_weight, offset_noise_level=offset_noise_level)
    clock = {"load": 0.0, "condition": 0.0, "encode": 0.0, "forward": 0.0, "loss": 0.0}

    def lap(stage, t0):
        torch.cuda.synchronize()
        clock[stage] += time.perf_counter() - t0
        return time.perf_counter()

    with torch.no_grad(), model.ema_scope("Sampling"):   # (the weights do_sample scores: a model that carries EMA weights swaps them in here)
        t0 = time.perf_counter()
        images = SU.load_img_seq(frame_list, height, width, "cuda")
        t0 = lap("load", t0)
        value_dict = frontdoor.first_window_values(model, images, cond_aug, action_dict)
        condition = getattr(model, "condition_fn", None) or SU.get_condition
        c, _uc = condition(model, value_dict, n_frames, sample.UC_KEYS, "cuda")   # (round 0's conditioning of sample.run; uc is dropped)
        t0 = lap("condition", t0)
        z = model.encode_first_stage(images).float().contiguous()
        t0 = lap("encode", t0)
        n = z.shape[0]
        cond_mask = torch.zeros(n, device=z.device)
        cond_mask[:n_conds] = 1
        per_image = z[0].numel()
        out = {k: [] for k in FIELDS}
        frame_mse = []
        for i, sigma in enumerate(sigmas):
            t0 = time.perf_counter()
            with torch.random.fork_rng(devices=[z.device]):
                torch.manual_seed(noise_seed + i)
                noise = torch.randn_like(z)
                offset = torch.randn((n, z.shape[1]), device=z.device) if offset_noise_level > 0.0 else None
            sig = torch.full((n,), sigma, dtype=torch.float32, device=z.device)
            spent = {"forward": 0.0}

            def denoiser(network, noised_input, s, cond, mask):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                result = model.denoiser(network, noised_input, s, cond, mask)
                torch.cuda.synchronize()
                spent["forward"] = time.perf_counter() - t1
                return result
            loss, sums, _w = loss_fn._forward(model.model, denoiser, c, z, sigmas=sig, cond_mask=cond_mask, noise=noise, offset=offset,
                                              return_sums=True)   # (the sums' copy to the host ends the stage)
            total = time.perf_counter() - t0
            clock["forward"] += spent["forward"]
            clock["loss"] += total - spent["forward"]
            out["loss"].append(float(loss.mean()))
            out["mse"].append(float(sums[:, 0].sum() / (n * per_image)))
            out["dynamics"].append(float(sums[:, 1].sum() / (n * per_image)))
            out["structure"].append(float(sums[:, 2].sum() / (n * per_image)))
            frame_mse.append([float(v) / per_image for v in sums[:, 0]])
    if timings is not None:
        timings.update(clock)
    return LossReport(sigmas, out["loss"], out["mse"], out["dynamics"], out["structure"], frame_mse, list(range(n_conds)))


# ---- records ------------------------------------------------------------------------------------------------------------------------------
def make_record(index, frame_list, report, opt_or_settings, timings=None):
    s = opt_or_settings if isinstance(opt_or_settings, dict) else settings_of(opt_or_settings)
    return {"index": int(index), "frames": [frame_list[0]], "seed": int(s["seed"]), "noise_seed": int(s["noise_seed"]), "settings": s,
            "sigmas": [float(v) for v in report.sigmas], **{k: [float(v) for v in getattr(report, k)] for k in FIELDS},
            "frame_mse": [[float(v) for v in row] for row in report.frame_mse], "cond": [int(i) for i in report.cond],
            "timings": frontdoor.rounded_timings(timings)}


def settings_of(opt):
    return {"seed": opt.seed, "noise_seed": opt.noise_seed, "action": opt.action, "n_frames": opt.n_frames, "n_conds": opt.n_conds,
            "height": opt.height, "width": opt.width, "cond_aug": opt.cond_aug, "n_sigmas": opt.n_sigmas, "p_mean": opt.p_mean, "p_std": opt.p_std,
            "loss_type": opt.loss_type, "weighting": opt.weighting, "additional_loss": not opt.no_additional_loss,
            "additional_loss_weight": opt.additional_loss_weight, "offset_noise_level": opt.offset_noise_level}


def summarize(records):
    """Scene count, the per-sigma means over scenes of every figure, and the per-frame curve (mean frame_mse over scenes, [n_sigmas][T])."""
    if not records:
        return {"scenes": 0, "sigmas": [], **{k: [] for k in FIELDS}, "frame_mse": [], "cond": []}
    S = len(records[0]["sigmas"])
    T = len(records[0]["frame_mse"][0])
    return {"scenes": len(records), "sigmas": records[0]["sigmas"],
            **{k: [mean([r[k][i] for r in records]) for i in range(S)] for k in FIELDS},
            "frame_mse": [[mean([r["frame_mse"][i][t] for r in records]) for t in range(T)] for i in range(S)], "cond": records[0]["cond"]}


def _scene_line(record):
    return (f"denoise_loss {record['index']}: " + ", ".join(f"sigma {s:.3g} loss {v:.5g}" for s, v in zip(record["sigmas"], record["loss"])) + " | "
            + frontdoor.timings_text(record["timings"]))


def main(argv=None):
    opt, _unknown = parse_args(prog="python -m vista_amd.denoise_loss").parse_known_args(argv)
    # what cannot run is refused here, before 2.5 billion parameters are built
    check_run(opt, frontdoor.net_params(opt))
    ranks = frontdoor.scene_ranks("denoise_loss", "scene-per-rank scoring with a merge of the records is not built", opt.n_scenes)
    try:
        return _loss_loop(opt, ranks.join())
    finally:
        ranks.leave()


def _loss_loop(opt, ranks=None):
    """The walk of vista_amd.sample over the dataset with the loss behind every scene."""
    _loss_scenes(opt, ranks or frontdoor.SceneRanks()).finish()
    return 0


def _loss_scenes(opt, ranks):
    """-> the frontdoor.RankedRun of this rank's scenes of the walk, scored and not yet finished."""
    model = frontdoor.build_model(opt, ranks.rank)
    run_, settings = frontdoor.RankedRun(ranks, opt.save, RECORDS_NAME, SUMMARY_NAME, summarize), settings_of(opt)
    for k, (frame_list, sample_index, _dataset_length, action_dict) in run_.scenes(opt, n_scenes=opt.n_scenes):
        timings = {}
        report = run(model, frame_list, action_dict, height=opt.height, width=opt.width, n_frames=opt.n_frames, n_conds=opt.n_conds,
                     cond_aug=opt.cond_aug, n_sigmas=opt.n_sigmas, p_mean=opt.p_mean, p_std=opt.p_std, loss_type=opt.loss_type,
                     weighting=opt.weighting, additional=not opt.no_additional_loss, additional_loss_weight=opt.additional_loss_weight,
                     offset_noise_level=opt.offset_noise_level, noise_seed=opt.noise_seed, timings=timings)
        record = make_record(sample_index, frame_list, report, settings, timings)
        run_.add(k, record)
        print(ranks.prefix + _scene_line(record), flush=True)
    return run_


if __name__ == "__main__":
    sys.exit(main())
