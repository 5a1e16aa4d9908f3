"""`python -m vista_amd.plan`: a rollout that chooses its own actions -- before every round a list of candidate actions is scored by Vista's
reward (low disagreement between an ensemble of imagined futures), and the round is stepped under the best one.

    p = Planner(DriveSession(model, frame_list, ...), ens_size=5, score_steps=10)
    scores = p.score([{"command": torch.tensor(1)}, {"command": torch.tensor(2)}, {}])   # the session is left exactly as it was
    result, scores = p.step([...])                                                       # score, then session.step(actions[scores.best])

One layer above vista_amd.drive (the session) and vista_amd.reward (the objective). What scoring a round costs, for K candidates and E members:
ONE 14-frame decode of the last window (it depends on the session only), ONE conditioner run per candidate (it depends on the candidate only),
K * E sampler runs of `score_steps` steps, and one call of vk_candidate_frame_stats, which returns every candidate's per-frame variance sums,
their total and the index of the smallest. A planner written over fork() + step() pays K * E decodes and conditioner runs instead.

The numbers. Round 0 scores frames [1, T) of the window grown from the encoded pictures (sample_utils.first_round; frame 0 is the conditioning
frame in every member), a later round frames [3, T) of the window grown from the session's last three latents (sample_utils.next_round's
halves). reward = exp(-total / (T' C h w)) with T' the number of SCORED frames: the mean is over predicted frames only, so that the rounds of a
rollout compare with each other. vista_amd.reward, like the reference, divides round 0's total by all T frames (the conditioning frame's zero
included): its reward for the same ensemble is exp(-(T - 1) / T * mean_variance) of this module's.

Random numbers. Member e of round r draws its noise after torch.manual_seed(score_seed + r * ens_size + e), the same draw for every candidate
(common random numbers, as reward_utils.estimate): two candidates' rewards differ by their actions, not by their draws. Scoring runs under
torch.random.fork_rng for the session's device: torch's CPU and GPU generator states, the session's tensors and its round count are after
score() what they were before it, so the committed rollout is the one `vista_amd.drive --script` gives for the chosen actions under the same seed.

The CLI takes every flag of vista_amd.drive except --script; on top --candidates FILE, --ens_size, --score_steps, --score_seed.

    python -m vista_amd.plan --ckpt ckpts/vista.safetensors --action cmd --n_rounds 3 --candidates turns.json --hud --save outputs

    {"candidates": [{"command": 1}, {"command": 2}, "scene", {}]}            the same list before every round (--n_rounds rounds)
    {"rounds": [[{"command": 1}, {}], [{"goal": [800, 450]}, "scene"]]}       a list per round (the number of lists is the number of rounds)

An entry is a drive script entry (drive.check_entry / entry_action). A "scene" entry the scene's annotation cannot supply is listed with
"reward": null and the reason, and is not a candidate. Files: vista_amd.drive's pictures, videos and --hud for the chosen actions, and
<save>/plan.jsonl: drive's record with every round extended by "candidates" ([{"action", "reward", "mean_variance", "frame_variance"}]) and
"chosen" (an index into that list; the round's "action" is the chosen entry), timings by "score".

Not built: several GPUs (WORLD_SIZE > 1 is refused by name), heat maps of the candidates, another objective than the ensemble variance, a
search deeper than one round.
"""
import collections
import functools
import json
import sys
import time

from . import drive, frontdoor, sample
from .frontdoor import json_number
from . import sample_utils as SU

CandidateScores = collections.namedtuple("CandidateScores", "best reward mean_variance frame_variance t0 map")
CandidateScores.__doc__ = """What one round's candidates scored. best: the index of the highest reward (the smallest variance total: ties to the
lowest index, a NaN never), -1 if every candidate's total is NaN; reward (K,), mean_variance (K,), frame_variance (K, T') float64 on the CPU;
t0: the first scored frame of the window (T' = T - t0); map (K, T', h, w) float32 on the GPU, or None."""
RECORDS_NAME = "plan.jsonl"
ENS_MAX = 64   # vk_candidate_frame_stats takes 2 .. 64 members


def check_ensemble(ens_size, score_steps):
    if not 2 <= ens_size <= ENS_MAX:
        raise ValueError(f"ens_size {ens_size}: the planner's reward is an unbiased ensemble variance over 2 .. {ENS_MAX} members")
    if score_steps < 1:
        raise ValueError(f"score_steps {score_steps}: a scoring run has at least one denoising step")


def scores_of(x, t0, want_map=False):
    """x (K, E, T, C, h, w) f32, the members of every candidate's ensemble -> CandidateScores over the frames [t0, T)
    (ops.candidate_frame_stats; the one synchronisation of a scoring round is the copy of its results to the host)."""
    import torch
    from . import ops
    frame_sum, total, best, fmap = ops.candidate_frame_stats(x, t0, want_map=want_map)
    per_frame = x[0, 0, 0].numel()
    frame_variance = frame_sum.cpu() / per_frame
    mean_variance = total.cpu() / (per_frame * frame_variance.shape[1])
    return CandidateScores(int(best), torch.exp(-mean_variance), mean_variance, frame_variance, t0, fmap)


def require_best(scores, r, where=None):
    """The chosen index of round r, or a RuntimeError that names the round when no candidate has a number."""
    if scores.best < 0:
        raise RuntimeError(f"plan: round {r}" + (f" of {where}" if where else "") + f": the variance total of every one of the "
                           f"{scores.reward.numel()} candidates is NaN; there is nothing to choose")
    return scores.best


class Planner:
    """Scores candidate actions for the next round of a DriveSession and steps it under the best. The scoring sampler has `score_steps` steps
    and the session's guider, cfg_scale and -- unless `eager` says otherwise -- graph settings; the UNet's captured graphs are keyed by the
    window's geometry, so the graphs the session's sampler captured serve this one as well. `sampler`: the scoring sampler's class, as in
    sample.run (None = the environment hook VISTA_SAMPLER)."""

    def __init__(self, session, *, ens_size=5, score_steps=10, score_seed=0, eager=None, sampler=None):
        check_ensemble(ens_size, score_steps)
        self.session, self.ens_size, self.score_steps, self.score_seed = session, ens_size, score_steps, score_seed
        self.sampler = SU.init_sampling(sampler=SU.sampler_name(sampler), guider=session.guider, steps=score_steps, cfg_scale=session.cfg_scale, num_frames=session.n_frames)
        graph = bool(session.sampler.graph) if eager is None else not eager
        self.sampler.graph = self.sampler.cfg_streams = graph

    def score(self, actions, want_map=False):
        """actions: a list of action dicts (as DriveSession.step takes them) -> CandidateScores for the session's NEXT round. See the module's
        docstring for what is scored, what it costs and what it leaves untouched (everything)."""
        import torch
        actions = [dict(a or {}) for a in actions]
        if not actions:
            raise ValueError("Planner.score: no candidate actions")
        s = self.session
        model, T, r = s.model, s.n_frames, s.rounds
        get_condition = model.condition_fn
        base = dict(s._scalars)
        base["cond_aug"] = s.cond_aug
        with torch.random.fork_rng(devices=[s._z.device]), torch.no_grad(), model.ema_scope("Sampling"):
            if r == 0:
                t0, cond_frame, mask = 1, s._z, s._first_mask
                base["cond_frames_without_noise"], base["cond_frames"] = s.inputs[:1], s._cond_frames
                conds = [get_condition(model, dict(base, **a), T, sample.UC_KEYS, "cuda") for a in actions]
            else:
                t0, mask = SU.CARRY, s._carry_mask
                base["cond_frames_without_noise"], base["cond_frames"], cond_frame = SU.next_round_inputs(model, s._sample, T, "cuda")
                conds = [SU.next_round_condition(model, dict(base, **a), T, get_condition, sample.UC_KEYS, "cuda") for a in actions]
            noises = []
            for e in range(self.ens_size):
                torch.manual_seed(self.score_seed + r * self.ens_size + e)
                noises.append(torch.randn_like(cond_frame))
            x = torch.empty((len(actions), self.ens_size) + tuple(cond_frame.shape), dtype=torch.float32, device=cond_frame.device)
            for k, (c, uc) in enumerate(conds):
                for e, noise in enumerate(noises):
                    # (the sampler scales its input in place: every candidate gets a copy of the member's noise)
                    if r == 0:
                        x[k, e] = SU.first_round(self.sampler, s._denoiser, c, uc, s._z, mask, lambda like, n=noise: n.clone())
                    else:
                        x[k, e] = self.sampler(s._denoiser, noise.clone(), cond=c, uc=uc, cond_frame=cond_frame, cond_mask=mask)
            return scores_of(x, t0, want_map)

    def step(self, actions):
        """Scores `actions`, then commits session.step(actions[best]) with the session's own sampler and the caller's random stream ->
        (RoundResult, CandidateScores). A round in which no candidate has a number raises a RuntimeError that names it."""
        scores = self.score(actions)
        k = require_best(scores, self.session.rounds)
        return self.session.step(actions[k]), scores


# ---- the candidates file ----------------------------------------------------------------------------------------------------------------------------
def _check_list(entries, where):
    if not isinstance(entries, list):
        raise ValueError(f"{where}: expected a list of entries, got {type(entries).__name__}")
    if not entries:
        raise ValueError(f"{where} is empty; a round chooses among at least one candidate")
    for k, entry in enumerate(entries):
        drive.check_entry(entry, f"{where} candidate {k}")
    return entries


def parse_candidates(obj):
    """The parsed JSON of a candidates file -> ("candidates", [entry, ...]): one list for every round, or ("rounds", [[entry, ...], ...]): a
    list per round. Every entry is checked (drive.check_entry), and refused with its round and candidate index."""
    if not isinstance(obj, dict) or len(obj) != 1 or next(iter(obj)) not in ("candidates", "rounds"):
        raise ValueError("candidates: expected an object with the one key \"candidates\" (a list of entries, the same for every round) or "
                         f"\"rounds\" (one list per round), got {sorted(obj) if isinstance(obj, dict) else type(obj).__name__}")
    if "candidates" in obj:
        return "candidates", _check_list(obj["candidates"], "candidates (every round)")
    rounds = obj["rounds"]
    if not isinstance(rounds, list) or not rounds:
        raise ValueError("candidates: \"rounds\" is empty; a rollout has at least one round")
    return "rounds", [_check_list(entries, f"candidates round {r}") for r, entries in enumerate(rounds)]


def load_candidates(path):
    with open(path, "r") as f:
        return parse_candidates(json.load(f))


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------------
def parse_args(**parser_kwargs):
    parser = sample.parse_args(**parser_kwargs)
    add = parser.add_argument
    add("--hud", action="store_true", help="also write hud/videos: the predicted frames with every round's command drawn in")
    add("--candidates", type=str, default=None, metavar="FILE", help="JSON file with the candidate actions ({\"candidates\": [...]}: the same list "
        "before every round, or {\"rounds\": [[...], ...]}: a list per round)")
    add("--ens_size", type=int, default=5, help="ensemble members per candidate")
    add("--score_steps", type=int, default=10, help="sampling steps of a scoring run")
    add("--score_seed", type=int, default=0, help="member e of round r draws its noise under seed score_seed + r * ens_size + e")
    return parser


def n_rounds_given(argv):
    """Whether the command line names --n_rounds (under any abbreviation argparse accepts), and its value."""
    return frontdoor.n_rounds_given(parse_args, argv)


def plan_run(opt, argv=None, net_params=None):
    """Refuses, by name and before any model is built, what a planned run cannot do -> every round's list of candidate entries."""
    if opt.candidates is None:
        raise ValueError("--candidates FILE is required: the planner chooses among the actions it lists (vista_amd.drive steps a given script)")
    kind, lists = load_candidates(opt.candidates)
    if kind == "rounds":
        given = n_rounds_given(argv)
        if given is not None and given != len(lists):
            raise ValueError(f"--n_rounds {given} disagrees with --candidates {opt.candidates}, which lists {len(lists)} rounds (leave --n_rounds "
                             "out: the file's length decides)")
        rounds = lists
    else:
        if opt.n_rounds < 1:
            raise ValueError(f"--n_rounds {opt.n_rounds}: a rollout has at least one round")
        rounds = [lists] * opt.n_rounds
    try:
        check_ensemble(opt.ens_size, opt.score_steps)
    except ValueError as e:
        raise ValueError("--" + str(e)) from None
    frontdoor.check_world("plan", "neither a frame-sharded session nor members over ranks are built")
    SU.check_sizes(opt.height, opt.width, opt.n_frames, len(rounds), opt.n_conds, net_params)
    SU.sampler_name()   # (a bad VISTA_SAMPLER is refused by name, here)
    SU.video_format()   # (and a bad VISTA_VIDEO or VISTA_VIDEO_QUALITY)
    SU.png_format()     # (and a bad VISTA_PNG)
    return rounds


def unsupplied(action_mode, scene_action):
    """Why a "scene" entry is no candidate for this scene, or None: get_sample returns an EMPTY dict where the annotation lacks what
    `action_mode` names (no CAN bus record, a goal outside the frame); None (a dataset without annotations, --action free) runs action-free."""
    from .reward import _WHY_EMPTY
    if action_mode == "free" or scene_action is None or scene_action:
        return None
    return _WHY_EMPTY.get(action_mode, "the scene's annotation does not supply this action")


def round_extra(entries, live, scores, reason):
    """What a round adds to its record: `entries` the round's candidates as given, `live` the indices of those that were scored (in score
    order), `reason` why the others ("scene" entries the annotation cannot supply) were not."""
    row = {k: i for i, k in enumerate(live)}
    candidates = []
    for k, entry in enumerate(entries):
        if k not in row:
            candidates.append({"action": entry, "reward": None, "reason": reason})
            continue
        i = row[k]
        # (the record is strict JSON: a candidate whose ensemble went non-finite reports null)
        candidates.append({"action": entry, "reward": json_number(scores.reward[i]), "mean_variance": json_number(scores.mean_variance[i]),
                           "frame_variance": [json_number(v) for v in scores.frame_variance[i]]})
    return {"candidates": candidates, "chosen": live[scores.best]}


def plan_rounds(opt, session, rounds, scene_action, timings, where):
    """drive._drive_loop's round stepping for a planned run: before every round its live candidates are scored, the best is stepped."""
    import torch
    planner = Planner(session, ens_size=opt.ens_size, score_steps=opt.score_steps, score_seed=opt.score_seed)
    reason = unsupplied(opt.action, scene_action)
    chosen, extras, spent = [], [], 0.0
    for r, entries in enumerate(rounds):
        live = [k for k, e in enumerate(entries) if not (e == "scene" and reason)]
        if not live:
            raise RuntimeError(f"plan: round {r} of {where}: no candidate is left ({len(entries)} \"scene\" entries, and {reason})")
        actions = [drive.entry_action(entries[k], scene_action) for k in live]
        torch.cuda.synchronize()
        t = time.perf_counter()
        scores = planner.score(actions)
        torch.cuda.synchronize()
        spent += time.perf_counter() - t
        best = require_best(scores, r, where)
        session.step(actions[best])
        chosen.append(entries[live[best]])
        extras.append(round_extra(entries, live, scores, reason))
    timings["score"] = spent
    return chosen, extras


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    opt, _unknown = parse_args(prog="python -m vista_amd.plan").parse_known_args(argv)
    # what cannot run is refused here, before 2.5 billion parameters are built
    rounds = plan_run(opt, argv, frontdoor.net_params(opt))
    return drive._drive_loop(opt, rounds, step_rounds=functools.partial(plan_rounds, opt), records_name=RECORDS_NAME, label="plan")


if __name__ == "__main__":
    sys.exit(main())
