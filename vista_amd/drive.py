"""`python -m vista_amd.drive`: a rollout you can steer -- every sampling round takes an action of its own, and the video shows what was commanded.

`vista_amd.sample` mirrors the reference: one action dict, built before round 0, conditions every round of a rollout (`--action traj --n_rounds 4`
applies the scene's first 2.3 s of trajectory four times over). Here a rollout is an object that stays open between rounds:

    s = DriveSession(model, frame_list, height=576, width=1024, n_frames=25, n_steps=50)
    s.step({"command": torch.tensor(1)})          # round 0: frames [0, 25)
    s.step({"trajectory": torch.tensor([...])})   # round 1: frames [25, 47)
    b = s.fork()                                  # an independent branch from here
    s.frames(), s.samples_z, s.inputs             # what sample.run returns, for the rounds stepped so far

The rounds are do_sample's own (sample_utils.first_round / next_round): a session stepped R times with one action dict under one seed returns
bit for bit what sample.run(..., n_rounds=R) returns (R >= 2 with the default guider, R = 1 with guider="VanillaCFG").

The CLI takes every flag of `vista_amd.sample` under its name with its default (the parser is built from sample.parse_args); on top: --script FILE
(the rounds' actions as JSON) and --hud (a second video with every round's command drawn over the predicted frames, vk_stroke_overlay_u8).

    python -m vista_amd.drive --ckpt ckpts/vista.safetensors --action traj --script turn_left.json --hud --save outputs

    {"rounds": [{"command": 1},
                {"trajectory": [[0.5, 0.0], [1.0, 0.0], [1.5, 0.1], [2.0, 0.2]]},
                {"speed": [3.0, 3.5, 4.0, 4.0], "angle": [0.0, 39.0, 78.0, 78.0]},
                {"goal": [800, 450]},
                {},
                "scene"]}

Values are in the annotation file's own units and are scaled exactly as get_sample scales them (the trajectory flattened to 8 numbers,
angle / 780, goal / (1600, 900)); any combination of keys may share a round, {} is action-free, "scene" is the scene's annotated action under
--action (get_sample's dict). Without --script every round is "scene" and the run equals vista_amd.sample's. Files: <save>/{virtual,real}/
{images,grids,videos} under perform_save_locally's names, <save>/drive.jsonl (one line per scene: index, frames, seed, action, n_rounds, per round
{"round", "action" as given, "frames": [lo, hi]}, timings) and, with --hud, <save>/hud/videos. The plain frames are always written unmodified.

Choosing the actions by reward is vista_amd.plan's (a Planner over a DriveSession). Not built: several GPUs (WORLD_SIZE > 1 is refused by name).
"""
import collections
import json
import math
import os
import sys
import time

from . import frontdoor, sample
from . import sample_utils as SU
from .evaluate import frame_round   # (the round that produced frame i of a rollout)

ACTION_LENGTHS = {"command": 1, "trajectory": 4, "speed": 4, "angle": 4, "goal": 2}   # trajectory: 4 (forward, left) pairs
RECORDS_NAME = "drive.jsonl"
RECORD_KEYS = ("index", "frames", "seed", "action", "n_rounds", "rounds", "timings")
RoundResult = collections.namedtuple("RoundResult", "round lo hi latents action")


def round_range(r, n_frames):
    """The frames [lo, hi) of a rollout that round r contributes: round 0 the whole first window, every later one n_frames - 3 new frames."""
    if r == 0:
        return 0, n_frames
    lo = r * (n_frames - SU.CARRY) + SU.CARRY
    return lo, lo + n_frames - SU.CARRY


# ---- the script -----------------------------------------------------------------------------------------------------------------------------------
def _is_finite_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_entry(entry, where="script entry"):
    """Refuses, by name, a script entry that is not "scene" or a dict of command / trajectory / speed / angle / goal in their annotated shapes."""
    if entry == "scene":
        return
    if not isinstance(entry, dict):
        raise ValueError(f"{where}: expected an object of action keys or the string \"scene\", got {entry!r}")
    for key, value in entry.items():
        if key not in ACTION_LENGTHS:
            raise ValueError(f"{where}: unknown key {key!r} (known: {', '.join(ACTION_LENGTHS)})")
        if key == "command":
            if not isinstance(value, int) or isinstance(value, bool):
                raise ValueError(f"{where}: command must be one integer, got {value!r}")
        elif key == "trajectory":
            if not (isinstance(value, list) and len(value) == 4 and all(isinstance(p, list) and len(p) == 2 and all(_is_finite_number(x) for x in p) for p in value)):
                raise ValueError(f"{where}: trajectory must be 4 [forward, left] pairs of numbers, got {value!r}")
        else:
            n = ACTION_LENGTHS[key]
            if not (isinstance(value, list) and len(value) == n and all(_is_finite_number(x) for x in value)):
                raise ValueError(f"{where}: {key} must be {n} numbers, got {value!r}")
            if key == "goal" and not (0 < value[0] < 1600 and 0 < value[1] < 900):
                raise ValueError(f"{where}: goal {value!r} lies outside the open 1600 x 900 camera frame")


def parse_script(obj):
    """The parsed JSON of a script -> its list of round entries, every one checked."""
    if not isinstance(obj, dict) or set(obj) != {"rounds"}:
        raise ValueError(f"script: expected an object with the one key \"rounds\", got {sorted(obj) if isinstance(obj, dict) else type(obj).__name__}")
    rounds = obj["rounds"]
    if not isinstance(rounds, list) or not rounds:
        raise ValueError("script: \"rounds\" is empty; a rollout has at least one round")
    for r, entry in enumerate(rounds):
        check_entry(entry, f"script round {r}")
    return rounds


def load_script(path):
    with open(path, "r") as f:
        return parse_script(json.load(f))


def entry_action(entry, scene_action=None):
    """A script entry -> the action dict of tensors the conditioner takes, scaled as get_sample scales an annotation's numbers (pipeline.py).
    "scene" -> the scene's own dict (None becomes {})."""
    import torch
    check_entry(entry)
    if entry == "scene":
        return dict(scene_action or {})
    action = {}
    for key, value in entry.items():
        if key == "trajectory":
            action[key] = torch.tensor([x for pair in value for x in pair])
        elif key == "angle":
            action[key] = torch.tensor(value) / 780
        elif key == "goal":
            action[key] = torch.tensor([value[0] / 1600, value[1] / 900])
        else:
            action[key] = torch.tensor(value)
    return action


# ---- the session ----------------------------------------------------------------------------------------------------------------------------------
class DriveSession:
    """A rollout held open between rounds. Construction does what sample.run does before do_sample (load and resize the pictures, draw the
    cond_aug noise, build the sampler) and encodes the pictures; `step(action)` samples one round. Noise comes from torch's global generator at
    step time, in do_sample's order; that the pictures are encoded before round 0's conditioning instead of after it changes nothing as long
    as the conditioner draws nothing from the generator (the shipped one encodes with the posterior's mode). Graph replay and concurrent guidance
    halves are on unless `eager`, as in sample.run. `sampler`: as in sample.run (None = the environment hook VISTA_SAMPLER)."""

    def __init__(self, model, frame_list, *, height=576, width=1024, n_frames=25, n_conds=1, n_steps=50, cfg_scale=2.5, cond_aug=0.0, eager=False,
                 guider="TrianglePredictionGuider", sampler=None):
        import torch
        self.model, self.n_frames, self.cond_aug = model, n_frames, cond_aug
        self.guider, self.cfg_scale = guider, cfg_scale   # (what vista_amd.plan builds its scoring sampler from)
        self.inputs = SU.load_img_seq(frame_list, height, width, "cuda")
        cond_img = self.inputs[:1]
        self._cond_frames = cond_img + cond_aug * torch.randn_like(cond_img)
        self._scalars = SU.init_embedder_options(set(e.input_key for e in model.conditioner.embedders))
        self.sampler_name = SU.sampler_name(sampler)   # (None: the environment hook VISTA_SAMPLER, read once: the session and its forks keep it)
        self.sampler = SU.init_sampling(sampler=self.sampler_name, guider=guider, steps=n_steps, cfg_scale=cfg_scale, num_frames=n_frames)
        self.sampler.graph = self.sampler.cfg_streams = not eager
        self._denoiser = SU.rollout_denoiser(model)
        with torch.no_grad(), model.ema_scope("Sampling"):
            self._z = model.encode_first_stage(self.inputs)
        self._first_mask, self._carry_mask = SU.rollout_masks(n_frames, list(range(n_conds)), "cuda")
        self._sample = None      # the last window
        self._latents = []       # every round's contribution
        self.actions = []        # every round's action dict

    @property
    def rounds(self):
        return len(self._latents)

    @property
    def samples_z(self):
        """Every latent so far: R (n_frames - 3) + 3 frames after R rounds."""
        import torch
        if not self._latents:
            raise RuntimeError("DriveSession.samples_z: no round has been stepped")
        return torch.cat(self._latents)

    def frames(self):
        """The samples in [0, 1]: decode_first_stage(samples_z), clamped as do_sample clamps."""
        import torch
        with torch.no_grad(), self.model.ema_scope("Sampling"):
            samples_x = self.model.decode_first_stage(self.samples_z)
        return torch.clamp((samples_x + 1.0) / 2.0, min=0.0, max=1.0)

    def step(self, action=None):
        """One round under `action` (a dict of command / trajectory / speed / angle / goal tensors as get_sample returns them, or None / {} for an
        action-free round) -> RoundResult(round, lo, hi, latents, action); latents are frames [lo, hi) of the rollout. The round's conditioning
        is built from a fresh dict -- the fixed scalars, the round's conditioning frames, this round's action entries -- so nothing of the
        previous round's action survives."""
        import torch
        action = dict(action or {})
        r = self.rounds
        value_dict = dict(self._scalars)
        value_dict["cond_aug"] = self.cond_aug
        value_dict.update(action)
        get_condition = self.model.condition_fn
        with torch.no_grad(), self.model.ema_scope("Sampling"):
            if r == 0:
                value_dict["cond_frames_without_noise"] = self.inputs[:1]
                value_dict["cond_frames"] = self._cond_frames
                c, uc = get_condition(self.model, value_dict, self.n_frames, sample.UC_KEYS, "cuda")
                self._sample = SU.first_round(self.sampler, self._denoiser, c, uc, self._z, self._first_mask, torch.randn_like)
                latents = self._sample
            else:
                self._sample = SU.next_round(self.model, self.sampler, self._denoiser, value_dict, self._sample, self.n_frames, self._carry_mask,
                                             get_condition, sample.UC_KEYS, "cuda", torch.randn_like)
                latents = self._sample[SU.CARRY:]
        self._latents.append(latents)
        self.actions.append(action)
        lo, hi = round_range(r, self.n_frames)
        return RoundResult(r, lo, hi, latents, action)

    def fork(self):
        """An independent branch from here: the session's tensors are cloned; the model, the sampler with its captured graphs and torch's global
        generator are shared. Both branches draw from that one generator, so two branches compare only after a reseed (torch.manual_seed before
        each branch's step)."""
        b = object.__new__(DriveSession)
        b.__dict__.update(self.__dict__)
        b.inputs, b._cond_frames, b._z = self.inputs.clone(), self._cond_frames.clone(), self._z.clone()
        b._sample = None if self._sample is None else self._sample.clone()
        b._latents = [t.clone() for t in self._latents]
        b.actions = [dict(a) for a in self.actions]
        return b


# ---- the head-up display --------------------------------------------------------------------------------------------------------------------------
# one colour scale and one geometry per run: constants, no per-round autoscale
HUD_FORWARD_M, HUD_LATERAL_M = 40.0, 20.0    # what the trajectory inset spans: 0 .. 40 m ahead, 20 m to either side
HUD_SPEED_MAX = 20.0                         # full scale of the speed sparkline, in the annotation's units
HUD_COLOURS = {"goal": (255.0, 64.0, 32.0), "trajectory": (64.0, 255.0, 96.0), "slots": (255.0, 255.0, 255.0), "command": (255.0, 208.0, 0.0),
               "speed": (64.0, 192.0, 255.0), "angle": (255.0, 96.0, 224.0)}
HUD_MAX_STROKES, HUD_MAX_SEGMENTS = 6, 16    # what one round draws at most


def _values(v):
    return [float(x) for x in (v.reshape(-1).tolist() if hasattr(v, "reshape") else (v if isinstance(v, (list, tuple)) else [v]))]


def hud_strokes(action, H, W):
    """One round's action dict (as the conditioner takes it: get_sample's scaling) -> the list of strokes (colour, alpha, r, segments) that shows
    it on an H x W frame; a pure host function, the same strokes for the same action. {} gives no strokes.
      goal        a disc at its image position (goal x W, goal y H)
      trajectory  a polyline from the ego position through the four waypoints in a top-down inset at the bottom left. ASSUMPTION: the first
                  coordinate of a waypoint is plotted upward (forward) and the second to the left -- the nuScenes ego frame; the reference
                  does not document the trajectory's axes
      command     four slots at the top centre, the commanded one highlighted
      speed, angle  two four-point sparklines at the bottom right (speed against HUD_SPEED_MAX, angle / 780 against +-1)
    Every stroke stays inside the frame, and a round takes at most HUD_MAX_STROKES strokes and HUD_MAX_SEGMENTS segments."""
    action = action or {}
    if not action:
        return []
    u = min(H, W) / 64.0                     # the unit every size is a multiple of
    r = max(0.5, 0.6 * u)
    margin = 2.0 * u + r + 0.5

    def clip(x, y):
        return (min(max(x, min(margin, W / 2.0)), max(W - margin, W / 2.0)), min(max(y, min(margin, H / 2.0)), max(H - margin, H / 2.0)))

    def polyline(points):
        points = [clip(*p) for p in points]
        return [(a[0], a[1], b[0], b[1]) for a, b in zip(points, points[1:])]

    def disc(x, y):
        x, y = clip(x, y)
        return (x, y, x, y)
    side = 18.0 * u
    strokes = []
    if "goal" in action:
        gx, gy = _values(action["goal"])[:2]
        strokes.append((HUD_COLOURS["goal"], 0.9, 2.0 * u, [disc(gx * W, gy * H)]))
    if "trajectory" in action:
        t = _values(action["trajectory"])[:8]
        x0, y0 = margin + side / 2.0, H - margin                     # the ego position: bottom centre of the inset
        pts = [(x0, y0)] + [(x0 - min(max(t[i + 1] / HUD_LATERAL_M, -1.0), 1.0) * side / 2.0, y0 - min(max(t[i] / HUD_FORWARD_M, 0.0), 1.0) * side)
                            for i in range(0, len(t) - 1, 2)]
        strokes.append((HUD_COLOURS["trajectory"], 0.9, r, polyline(pts)))
    if "command" in action:
        cmd = int(_values(action["command"])[0])
        gap = 4.0 * u
        slots = [(W / 2.0 + (i - 1.5) * gap, margin + u) for i in range(4)]
        strokes.append((HUD_COLOURS["slots"], 0.35, u, [disc(*p) for p in slots]))
        if 0 <= cmd < 4:
            strokes.append((HUD_COLOURS["command"], 0.95, 1.4 * u, [disc(*slots[cmd])]))
    for row, key in enumerate(("speed", "angle")):
        if key in action:
            v = _values(action[key])[:4]
            left, base, height = W - margin - side, H - margin - row * 8.0 * u, 6.0 * u
            if key == "speed":
                level = [min(max(x / HUD_SPEED_MAX, 0.0), 1.0) for x in v]
            else:
                level = [0.5 + 0.5 * min(max(x, -1.0), 1.0) for x in v]
            pts = [(left + side * i / max(1, len(v) - 1), base - height * lv) for i, lv in enumerate(level)]
            strokes.append((HUD_COLOURS[key], 0.9, r, polyline(pts) if len(pts) > 1 else [disc(*pts[0])]))
    return strokes


def draw_hud(frames_u8, actions, n_frames):
    """frames_u8 (n, H, W, 3) uint8 on the GPU, the frames of a rollout whose round r ran under actions[r] -> a new stack with every round's
    HUD drawn over its frames (ops.stroke_overlay). One launch as long as the rounds' strokes fit one plan (four full rounds do); a longer
    rollout is drawn in runs of consecutive rounds, each over its own frames."""
    import torch
    from . import ops
    n, H, W, _ = frames_u8.shape
    out = frames_u8.clone()
    per_round = [hud_strokes(a, H, W) for a in actions]
    limits = (ops.OVERLAY_MAX_SETS, ops.OVERLAY_MAX_STROKES, ops.OVERLAY_MAX_SEGMENTS)
    r = 0
    while r < len(per_round):
        first, sets = r, []
        while r < len(per_round) and all(c <= m for c, m in zip(ops.stroke_counts(sets + [per_round[r]]), limits)):
            sets.append(per_round[r])
            r += 1
        if not sets:
            raise ValueError(f"draw_hud: round {r} alone takes {ops.stroke_counts([per_round[r]])} (sets, strokes, segments), a plan {limits}")
        lo, hi = round_range(first, n_frames)[0], min(n, round_range(r - 1, n_frames)[1])
        if lo >= hi or not any(sets):
            continue
        which = torch.tensor([frame_round(i, n_frames) - first if sets[frame_round(i, n_frames) - first] else -1 for i in range(lo, hi)],
                             dtype=torch.int32, device=out.device)
        ops.stroke_overlay(out[lo:hi], sets, which, out=out[lo:hi])
    return out


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------
def parse_args(**parser_kwargs):
    parser = sample.parse_args(**parser_kwargs)
    add = parser.add_argument
    add("--script", type=str, default=None, metavar="FILE", help="JSON file with the rounds' actions ({\"rounds\": [...]}); default: every round \"scene\"")
    add("--hud", action="store_true", help="also write hud/videos: the predicted frames with every round's command drawn in")
    return parser


def n_rounds_given(argv):
    """Whether the command line names --n_rounds (under any abbreviation argparse accepts), and its value."""
    return frontdoor.n_rounds_given(parse_args, argv)


def plan_run(opt, argv=None, net_params=None):
    """Refuses, by name and before any model is built, what a drive run cannot do -> the list of round entries."""
    if opt.script is not None:
        entries = load_script(opt.script)
        given = n_rounds_given(argv)
        if given is not None and given != len(entries):
            raise ValueError(f"--n_rounds {given} disagrees with --script {opt.script}, which lists {len(entries)} rounds (leave --n_rounds out: "
                             "the script's length decides)")
    else:
        if opt.n_rounds < 1:
            raise ValueError(f"--n_rounds {opt.n_rounds}: a rollout has at least one round")
        entries = ["scene"] * opt.n_rounds
    frontdoor.check_world("drive", "a frame-sharded session is not built")
    SU.check_sizes(opt.height, opt.width, opt.n_frames, len(entries), opt.n_conds, net_params)
    SU.sampler_name()   # (a bad VISTA_SAMPLER is refused by name, here)
    SU.video_format()   # (and a bad VISTA_VIDEO or VISTA_VIDEO_QUALITY)
    SU.png_format()     # (and a bad VISTA_PNG)
    return entries


def make_record(index, frame_list, entries, *, seed, action, n_frames, timings=None):
    """The JSON record of one scene; "action" of a round is the script's entry as given."""
    rounds = [{"round": r, "action": e, "frames": list(round_range(r, n_frames))} for r, e in enumerate(entries)]
    return {"index": int(index), "frames": [frame_list[0]], "seed": int(seed), "action": str(action), "n_rounds": len(entries), "rounds": rounds,
            "timings": frontdoor.rounded_timings(timings)}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    opt, _unknown = parse_args(prog="python -m vista_amd.drive").parse_known_args(argv)
    # what cannot run is refused here, before 2.5 billion parameters are built
    entries = plan_run(opt, argv, frontdoor.net_params(opt))
    return _drive_loop(opt, entries)


def _step_entries(session, entries, scene_action, timings, where):
    """The rounds of a drive run: one step per script entry -> (the entries the record lists, nothing to add to its rounds)."""
    for entry in entries:
        session.step(entry_action(entry, scene_action))
    return entries, None


def _drive_loop(opt, entries, step_rounds=_step_entries, records_name=RECORDS_NAME, label="drive"):
    """The loop of vista_amd.sample with a DriveSession in place of do_sample. `step_rounds(session, entries, scene_action, timings, where)` steps
    the session len(entries) times and returns (the entry every round ran under, one dict per round to merge into the record's rounds, or
    None); vista_amd.plan passes its own, which scores a list of candidates before every step, and writes plan.jsonl."""
    import torch
    from . import ops
    model = frontdoor.build_model(opt)
    frontdoor.start_records(opt.save, records_name)   # the file describes this run only

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    for frame_list, sample_index, _dataset_length, scene_action in frontdoor.walk(opt):
        timings = {}
        t0 = clock()
        session = DriveSession(model, frame_list, height=opt.height, width=opt.width, n_frames=opt.n_frames, n_conds=opt.n_conds,
                               n_steps=opt.n_steps, cfg_scale=opt.cfg_scale, cond_aug=opt.cond_aug, eager=opt.eager,
                               guider="TrianglePredictionGuider" if len(entries) > 1 else "VanillaCFG")
        t1 = clock()
        stepped, extras = step_rounds(session, entries, scene_action, timings, f"{opt.dataset} scene {sample_index}")
        t2 = clock()
        samples, inputs = session.frames(), session.inputs
        t3 = clock()
        timings.update(load=t1 - t0, sample=t2 - t1 - timings.get("score", 0.0), decode=t3 - t2)
        frontdoor.save_pictures(opt.save, opt.dataset, sample_index, virtual=samples, real=inputs)
        t4 = clock()
        timings["save"] = t4 - t3
        if opt.hud:
            hud = draw_hud(ops.frames_to_u8(samples.float()), session.actions, opt.n_frames)
            folder = os.path.join(opt.save, "hud", "videos")
            os.makedirs(folder, exist_ok=True)
            SU.save_video(os.path.join(folder, f"{opt.dataset}_{sample_index:06}"), hud, 10)
            timings["hud"] = clock() - t4
        record = make_record(sample_index, frame_list, stepped, seed=opt.seed, action=opt.action, n_frames=opt.n_frames, timings=timings)
        for round_record, extra in zip(record["rounds"], extras or ()):
            round_record.update(extra)
        frontdoor.append_record(opt.save, records_name, record)
        print(f"{label} {sample_index}: {len(entries)} rounds, " + frontdoor.timings_text(timings), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
