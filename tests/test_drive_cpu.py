"""Host side of the drive front door (vista_amd/drive.py) and the numpy definition of vk_stroke_overlay_u8 (tests/_overlay_ref.py): flags, the
script's parsing and refusals, round ranges, the HUD's strokes, the reference's own known answers, and the header / ctypes / ops agreement.
No GPU. Every comparison is exact."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _overlay_ref as R  # noqa: E402

# the scene of tests/test_frontdoor_cpu.py: five angles, goal 800 / 450
SCENE = {"traj": [0.0, 0.0, 1.0, 0.5, 2.0, 1.0, 3.0, 1.5, 4.0, 2.0], "cmd": 2, "speed": [1.0, 2.0, 3.0, 4.0, 5.0],
         "angle": [0.0, 78.0, -390.0, 780.0, 39.0], "z": 1.5, "goal": [800.0, 450.0]}
ENTRIES = {"traj": {"trajectory": [[1.0, 0.5], [2.0, 1.0], [3.0, 1.5], [4.0, 2.0]]}, "cmd": {"command": 2},
           "steer": {"speed": [2.0, 3.0, 4.0, 5.0], "angle": [78.0, -390.0, 780.0, 39.0]}, "goal": {"goal": [800.0, 450.0]}}


def test_flags_are_samples_plus_script_and_hud():
    from vista_amd import drive, sample
    base = {a.dest: a for a in sample.parse_args()._actions if a.dest != "help"}
    ours = {a.dest: a for a in drive.parse_args()._actions if a.dest != "help"}
    assert set(ours) == set(base) | {"script", "hud"}
    for name, a in base.items():
        b = ours[name]
        assert (b.option_strings, b.default, b.type, b.nargs, b.const) == (a.option_strings, a.default, a.type, a.nargs, a.const), name
    assert ours["script"].default is None and ours["script"].type is str and ours["hud"].default is False and ours["hud"].const is True
    opt = drive.parse_args().parse_args(["--script", "s.json", "--hud", "--rand_gen"])
    assert (opt.script, opt.hud, opt.rand_gen, opt.n_rounds) == ("s.json", True, False, 1)
    assert drive.n_rounds_given([]) is None and drive.n_rounds_given(["--n_rounds", "3"]) == 3 and drive.n_rounds_given(["--n_round=1"]) == 1


@pytest.mark.parametrize("mode", ["traj", "cmd", "steer", "goal"])
def test_a_script_entry_scales_like_get_sample(tmp_path, mode):
    from vista_amd import drive
    from vista_amd import sample_utils as SU
    root = tmp_path / "data"
    root.mkdir()
    (root / "f.jpg").write_bytes(b"x")
    anno = tmp_path / "anno.json"
    anno.write_text(json.dumps([dict(SCENE, frames=["f.jpg"] * 2)]))
    want = SU.get_sample(0, "NUSCENES", 2, mode, data_root=str(root), anno_file=str(anno))[3]
    got = drive.entry_action(json.loads(json.dumps(ENTRIES[mode])))
    assert list(got) == list(want) and want
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and torch.equal(got[key], want[key]), key
    assert drive.entry_action("scene", want) == want and drive.entry_action("scene", None) == {} and drive.entry_action({}) == {}
    both = drive.entry_action({**ENTRIES["cmd"], **ENTRIES["goal"]})
    assert list(both) == ["command", "goal"], "any combination of keys may share a round"


BAD_ENTRIES = [
    ({"steer": [1, 2, 3, 4]}, "unknown key 'steer'"),
    ({"trajectory": [[0.5, 0.0], [1.0, 0.0], [1.5, 0.1]]}, "trajectory must be 4"),
    ({"trajectory": [0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2]}, "trajectory must be 4"),
    ({"speed": [1.0, 2.0, 3.0]}, "speed must be 4 numbers"),
    ({"angle": [1.0, 2.0, 3.0, 4.0, 5.0]}, "angle must be 4 numbers"),
    ({"goal": [800.0]}, "goal must be 2 numbers"),
    ({"command": [1]}, "command must be one integer"),
    ({"command": 1.5}, "command must be one integer"),
    ({"goal": [1600, 450]}, "outside the open 1600 x 900"),
    ({"goal": [800, 0]}, "outside the open 1600 x 900"),
    ({"goal": [-3, 450]}, "outside the open 1600 x 900"),
    ("free", "expected an object of action keys"),
]


@pytest.mark.parametrize("entry,message", BAD_ENTRIES, ids=[m for _, m in BAD_ENTRIES])
def test_a_bad_script_entry_is_refused_by_name(entry, message):
    from vista_amd import drive
    with pytest.raises(ValueError, match=re.escape(message)):
        drive.parse_script({"rounds": [{}, entry]})
    with pytest.raises(ValueError, match="script round 1"):
        drive.parse_script({"rounds": [{}, entry]})


def test_cli_refuses_before_any_model_is_built(tmp_path, monkeypatch):
    from vista_amd import drive
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused run"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def script(obj):
        path = tmp_path / f"s{len(os.listdir(tmp_path))}.json"
        path.write_text(json.dumps(obj))
        return str(path)
    three = script({"rounds": [{"command": 1}, {}, "scene"]})
    with pytest.raises(ValueError, match="\"rounds\" is empty"):
        drive.main(["--script", script({"rounds": []})])
    with pytest.raises(ValueError, match="the one key \"rounds\""):
        drive.main(["--script", script({"rounds": [{}], "fps": 10})])
    with pytest.raises(ValueError, match="unknown key 'brake'"):
        drive.main(["--script", script({"rounds": [{"brake": 1}]})])
    with pytest.raises(ValueError, match="--n_rounds 2 disagrees with --script .* 3 rounds"):
        drive.main(["--script", three, "--n_rounds", "2"])
    with pytest.raises(ValueError, match="carries 3 frames"):                      # what check_sizes refuses, for the script's round count
        drive.main(["--script", three, "--n_frames", "3"])
    with pytest.raises(ValueError, match="attention level"):
        drive.main(["--script", three, "--height", "576", "--width", "1088"])
    with pytest.raises(ValueError, match="n_frames 40"):
        drive.main(["--n_frames", "40"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE 2: vista_amd.drive runs on one GPU"):
        drive.main(["--script", three, "--n_rounds", "3"])
    monkeypatch.delenv("WORLD_SIZE")
    opt = drive.parse_args().parse_args(["--script", three, "--n_rounds", "3", "--n_frames", "5", "--height", "128", "--width", "256"])
    assert drive.plan_run(opt, ["--script", three, "--n_rounds", "3"]) == [{"command": 1}, {}, "scene"]
    opt = drive.parse_args().parse_args(["--n_rounds", "2"])
    assert drive.plan_run(opt, ["--n_rounds", "2"]) == ["scene", "scene"], "without --script every round is the scene's action"


@pytest.mark.parametrize("T", [5, 25])
def test_round_frame_ranges(T):
    from vista_amd import drive
    ranges = [drive.round_range(r, T) for r in range(4)]
    assert ranges[0] == (0, T) and ranges[1:] == [(r * (T - 3) + 3, r * (T - 3) + T) for r in (1, 2, 3)]
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] == 4 * (T - 3) + 3
    for r, (lo, hi) in enumerate(ranges):
        assert all(drive.frame_round(i, T) == r for i in range(lo, hi))
    rec = drive.make_record(7, ["a.jpg", "b.jpg"], [{"command": 1}, "scene"], seed=23, action="traj", n_frames=T, timings={"load": 0.12345678})
    assert tuple(rec) == drive.RECORD_KEYS and rec["frames"] == ["a.jpg"] and rec["n_rounds"] == 2 and rec["timings"] == {"load": 0.1235}
    assert rec["rounds"] == [{"round": 0, "action": {"command": 1}, "frames": [0, T]}, {"round": 1, "action": "scene", "frames": [T, 2 * T - 3]}]


FULL_ACTION = {"goal": torch.tensor([0.5, 0.5]), "trajectory": torch.tensor([1.0, 0.5, 2.0, 1.0, 3.0, 1.5, 4.0, 2.0]), "command": torch.tensor(2),
               "speed": torch.tensor([2.0, 3.0, 4.0, 5.0]), "angle": torch.tensor([0.1, -0.5, 1.0, 0.05])}
WILD_ACTION = {"goal": torch.tensor([0.999, 0.001]), "trajectory": torch.tensor([500.0, -90.0, -3.0, 80.0, 1e6, 1e6, 0.0, 0.0]), "command": torch.tensor(9),
               "speed": torch.tensor([-5.0, 1e9, 0.0, 20.0]), "angle": torch.tensor([-7.0, 7.0, 0.0, 1.0])}


@pytest.mark.parametrize("H,W", [(576, 1024), (128, 256), (320, 576), (64, 64)])
def test_hud_strokes_are_deterministic_bounded_and_fit_a_plan(H, W):
    from vista_amd import drive, ops
    assert drive.hud_strokes({}, H, W) == [] and drive.hud_strokes(None, H, W) == []
    for action in (FULL_ACTION, WILD_ACTION, {k: v.tolist() for k, v in FULL_ACTION.items()}):
        strokes = drive.hud_strokes(action, H, W)
        assert strokes == drive.hud_strokes(dict(action), H, W) and strokes
        n_seg = sum(len(s[3]) for s in strokes)
        assert len(strokes) <= drive.HUD_MAX_STROKES and n_seg <= drive.HUD_MAX_SEGMENTS
        for colour, alpha, r, segments in strokes:
            assert len(colour) == 3 and all(0.0 <= c <= 255.0 for c in colour) and 0.0 <= alpha <= 1.0 and r >= 0.0 and segments
            for ax, ay, bx, by in segments:   # the whole round-capped stroke, anti-aliasing fringe included, lies inside the frame
                assert r + 0.5 <= min(ax, bx) and max(ax, bx) <= W - r - 0.5 and r + 0.5 <= min(ay, by) and max(ay, by) <= H - r - 0.5
    assert len(drive.hud_strokes(FULL_ACTION, H, W)) == 6 and len(drive.hud_strokes(WILD_ACTION, H, W)) == 5, "command 9 highlights no slot"
    assert [len(drive.hud_strokes({k: FULL_ACTION[k]}, H, W)) for k in ("goal", "trajectory", "command", "speed", "angle")] == [1, 1, 2, 1, 1]
    # one launch holds four full rounds
    assert ops.stroke_counts([drive.hud_strokes(FULL_ACTION, H, W)] * 4) <= (ops.OVERLAY_MAX_SETS, ops.OVERLAY_MAX_STROKES, ops.OVERLAY_MAX_SEGMENTS)
    assert 4 * drive.HUD_MAX_STROKES <= ops.OVERLAY_MAX_STROKES and 4 * drive.HUD_MAX_SEGMENTS <= ops.OVERLAY_MAX_SEGMENTS


# ---- the numpy reference itself -------------------------------------------------------------------------------------------------------------------
def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def test_reference_alpha_zero_and_empty_strokes_are_the_identity():
    frame = _noise(19, 23, 0)
    assert np.array_equal(R.draw(frame, [((255.0, 0.0, 9.0), 0.0, 3.0, [(2.0, 2.0, 20.0, 15.0)])]), frame)
    assert np.array_equal(R.draw(frame, []), frame) and np.array_equal(R.draw(frame, [((1.0, 2.0, 3.0), 1.0, 2.0, [])]), frame)
    frames = np.stack([frame, frame[::-1].copy()])
    sets = [[((0.0, 0.0, 0.0), 1.0, 1.0, [(5.0, 5.0, 5.0, 5.0)])]]
    out = R.overlay(frames, sets, [-1, 0])
    assert np.array_equal(out[0], frames[0]) and not np.array_equal(out[1], frames[1]) and np.array_equal(R.overlay(frames, sets, [1, 7]), frames)


def test_reference_horizontal_stroke_changes_the_expected_rows_by_the_expected_amounts():
    H, W, r = 16, 24, 2.0
    frame = np.full((H, W, 3), 100, dtype=np.uint8)
    # the axis y = 8 runs between the centres of rows 7 and 8 and reaches far past both borders: row y lies |y + 0.5 - 8| from it
    out = R.draw(frame, [((200.0, 0.0, 100.0), 0.5, r, [(-50.0, 8.0, 80.0, 8.0)])])
    for y in range(H):
        cov = min(max(r + 0.5 - abs(y + 0.5 - 8.0), 0.0), 1.0)     # rows 6 .. 9: 1, rows 5 and 10: 0.0 at distance 2.5, the rest 0
        want = [int(100 + 0.5 * cov * (k - 100)) for k in (200.0, 0.0, 100.0)]
        assert (out[y] == np.array(want, dtype=np.uint8)).all(), (y, out[y, 0], want)
    assert (out[6:10, :, 0] == 150).all() and (out[6:10, :, 1] == 50).all() and (out[:6] == 100).all() and (out[10:] == 100).all()
    # a half-covered row: the axis at y = 8.25 leaves row 5 at distance 2.75 (nothing) and row 10 at 2.25 (coverage 0.25)
    out = R.draw(frame, [((200.0, 0.0, 100.0), 1.0, r, [(-50.0, 8.25, 80.0, 8.25)])])
    assert (out[10, :, 0] == 125).all() and (out[10, :, 1] == 75).all() and (out[5] == 100).all() and (out[11] == 100).all()


def test_reference_polyline_joint_is_no_darker_than_its_body():
    frame = np.full((40, 40, 3), 255, dtype=np.uint8)
    stroke = ((0.0, 0.0, 0.0), 0.5, 2.0, [(5.0, 20.5, 20.5, 20.5), (20.5, 20.5, 20.5, 35.0)])
    out = R.draw(frame, [stroke])
    body = int(out[20, 10, 0])                          # on the first segment's axis, far from the joint
    assert body == 127 and int(out[30, 20, 0]) == body  # ... and on the second's
    assert int(out[20, 20, 0]) == body, "the joint's pixel is covered by both segments: the maximum, not two blends"
    assert out.min() == body
    twice = R.draw(frame, [stroke[:3] + (stroke[3][:1],), stroke[:3] + (stroke[3][1:],)])
    assert int(twice[20, 20, 0]) < body, "two strokes do blend twice there"
    assert np.array_equal(R.draw(frame, [stroke[:3] + (stroke[3][::-1],)]), out), "the order of a stroke's segments does not matter"


def test_header_signature_table_and_ops_agree_on_the_new_entry():
    from vista_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    decl = re.search(r"^int vk_stroke_overlay_u8\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ["const void*", "void*", "const int32_t*", "const VkStrokePlan*", "int32_t", "int32_t", "int32_t", "void*"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["vk_stroke_overlay_u8"] == [vp, vp, vp, ctypes.POINTER(_lib.VkStrokePlan), i32, i32, i32, vp]
    maxima = {k: int(v) for k, v in re.findall(r"#define VK_OVERLAY_MAX_(\w+) (\d+)", hdr)}
    assert maxima == {"SETS": _lib.VK_OVERLAY_MAX_SETS, "STROKES": _lib.VK_OVERLAY_MAX_STROKES, "SEGMENTS": _lib.VK_OVERLAY_MAX_SEGMENTS}
    assert (ops.OVERLAY_MAX_SETS, ops.OVERLAY_MAX_STROKES, ops.OVERLAY_MAX_SEGMENTS) == (maxima["SETS"], maxima["STROKES"], maxima["SEGMENTS"])
    for name, cls in (("VkStrokeSegment", _lib.VkStrokeSegment), ("VkStroke", _lib.VkStroke), ("VkStrokeSet", _lib.VkStrokeSet), ("VkStrokePlan", _lib.VkStrokePlan)):
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)].split("{", 1)[1]
        names = [n.strip().split("[")[0] for d in body.split(";") if d.strip() for n in d.strip().split(" ", 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], (name, names)
    assert ctypes.sizeof(_lib.VkStrokePlan) == 16 + 8 * maxima["SETS"] + 28 * maxima["STROKES"] + 20 * maxima["SEGMENTS"]
    assert _lib.ABI_VERSION == 9, "the entry is additive"
    assert os.path.exists(_lib.LIB_PATH) and hasattr(ctypes.CDLL(_lib.LIB_PATH), "vk_stroke_overlay_u8")
    assert "overlay.hip" in __import__("vista_amd.build", fromlist=["SOURCES"]).SOURCES
    # the plan ops builds: runs, counts, and inv_len2 as the reference forms it
    sets = [[((1.0, 2.0, 3.0), 0.5, 1.5, [(0.0, 0.0, 3.0, 4.0), (2.0, 2.0, 2.0, 2.0)])], [], [((9.0, 8.0, 7.0), 1.0, 0.0, [(1.0, 1.0, 1.0, 8.0)])]]
    plan = ops.stroke_plan(sets)
    assert (plan.n_sets, plan.n_strokes, plan.n_segments) == ops.stroke_counts(sets) == (3, 2, 3)
    assert [(s.stroke_begin, s.stroke_count) for s in plan.set[:3]] == [(0, 1), (1, 0), (1, 1)]
    assert [(s.seg_begin, s.seg_count, s.alpha, s.r, list(s.color)) for s in plan.stroke[:2]] == [(0, 2, 0.5, 1.5, [1.0, 2.0, 3.0]), (2, 1, 1.0, 0.0, [9.0, 8.0, 7.0])]
    assert [g.inv_len2 for g in plan.seg[:3]] == [float(R.inv_len2(0, 0, 3, 4)), 0.0, float(R.inv_len2(1, 1, 1, 8))] == [float(np.float32(1) / np.float32(25)), 0.0, float(np.float32(1) / np.float32(49))]
    with pytest.raises((TypeError, _lib.VistaHipError)):
        ops.stroke_overlay(torch.zeros(1, 4, 4, 3), [], [-1])
