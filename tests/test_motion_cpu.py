"""Motion scores without a GPU: the numpy restatement of the block-matching flow (tests/_motion_ref.py) on cases whose answer is known, the
arithmetic from the sums to the scores, the records and the summary with motion=, and the VISTA_EVAL_MOTION hook."""
import math
import os
import re

import numpy as np
import pytest

from tests import _motion_ref as R
from tests.test_perceptual_cpu import KW, PARENT_RECORD, _clip_report, _fidelity_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def test_luma_and_pyramid_by_hand():
    frame = np.zeros((1, 32, 32, 3), np.uint8)
    frame[0, 0, 0], frame[0, 0, 1], frame[0, 1, 0], frame[0, 1, 1] = (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)
    l0, l1, l2 = R.pyramid(frame)
    assert (l0.shape, l1.shape, l2.shape) == ((1, 32, 32), (1, 16, 16), (1, 8, 8)) and l0.dtype == l2.dtype == np.uint8
    assert l0[0, :2, :2].tolist() == [[255, 77], [149, 29]], "(77 R + 150 G + 29 B + 128) >> 8; the weights add up to 256"
    assert l1[0, 0, 0] == (255 + 77 + 149 + 29 + 2) >> 2 == 128 and l2[0, 0, 0] == (128 + 2) >> 2 and not l1[0, 1:].any()
    tex = R.texture(64, 96)
    assert tex.shape == (64, 96, 3) and tex.min() == 0 and tex.max() == 255 and R.texture(64, 96) is tex
    a = tex[..., 0].astype(np.float64)
    assert np.corrcoef(a[:, :-1].ravel(), a[:, 1:].ravel())[0, 1] > 0.85, "smooth: neighbours are alike (white noise: about 0)"


@pytest.mark.parametrize("vector", R.TRANSLATIONS, ids=lambda v: "%d_%d" % v)
def test_translation_is_recovered_on_every_interior_block(vector):
    frames = R.translated_pair(vector)
    assert frames.shape == (2, 128, 160, 3)
    vy, vx = vector
    assert np.array_equal(frames[1][40 + vy:48 + vy, 40 + vx:48 + vx], frames[0][40:48, 40:48]), "content at (y, x) is found at (y + vy, x + vx)"
    flow, sad = R.block_flow(frames)
    assert flow.shape == sad.shape == (1, 16, 20, 2) and flow.dtype == np.int16 and sad.dtype == np.uint16
    inside = R.interior_blocks((128, 160), vector)
    assert inside.sum() >= 96
    assert (flow[0][inside] == vector).all(), f"{int((flow[0][inside] != vector).any(axis=-1).sum())} interior blocks missed {vector}"
    assert not sad[0][inside][:, 0].any(), "an exact match: SAD 0"
    if vector != (0, 0):
        assert sad[0][inside][:, 1].min() > 0, "the SAD at zero displacement is another number"
    else:
        assert not flow.any() and not sad.any()


def test_flat_frames_ties_and_two_populations():
    flow, sad = R.block_flow(np.full((3, 32, 64, 3), 200, np.uint8))
    assert flow.shape == (2, 4, 8, 2) and not flow.any() and not sad.any(), "all candidates tie: the increment 0 wins at every level"
    # a constant change of brightness ties everywhere too, at a SAD that is not zero
    two = np.stack([np.full((32, 32, 3), 10, np.uint8), np.full((32, 32, 3), 13, np.uint8)])
    flow, sad = R.block_flow(two)
    assert not flow.any() and (sad == 3 * 64).all()
    # the left half moves by (0, 4), the right half by (2, -6)
    flow, sad = R.block_flow(R.split_pair())
    left, right = flow[0, :, :6].reshape(-1, 2), flow[0, :, 10:].reshape(-1, 2)
    assert (left == (0, 4)).all() and (right == (2, -6)).all()
    sums = R.pair_sums(flow, sad)
    assert sums[0, 0] == 8 * 16 and sums[0, 1] == int((flow.astype(np.int64) ** 2).sum()) and sums[0, 4] == 0
    assert R.block_flow(R.split_pair()[:1])[0].shape == (0, 8, 16, 2)


def test_identical_stacks_have_no_end_point_error():
    from vista_amd import motion
    frames = R.translated_pair((3, 5), shape=(64, 96))
    flow, sad = R.block_flow(frames)
    sums = R.pair_sums(flow, sad, flow)
    rep = motion.report_from_sums(sums, 64, 96, R.pair_sums(flow, sad))
    assert rep.epe[1] == 0.0 and np.isnan(rep.epe[0]) and np.array_equal(rep.rms, rep.rms_real, equal_nan=True)
    assert np.array_equal(rep.warp_err, rep.warp_err_real, equal_nan=True) and rep.rms[1] > 0
    still = np.ascontiguousarray(np.stack([frames[0], frames[0]]))
    f0, s0 = R.block_flow(still)
    rep = motion.report_from_sums(R.pair_sums(flow, sad, f0), 64, 96, R.pair_sums(f0, s0))
    assert rep.rms_real[1] == 0.0 and rep.moving_real[1] == 0.0 and rep.epe[1] == rep.rms[1], "against a still clip the error is the motion itself"


# ---- from the sums to the scores --------------------------------------------------------------------------------------------------------------
def test_report_arithmetic_from_hand_made_sums():
    from vista_amd import motion
    assert motion.motion_info() == {"block": 8, "levels": 3, "coarse_range": 7, "refine_range": 2, "reach_px": 30}
    H, W = 32, 64   # 32 blocks, 2048 pixels
    pred = np.array([[16, 32 * 25, 4096, 8192, 32 * 9], [0, 0, 0, 1024, 32 * 4]], np.int64)
    real = np.array([[32, 32 * 4, 2048, 2048, 0], [8, 32, 1024, 3072, 0]], np.int64)
    rep = motion.report_from_sums(pred, H, W, real)
    assert [len(getattr(rep, k)) for k in ("rms", "moving", "warp_err", "diff", "rms_real", "moving_real", "warp_err_real", "diff_real", "epe")] == [3] * 9
    assert all(np.isnan(getattr(rep, k)[0]) for k in ("rms", "moving", "warp_err", "diff", "rms_real", "epe"))
    assert rep.rms[1:].tolist() == [5.0, 0.0] and rep.moving[1:].tolist() == [0.5, 0.0]
    assert rep.warp_err[1:].tolist() == [2.0, 0.0] and rep.diff[1:].tolist() == [4.0, 0.5]
    assert rep.rms_real[1:].tolist() == [2.0, 1.0] and rep.moving_real[1:].tolist() == [1.0, 0.25]
    assert rep.warp_err_real[1:].tolist() == [1.0, 0.5] and rep.diff_real[1:].tolist() == [1.0, 1.5]
    assert rep.epe[1:].tolist() == [3.0, 2.0]
    alone = motion.report_from_sums(pred, H, W)
    assert alone.epe is None and alone.rms_real is None and alone.rms[1:].tolist() == [5.0, 0.0]
    empty = motion.report_from_sums(np.zeros((0, 5), np.int64), H, W, np.zeros((0, 5), np.int64))
    assert empty.rms.shape == (1,) and np.isnan(empty.rms[0]) and np.isnan(empty.epe[0])
    with pytest.raises(ValueError, match="pairs of sums"):
        motion.report_from_sums(pred, H, W, real[:1])
    for bad in ((48, 64), (32, 40), (0, 64)):
        with pytest.raises(ValueError, match="multiples of 32"):
            motion.check_size(*bad)
    motion.check_size(576, 1024)


# ---- records and summary -----------------------------------------------------------------------------------------------------------------------
def _motion_report(n, real=True):
    from vista_amd import motion
    nan = [np.nan]
    rep = motion.MotionReport(rms=np.array(nan + [1.0 + 0.5 * i for i in range(1, n)]), moving=np.array(nan + [0.25] * (n - 1)),
                              warp_err=np.array(nan + [2.0 + 0.125 * i for i in range(1, n)]), diff=np.array(nan + [9.0] * (n - 1)))
    if real:
        rep.rms_real, rep.moving_real = np.array(nan + [2.0] * (n - 1)), np.array(nan + [0.5] * (n - 1))
        rep.warp_err_real, rep.diff_real = np.array(nan + [1.5] * (n - 1)), np.array(nan + [8.0] * (n - 1))
        rep.epe = np.array(nan + [0.5 * i for i in range(1, n)])
    return rep


LISTS = ["flow_rms", "flow_rms_real", "flow_epe", "flow_moving", "warp_err", "warp_err_real"]
MOTION_KEYS = LISTS + ["mean_" + k for k in LISTS]


def test_records_and_summary_without_the_keyword_are_the_parents():
    from vista_amd import evaluate
    rec = evaluate.make_record(4, ["a.png", "b.png"], _fidelity_report(7), motion=None, **KW)
    assert rec == PARENT_RECORD and list(rec) == list(PARENT_RECORD)
    assert evaluate.make_record(4, ["a.png", "b.png"], _fidelity_report(7), clip=None, motion=None, **KW) == PARENT_RECORD
    assert evaluate.summarize([rec], motion=None) == evaluate.summarize([rec]) == evaluate.summarize([rec], clip=None, motion=None)
    assert list(evaluate.summarize([rec], motion=None)) == ["scenes", "mean_psnr", "mean_ssim", "horizon"]
    assert evaluate._summary([rec], None) == evaluate._summary([rec], None, None) == evaluate.summarize([rec])
    assert evaluate._motion_stage(None, None, None, {}) == {}
    assert evaluate._scene_line(rec).startswith("evaluate 4: 7 frames, mean_psnr 33.5000, mean_ssim 0.7188 | load")


def test_records_and_summary_with_the_keyword():
    from vista_amd import evaluate, motion
    rec = evaluate.make_record(4, ["a.png"], _fidelity_report(7), motion=_motion_report(7), **KW)
    assert list(rec) == list(PARENT_RECORD)[:-1] + MOTION_KEYS + ["timings"]
    assert {k: v for k, v in rec.items() if k not in MOTION_KEYS and k != "rounds"} == {k: v for k, v in PARENT_RECORD.items() if k != "rounds"}
    assert all(rec[k][0] is None and len(rec[k]) == 7 for k in LISTS), "no predecessor: null"
    assert rec["flow_rms"][1:] == [1.5, 2.0, 2.5, 3.0, 3.5, 4.0] and rec["flow_epe"][1:] == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    assert rec["mean_flow_rms"] == 2.75 and rec["mean_flow_rms_real"] == 2.0 and rec["mean_flow_epe"] == 1.75 and rec["mean_flow_moving"] == 0.25
    assert rec["mean_warp_err"] == 2.0 + 0.125 * 3.5 and rec["mean_warp_err_real"] == 1.5, "over the predicted frames; the conditioning frame is in none"
    assert [list(r) for r in rec["rounds"]] == [["round", "frames", "mean_psnr", "mean_ssim", "mean_flow_epe"]] * 2
    assert [r["mean_flow_epe"] for r in rec["rounds"]] == [1.25, 2.75]
    assert [{k: v for k, v in r.items() if k != "mean_flow_epe"} for r in rec["rounds"]] == PARENT_RECORD["rounds"]
    assert "mean_ssim 0.7188, mean_flow_epe 1.7500 | load" in evaluate._scene_line(rec)
    # two conditioning frames: frame 1 has a predecessor and a value, and is still in no mean
    two = evaluate.make_record(6, ["d.png"], _fidelity_report(5), motion=_motion_report(5), **{**KW, "n_conds": 2})
    assert two["cond"] == [0, 1] and two["flow_rms"][1] == 1.5 and two["mean_flow_rms"] == (2.0 + 2.5 + 3.0) / 3
    # both keywords: the motion keys after the clip keys, timings last
    both = evaluate.make_record(4, ["a.png"], _fidelity_report(7), clip=_clip_report(7), motion=_motion_report(7), **KW)
    clip_only = evaluate.make_record(4, ["a.png"], _fidelity_report(7), clip=_clip_report(7), **KW)
    assert list(both) == list(clip_only)[:-1] + MOTION_KEYS + ["timings"]
    assert {k: both[k] for k in clip_only if k != "rounds"} == {k: v for k, v in clip_only.items() if k != "rounds"}
    assert list(both["rounds"][0]) == ["round", "frames", "mean_psnr", "mean_ssim", "mean_clip_sim", "mean_flow_epe"]
    assert "mean_clip_sim 0.6094, mean_flow_epe 1.7500 | load" in evaluate._scene_line(both)
    # the summary: means over scenes, three horizon curves, the method's parameters
    short = evaluate.make_record(5, ["c.png"], _fidelity_report(5), motion=_motion_report(5), **KW)
    summary = evaluate.summarize([rec, short], motion=motion.motion_info())
    plain = evaluate.summarize([rec, short])
    assert list(summary) == list(plain) + ["mean_" + k for k in LISTS] + ["motion"]
    assert {k: summary[k] for k in plain if k != "horizon"} == {k: plain[k] for k in plain if k != "horizon"}
    assert list(summary["horizon"]) == list(plain["horizon"]) + ["flow_rms", "flow_rms_real", "flow_epe"]
    assert {k: summary["horizon"][k] for k in plain["horizon"]} == plain["horizon"]
    assert summary["mean_flow_rms"] == (2.75 + 2.25) / 2 and summary["mean_flow_epe"] == (1.75 + 1.25) / 2 and summary["mean_warp_err_real"] == 1.5
    assert summary["horizon"]["flow_rms"] == [None, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0] and summary["horizon"]["flow_rms_real"] == [None] + [2.0] * 6
    assert summary["horizon"]["flow_epe"] == [None, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    assert summary["motion"] == {"block": 8, "levels": 3, "coarse_range": 7, "refine_range": 2, "reach_px": 30}
    with_clip = evaluate.summarize([both], clip={"mmd": None, "tower": {"embed": 1024}}, motion=motion.motion_info())
    assert list(with_clip)[-9:] == ["clip_mmd", "clip"] + ["mean_" + k for k in LISTS] + ["motion"]
    assert list(with_clip["horizon"])[-5:] == ["clip_sim", "clip_step", "flow_rms", "flow_rms_real", "flow_epe"]
    # a report of another length, or one without the real stack, is refused
    with pytest.raises(ValueError, match="holds 5 frames"):
        evaluate.make_record(4, ["a.png"], _fidelity_report(7), motion=_motion_report(5), **KW)
    with pytest.raises(ValueError, match="no real stack"):
        evaluate.make_record(4, ["a.png"], _fidelity_report(7), motion=_motion_report(7, real=False), **KW)


# ---- the hook ----------------------------------------------------------------------------------------------------------------------------------
def test_the_hook_is_read_in_one_place_and_refuses_by_name(monkeypatch):
    from vista_amd import evaluate, pipeline
    from vista_amd import sample_utils as SU
    assert SU.eval_motion is pipeline.eval_motion
    for value, want in ((None, False), ("", False), ("0", False), ("1", True)):
        monkeypatch.delenv("VISTA_EVAL_MOTION", raising=False)
        if value is not None:
            monkeypatch.setenv("VISTA_EVAL_MOTION", value)
        assert SU.eval_motion() is want
    readers = [f for f in os.listdir(os.path.join(ROOT, "vista_amd")) if f.endswith(".py")
               and re.search(r"os\.environ[^\n]*VISTA_EVAL_MOTION", open(os.path.join(ROOT, "vista_amd", f)).read())]
    assert readers == ["pipeline.py"]
    monkeypatch.setattr(SU, "init_model", None)   # (nothing below gets as far as a model)
    for bad in ("2", "yes", "true", " 1"):
        monkeypatch.setenv("VISTA_EVAL_MOTION", bad)
        with pytest.raises(ValueError, match="VISTA_EVAL_MOTION"):
            SU.eval_motion()
        with pytest.raises(ValueError, match=f"Bad value {bad} .environment hook VISTA_EVAL_MOTION."):   # before a model is built
            evaluate.main(["--dataset", "NUSCENES", "--rand_gen", "--n_scenes", "1"])
        with pytest.raises(ValueError, match="VISTA_EVAL_MOTION"):
            evaluate.main(["--compare", "nowhere"])


def test_compare_with_the_hook_refuses_a_picture_size_before_anything_is_scored(monkeypatch, tmp_path):
    from PIL import Image
    from vista_amd import evaluate
    for sub in ("virtual", "real"):
        (tmp_path / sub / "images").mkdir(parents=True)
        for i, size in enumerate(((64, 32), (64, 32), (72, 32))):   # (width, height): the third picture is 72 wide
            Image.fromarray(np.zeros((size[1], size[0], 3), np.uint8)).save(tmp_path / sub / "images" / f"NUSCENES_000000_{i:04}.png")
    monkeypatch.setenv("VISTA_EVAL_MOTION", "1")
    with pytest.raises(ValueError, match=r"NUSCENES_000000_0002.png: 32 x 72 frames: .* multiples of 32"):
        evaluate.main(["--compare", str(tmp_path)])
    assert sorted(os.listdir(tmp_path)) == ["real", "virtual"], "no metrics file was begun"


# ---- the library's table and the wrappers' refusals ----------------------------------------------------------------------------------------------
def test_entry_points_are_declared_listed_and_built():
    import ctypes
    from vista_amd import _lib, build, motion, ops
    assert "flow.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["vk_flow_pyramid_bytes"] == [i32] * 3
    assert _lib.SIGNATURES["vk_flow_luma_pyramid_u8"] == [vp, vp, i32, i32, i32, vp]
    assert _lib.SIGNATURES["vk_block_flow_u8"] == [vp, vp, vp, i32, i32, i32, vp]
    assert _lib.SIGNATURES["vk_flow_pair_sums"] == [vp] * 4 + [i32, i32, vp]
    assert _lib.ABI_VERSION == 9
    for name in ("libvista_hip.so", "libvista_hip_f16.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "vista_amd", "lib", name))
        for fn in ("vk_flow_pyramid_bytes", "vk_flow_luma_pyramid_u8", "vk_block_flow_u8", "vk_flow_pair_sums"):
            assert hasattr(lib, fn) and re.search(rf"^int {fn}\(", hdr, flags=re.M), (name, fn)
    defines = {k: int(v) for k, v in re.findall(r"#define (VK_FLOW_\w+) (\d+)", hdr)}
    assert defines == {"VK_FLOW_BLOCK": ops.FLOW_BLOCK, "VK_FLOW_LEVELS": ops.FLOW_LEVELS, "VK_FLOW_COARSE_RANGE": ops.FLOW_COARSE_RANGE,
                       "VK_FLOW_REFINE_RANGE": ops.FLOW_REFINE_RANGE, "VK_FLOW_MAX_FRAMES": ops.FLOW_MAX_FRAMES, "VK_FLOW_MAX_SIDE": ops.FLOW_MAX_SIDE}
    assert (ops.FLOW_BLOCK, ops.FLOW_LEVELS, ops.FLOW_COARSE_RANGE, ops.FLOW_REFINE_RANGE) == (motion.BLOCK, motion.LEVELS, motion.COARSE_RANGE,
                                                                                              motion.REFINE_RANGE) == (R.BLOCK, R.LEVELS, R.COARSE, R.REFINE)
    lib = _lib.load()
    assert lib.vk_flow_pyramid_bytes(91, 576, 1024) == 91 * 576 * 1024 * 21 // 16 and lib.vk_flow_pyramid_bytes(1, 32, 32) == 1344
    for n, H, W in ((0, 32, 32), (1, 33, 32), (1, 32, 48), (1, 16, 32), (65536, 32, 32), (2048, 1024, 1024)):
        assert lib.vk_flow_pyramid_bytes(n, H, W) == -22, (n, H, W)
    # extents whose product would wrap 64 or 32 bits are refused from the sides alone, by every entry point, with operands that are not NULL
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    for n, H, W in R.WRAPPING_SHAPES:
        assert lib.vk_flow_pyramid_bytes(n, H, W) == -22, (n, H, W)
        assert lib.vk_flow_luma_pyramid_u8(ptr, ptr, n, H, W, None) == -22, (n, H, W)
        assert lib.vk_block_flow_u8(ptr, ptr, ptr, n, H, W, None) == -22, (n, H, W)
        with pytest.raises(ValueError, match="a call"):
            ops.flow_check_shape("x", n, H, W)
    assert lib.vk_flow_pyramid_bytes(1, ops.FLOW_MAX_SIDE, 1536) == ops.FLOW_MAX_SIDE * 1536 * 21 // 16, "the largest side is taken"
    assert lib.vk_flow_pyramid_bytes(1, ops.FLOW_MAX_SIDE + 32, 32) == -22
    # NULL operands and bad shapes come back as -22 before anything is launched (no GPU needed)
    assert lib.vk_flow_luma_pyramid_u8(None, None, 1, 32, 32, None) == -22
    assert lib.vk_block_flow_u8(None, None, None, 2, 32, 32, None) == -22
    assert lib.vk_flow_pair_sums(None, None, None, None, 1, 16, None) == -22


def test_wrappers_refuse_before_the_library_is_asked():
    import torch
    from vista_amd import _lib, motion, ops
    u8 = torch.zeros(2, 32, 64, 3, dtype=torch.uint8)
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.flow_luma_pyramid_u8(u8)
    with pytest.raises(TypeError):
        ops.flow_luma_pyramid_u8(u8.float())
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.block_flow_u8(torch.zeros(2 * 32 * 64 * 21 // 16, dtype=torch.uint8), 2, 32, 64)
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.flow_pair_sums(torch.zeros(1, 4, 8, 2, dtype=torch.int16), torch.zeros(1, 4, 8, 2, dtype=torch.uint16))
    with pytest.raises(TypeError):
        ops.flow_pair_sums(torch.zeros(1, 4, 8, 2, dtype=torch.int32), torch.zeros(1, 4, 8, 2, dtype=torch.uint16))
    with pytest.raises(ValueError, match="multiples of 32"):
        motion.block_flow(torch.zeros(2, 40, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="pair up"):
        motion.clip_motion(u8, u8[:1])
    for bad in (u8[0], u8[..., :2], u8[:0]):
        with pytest.raises(ValueError, match=r"clip_motion: expected an \(n, H, W, 3\)"):
            motion.clip_motion(bad)
        with pytest.raises(ValueError, match=r"block_flow: expected an \(n, H, W, 3\)"):
            motion.block_flow(bad)
    assert math.isnan(motion.report_from_sums(np.zeros((1, 5), np.int64), 32, 32).rms[0])
