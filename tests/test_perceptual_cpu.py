"""CLIP-space scores without a GPU: the host arithmetic of vista_amd/perceptual.py against the definitions, the bound tests/_perceptual_ref.py
states for vk_embed_mmd_sums and that it tells the stated arithmetic from the two forms it excludes, the records and the summary with and
without the new keyword, and the refusals of the VISTA_EVAL_CLIP hook."""
import math
import os
import re

import numpy as np
import pytest

from tests import _perceptual_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- from the sums to the MMD ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_mmd_from_sums_is_the_brute_force_definition(case):
    from vista_amd import perceptual
    x, y = R.make_sets(case)
    got = perceptual.mmd_from_sums(R.mmd_sums_ref(x, y), len(x), len(y))
    want = R.mmd_ref(x, y)
    assert got["m"] == want["m"] == len(x) and got["n"] == want["n"] == len(y)
    # both are differences of means of k (each about 1) times 1000: 1e-12 is ten thousand ulps of fp64 below the scale
    assert abs(got["biased"] - want["biased"]) <= 1e-9, (got, want)
    if min(len(x), len(y)) == 1:
        assert got["unbiased"] is None and want["unbiased"] is None
    else:
        assert abs(got["unbiased"] - want["unbiased"]) <= 1e-9, (got, want)
        assert got["unbiased"] != got["biased"]


def test_identical_sets_have_no_distance_and_one_row_no_pairs():
    from vista_amd import perceptual
    x, _ = R.make_sets((63, 65, 80))
    got = perceptual.mmd_from_sums(R.mmd_sums_ref(x, x), len(x), len(x))
    assert abs(got["biased"]) <= 1e-9, got
    assert got["unbiased"] < 0, "the U-statistic of a set against itself is below zero by the diagonal it leaves out"
    one = R.mmd_sums_ref(x[:1], x[:5])
    assert one[0] == 0.0 and perceptual.mmd_from_sums(one, 1, 5)["unbiased"] is None
    nan = perceptual.mmd_from_sums([float("nan"), 1.0, 2.0], 3, 3)
    assert math.isnan(nan["biased"]) and perceptual.mmd_json(nan) == {"biased": None, "unbiased": None, "m": 3, "n": 3}


# ---- the bound of vk_embed_mmd_sums ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def errors():
    """case -> {form: the three relative errors against float64}, computed once."""
    out = {}
    for case in R.CASES:
        x, y = R.make_sets(case)
        want = R.mmd_sums_ref(x, y)
        out[case] = {form: R.rel_errors(R.mmd_sums_emulated(x, y, form=form), want) for form in ("expm1", "one_minus_exp", "dot")}
    return out


def test_the_bounds_are_four_times_the_emulations_error(errors):
    for near, bound in ((False, R.MMD_REL_BOUND), (True, R.MMD_REL_BOUND_NEAR)):
        worst = max(float(errors[c]["expm1"].max()) for c in R.CASES if (len(c) > 3) == near)
        print(f"[parity] mmd emulation, {'near' if near else 'plain'} sets: worst relative error {worst:.3e}, bound {bound:.2e}")
        assert bound / 8 <= worst <= bound / 4, (near, worst, bound)
    large = max(float(errors[c]["expm1"].max()) for c in R.LARGE)
    assert 1e-8 <= large <= 6e-8, large   # (a mean of thousands of fp32 errors, and gamma's own rounding of 2.2e-8)
    m1 = errors[(1, 1, 1)]["expm1"]
    assert m1[0] == 0 and m1[1] == 0, "one row has no pair: S_xx and S_yy are exactly 0"


def test_the_bound_excludes_one_minus_exp(errors):
    for case in R.CASES:
        if len(case) > 3:
            assert np.all(errors[case]["one_minus_exp"] > R.mmd_bound(case)), case   # k rounds to 1: every term is lost
            assert np.all(errors[case]["one_minus_exp"] > 0.99)
    assert np.all(errors[(2, 3, 3)]["one_minus_exp"] > 100 * R.MMD_REL_BOUND)
    # where a sum has thousands of terms the form's error averages down, and is still several times what the stated arithmetic leaves
    emul = max(float(errors[c]["expm1"].max()) for c in R.LARGE)
    form = max(float(errors[c]["one_minus_exp"].max()) for c in R.LARGE)
    print(f"[parity] 1 - exp on the large plain sets: {form:.3e} against the emulation's {emul:.3e}")
    assert form > 4 * emul


def test_the_bound_excludes_two_minus_two_dot(errors):
    for case in R.CASES:
        if len(case) > 3:   # y = x + 1e-4 noise: 2 - 2 u.v is a difference of two numbers that agree to seven digits
            assert np.all(errors[case]["dot"] > 100 * R.mmd_bound(case)), (case, errors[case]["dot"])
    assert errors[(2, 3, 3)]["dot"].max() > R.MMD_REL_BOUND


def test_row_stats_and_frame_scores_references():
    from vista_amd import perceptual
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((5, 80)).astype(np.float32), rng.standard_normal((5, 80)).astype(np.float32)
    st = R.row_stats_ref(a, b)
    assert np.allclose(perceptual.cosines(st), R.cosines_ref(a, b), rtol=1e-15, atol=0)
    assert np.array_equal(perceptual.cosines(R.row_stats_ref(a, a)), np.ones(5)), "sqrt(s * s) is s: a row against itself is exactly 1"
    bad = np.array([[1.0, 0.0, 2.0], [1.0, float("inf"), 2.0], [float("nan"), 1.0, 1.0], [0.5, 1.0, 1.0]])
    got = perceptual.cosines(bad)
    assert np.isnan(got[:3]).all() and got[3] == 0.5
    ref = R.frame_scores_ref(a, b)
    assert np.isnan(ref["step"][0]) and np.isnan(ref["step_real"][0]) and ref["sim"].shape == ref["step"].shape == (5,)


# ---- records and summary -----------------------------------------------------------------------------------------------------------------------
def _fidelity_report(n):
    from vista_amd import fidelity
    sse = np.arange(3 * n, dtype=np.int64).reshape(n, 3) + 1
    return fidelity.FidelityReport(sse=sse, mse=sse.sum(1) / 300.0, psnr=np.array([30.0 + i for i in range(n)]), ssim=np.array([0.5 + 0.0625 * i for i in range(n)]))


KW = dict(seed=23, action="traj", n_conds=1, n_rounds=2, n_frames=5, timings={"load": 0.12345, "metrics": 0.5})
PARENT_RECORD = {
    "index": 4, "frames": ["a.png"], "seed": 23, "action": "traj", "n_conds": 1, "n_rounds": 2, "frames_scored": 7,
    "psnr": [30.0, 31.0, 32.0, 33.0, 34.0, 35.0, 36.0], "ssim": [0.5, 0.5625, 0.625, 0.6875, 0.75, 0.8125, 0.875],
    "sse": [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15], [16, 17, 18], [19, 20, 21]], "cond": [0],
    "mean_psnr": 33.5, "mean_ssim": 0.71875,
    "rounds": [{"round": 0, "frames": 4, "mean_psnr": 32.5, "mean_ssim": 0.65625}, {"round": 1, "frames": 2, "mean_psnr": 35.5, "mean_ssim": 0.84375}],
    "timings": {"load": 0.1235, "metrics": 0.5}}


def test_records_and_summary_without_the_keyword_are_the_parents():
    from vista_amd import evaluate
    rec = evaluate.make_record(4, ["a.png", "b.png"], _fidelity_report(7), **KW)
    assert rec == PARENT_RECORD and list(rec) == list(PARENT_RECORD), "key for key, in the parent's order"
    assert evaluate.make_record(4, ["a.png", "b.png"], _fidelity_report(7), clip=None, **KW) == PARENT_RECORD
    summary = evaluate.summarize([rec])
    assert summary == evaluate.summarize([rec], clip=None)
    assert list(summary) == ["scenes", "mean_psnr", "mean_ssim", "horizon"] and list(summary["horizon"]) == ["frame", "scenes", "psnr", "ssim"]
    assert summary["mean_psnr"] == 33.5 and summary["horizon"]["psnr"] == [None, 31.0, 32.0, 33.0, 34.0, 35.0, 36.0]
    assert evaluate._scene_line(rec).startswith("evaluate 4: 7 frames, mean_psnr 33.5000, mean_ssim 0.7188 | load")


def _clip_report(n, nan_at=None):
    from vista_amd import perceptual
    sim = np.array([1.0] + [0.5 + 0.03125 * i for i in range(1, n)])
    step = np.array([np.nan] + [0.75 + 0.015625 * i for i in range(1, n)])
    step_real = np.array([np.nan] + [0.875] * (n - 1))
    if nan_at is not None:
        sim[nan_at] = np.nan
    return perceptual.PerceptualReport(sim=sim, step=step, step_real=step_real, mmd={"biased": 1.5, "unbiased": float("nan"), "m": n - 1, "n": n - 1})


def test_records_and_summary_with_the_keyword():
    from vista_amd import evaluate
    rec = evaluate.make_record(4, ["a.png"], _fidelity_report(7), clip=_clip_report(7), **KW)
    assert {k: v for k, v in rec.items() if "clip" not in k and k != "rounds"} == {k: v for k, v in PARENT_RECORD.items() if k != "rounds"}
    assert list(rec)[-1] == "timings" and list(rec)[:len(PARENT_RECORD) - 1] == list(PARENT_RECORD)[:-1]
    assert rec["clip_sim"] == [1.0, 0.53125, 0.5625, 0.59375, 0.625, 0.65625, 0.6875]
    assert rec["clip_step"][0] is None and rec["clip_step_real"] == [None] + [0.875] * 6, "NaN is written as null"
    assert rec["mean_clip_sim"] == 0.609375, "the conditioning frame (sim 1.0) is in no mean"
    assert rec["mean_clip_step"] == 0.75 + 0.015625 * 3.5 and rec["mean_clip_step_real"] == 0.875
    assert rec["clip_mmd"] == {"biased": 1.5, "unbiased": None, "m": 6, "n": 6}
    assert [r["mean_clip_sim"] for r in rec["rounds"]] == [0.578125, 0.671875]
    assert [{k: v for k, v in r.items() if k != "mean_clip_sim"} for r in rec["rounds"]] == PARENT_RECORD["rounds"]
    assert "mean_ssim 0.7188, mean_clip_sim 0.6094 | load" in evaluate._scene_line(rec)
    # a second, shorter scene with a NaN score: null in the record, in its mean and at that index of the horizon
    short = evaluate.make_record(5, ["c.png"], _fidelity_report(5), clip=_clip_report(5, nan_at=2), **KW)
    assert short["clip_sim"][2] is None and short["mean_clip_sim"] is None and short["rounds"][0]["mean_clip_sim"] is None
    assert short["mean_clip_step"] == 0.75 + 0.015625 * 2.5
    tower = {"embed": 1024, "image": 224, "patch": 14, "sigma": 10.0, "scale": 1000.0}
    summary = evaluate.summarize([rec, short], clip={"mmd": {"biased": 0.25, "unbiased": 0.125, "m": 10, "n": 10}, "tower": tower})
    plain = evaluate.summarize([rec, short])
    assert {k: summary[k] for k in plain if k != "horizon"} == {k: plain[k] for k in plain if k != "horizon"}
    assert {k: summary["horizon"][k] for k in plain["horizon"]} == plain["horizon"]
    assert summary["mean_clip_sim"] is None, "a scene mean that is null makes the mean over scenes null, as for PSNR"
    assert summary["mean_clip_step"] == (rec["mean_clip_step"] + short["mean_clip_step"]) / 2 and summary["mean_clip_step_real"] == 0.875
    hz = summary["horizon"]
    assert hz["clip_sim"] == [None, 0.53125, None, 0.59375, 0.625, 0.65625, 0.6875] and hz["clip_step"][0] is None
    assert hz["clip_step"][1:] == [0.765625, 0.78125, 0.796875, 0.8125, 0.828125, 0.84375]
    assert summary["clip_mmd"] == {"biased": 0.25, "unbiased": 0.125, "m": 10, "n": 10} and summary["clip"] == tower
    assert evaluate.summarize([rec], clip={"mmd": None, "tower": tower})["clip_mmd"] is None
    with pytest.raises(ValueError, match="holds 5 frames"):
        evaluate.make_record(4, ["a.png"], _fidelity_report(7), clip=_clip_report(5), **KW)


# ---- the hook ----------------------------------------------------------------------------------------------------------------------------------
def test_the_hook_is_read_in_one_place_and_refuses_by_name(monkeypatch):
    from vista_amd import evaluate, pipeline
    from vista_amd import sample_utils as SU
    assert SU.eval_clip is pipeline.eval_clip
    for value, want in ((None, False), ("", False), ("0", False), ("1", True)):
        monkeypatch.delenv("VISTA_EVAL_CLIP", raising=False)
        if value is not None:
            monkeypatch.setenv("VISTA_EVAL_CLIP", value)
        assert SU.eval_clip() is want
    readers = [f for f in os.listdir(os.path.join(ROOT, "vista_amd")) if f.endswith(".py")
               and re.search(r"os\.environ[^\n]*VISTA_EVAL_CLIP", open(os.path.join(ROOT, "vista_amd", f)).read())]
    assert readers == ["pipeline.py"]
    for bad in ("2", "yes", "true", " 1"):
        monkeypatch.setenv("VISTA_EVAL_CLIP", bad)
        with pytest.raises(ValueError, match="VISTA_EVAL_CLIP"):
            SU.eval_clip()
        with pytest.raises(ValueError, match=f"Bad value {bad} .environment hook VISTA_EVAL_CLIP."):   # before a model is built
            evaluate.main(["--dataset", "NUSCENES", "--rand_gen", "--n_scenes", "1"])
        with pytest.raises(ValueError, match="VISTA_EVAL_CLIP"):
            evaluate.main(["--compare", "nowhere"])


def test_compare_with_the_hook_refuses_a_missing_checkpoint_before_anything_is_read(monkeypatch, tmp_path):
    from vista_amd import evaluate
    monkeypatch.setenv("VISTA_EVAL_CLIP", "1")
    missing = str(tmp_path / "no_such.safetensors")
    with pytest.raises(FileNotFoundError, match="no_such.safetensors does not exist"):   # (not the pictures' folder, not the GPU)
        evaluate.main(["--compare", str(tmp_path / "no_pictures_either"), "--ckpt", missing])
    with pytest.raises(FileNotFoundError, match="ckpts/vista.safetensors does not exist"):
        monkeypatch.chdir(tmp_path)
        evaluate.main(["--compare", str(tmp_path / "no_pictures_either")])
    monkeypatch.setenv("VISTA_EVAL_CLIP", "0")
    with pytest.raises(FileNotFoundError, match="virtual"):   # without the hook: the parent's refusal, of the folder
        evaluate.main(["--compare", str(tmp_path / "no_pictures_either"), "--ckpt", missing])


# ---- the library's table and the wrappers' refusals ----------------------------------------------------------------------------------------------
def test_entry_points_are_declared_listed_and_built():
    import ctypes
    from vista_amd import _lib, build, ops
    assert "perceptual.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "vista_hip.h")).read()
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    pf = ctypes.POINTER(f32)
    assert _lib.SIGNATURES["vk_clip_preprocess_patches_u8"] == _lib.SIGNATURES["vk_clip_preprocess_patches"] == [vp, vp] + [i32] * 6 + [f32, f32, i32, i32, pf, pf, vp]
    assert _lib.SIGNATURES["vk_embed_row_stats"] == [vp, vp, vp, i32, i32, vp]
    assert _lib.SIGNATURES["vk_embed_mmd_ws_bytes"] == [i32, i32, i32]
    assert _lib.SIGNATURES["vk_embed_mmd_sums"] == [vp] * 4 + [i32] * 3 + [f32, vp]
    for name in ("libvista_hip.so", "libvista_hip_f16.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "vista_amd", "lib", name))
        for fn in ("vk_clip_preprocess_patches_u8", "vk_embed_row_stats", "vk_embed_mmd_ws_bytes", "vk_embed_mmd_sums"):
            assert hasattr(lib, fn) and re.search(rf"^int {fn}\(", hdr, flags=re.M), (name, fn)
    defines = {k: v for k, v in re.findall(r"#define (VK_EMBED_\w+) (.+)", hdr)}
    assert eval(defines["VK_EMBED_MAX_ROWS"]) == ops.EMBED_MAX_ROWS and eval(defines["VK_EMBED_MAX_DIM"]) == ops.EMBED_MAX_DIM
    assert int(defines["VK_EMBED_MMD_TILE"]) == ops.EMBED_MMD_TILE == 64
    lib = _lib.load()
    # [3][T][T] fp64 partials and m + n fp32 inverse norms; what it cannot state it refuses, and so does the launch
    assert lib.vk_embed_mmd_ws_bytes(1, 1, 1) == 24 + 8 and lib.vk_embed_mmd_ws_bytes(65, 3, 7) == 24 * 4 + 68 * 4
    assert lib.vk_embed_mmd_ws_bytes(4550, 4550, 1024) == 24 * 72 * 72 + 9100 * 4
    for m, n, d in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (ops.EMBED_MAX_ROWS + 1, 1, 1), (1, 1, ops.EMBED_MAX_DIM + 1), (ops.EMBED_MAX_ROWS, 1, 1)):
        assert lib.vk_embed_mmd_ws_bytes(m, n, d) == -22, (m, n, d)
    # NULL operands and bad shapes come back as -22 before anything is launched (no GPU needed)
    assert lib.vk_embed_mmd_sums(None, None, None, None, 1, 1, 1, 10.0, None) == -22
    assert lib.vk_embed_row_stats(None, None, None, 1, 1, None) == -22
    assert lib.vk_clip_preprocess_patches_u8(None, None, 1, 16, 16, 28, 14, 640, 1.0, 1.0, 1, 1, None, None, None) == -22


def test_wrappers_refuse_before_the_library_is_asked():
    import torch
    from vista_amd import _lib, ops, perceptual
    u8, f = torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 8)
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.clip_preprocess_patches_u8(u8, 28, 14)
    with pytest.raises(TypeError):
        ops.clip_preprocess_patches_u8(u8.float(), 28, 14)
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.embed_row_stats(f, f)
    with pytest.raises(TypeError):
        ops.embed_row_stats(f.double(), f)
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.embed_mmd_sums(f, f, 10.0)
    with pytest.raises(TypeError):
        ops.embed_mmd_sums(f.half(), f, 10.0)
    assert perceptual.EMBED_CHUNK == 16 and (perceptual.SIGMA, perceptual.SCALE) == (10.0, 1000.0)
