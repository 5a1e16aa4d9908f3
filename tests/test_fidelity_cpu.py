"""Host side of the evaluation front door (vista_amd/evaluate.py, vista_amd/fidelity.py): CLI flags, what is refused before a model is built, the
record and summary writers, the window table, and the SSIM bound of tests/_fidelity_ref.py measured against the float32 emulations. No GPU."""
import json
import math
import os

import numpy as np
import pytest

from tests import _fidelity_ref as R


def test_cli_flags_are_the_sampling_flags_plus_three():
    from vista_amd import evaluate, sample
    base = {a.dest: a for a in sample.parse_args()._actions if a.dest != "help"}
    mine = {a.dest: a for a in evaluate.parse_args()._actions if a.dest != "help"}
    assert sorted(set(mine) - set(base)) == ["compare", "n_scenes", "no_pictures"] and not set(base) - set(mine)
    for name, a in base.items():
        b = mine[name]
        assert (b.option_strings, b.default, b.type, b.nargs, b.const) == (a.option_strings, a.default, a.type, a.nargs, a.const), name
    assert mine["n_scenes"].default == 0 and mine["n_scenes"].type is int
    assert mine["no_pictures"].default is False and mine["no_pictures"].nargs == 0
    assert mine["compare"].default is None and mine["compare"].type is str
    opt = evaluate.parse_args().parse_args(["--rand_gen", "--n_scenes", "4", "--no_pictures", "--compare", "out", "--n_rounds", "2"])
    assert (opt.rand_gen, opt.n_scenes, opt.no_pictures, opt.compare, opt.n_rounds) == (False, 4, True, "out", 2)


@pytest.mark.parametrize("flags,env,match", [
    (["--rand_gen"], {"WORLD_SIZE": "2"}, "WORLD_SIZE 2"),
    ([], {}, "--n_scenes 0"),                                        # the random walk (the default) never ends by itself
    (["--n_scenes", "-1"], {}, "--n_scenes -1"),
    (["--rand_gen", "--dataset", "IMG"], {}, "--dataset IMG"),
    (["--n_scenes", "2", "--dataset", "IMG"], {}, "--dataset IMG"),
    (["--rand_gen", "--height", "100"], {}, "--height 100"),
    (["--rand_gen", "--n_frames", "33"], {}, "--n_frames 33"),
    (["--rand_gen", "--n_rounds", "2", "--n_frames", "3"], {}, "--n_frames 3"),
    (["--rand_gen", "--n_conds", "0"], {}, "--n_conds 0"),
], ids=["world_size", "random_walk_without_a_count", "negative_count", "img_sequential", "img_counted", "height", "window", "rollout_window", "n_conds"])
def test_what_cannot_run_is_refused_before_a_model_is_built(flags, env, match, monkeypatch, tmp_path):
    from vista_amd import evaluate
    from vista_amd import sample_utils as SU

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(SU, "init_model", no_model)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(ValueError, match=match):
        evaluate.main(flags + ["--save", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists(), "a refused run writes nothing"


def test_compare_refuses_a_missing_tree_and_several_gpus(monkeypatch, tmp_path):
    from vista_amd import evaluate
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(FileNotFoundError, match="virtual"):
        evaluate.main(["--compare", str(tmp_path)])
    for sub in ("virtual", "real"):
        (tmp_path / sub / "images").mkdir(parents=True)
    (tmp_path / "virtual" / "images" / "NUSCENES_000000_0000.png").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="under both"):
        evaluate.main(["--compare", str(tmp_path)])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE 2"):
        evaluate.main(["--compare", str(tmp_path)])


def test_picture_pairs_group_the_reference_file_names(tmp_path):
    from vista_amd import evaluate
    names = {"virtual": ["NUSCENES_000003_0001.png", "NUSCENES_000003_0000.png", "NUSCENES_000003_0002.png", "NUSCENES_000001_0000.png", "notes.txt"],
             "real": ["NUSCENES_000003_0000.png", "NUSCENES_000003_0001.png", "NUSCENES_000001_0000.png", "NUSCENES_000001.png"]}
    for sub, files in names.items():
        (tmp_path / sub / "images").mkdir(parents=True)
        for f in files:
            (tmp_path / sub / "images" / f).write_bytes(b"")
    got = evaluate.picture_pairs(str(tmp_path))
    assert [(d, i, [f for f, _, _ in frames]) for d, i, frames in got] == [("NUSCENES", 1, [0]), ("NUSCENES", 3, [0, 1])]
    assert got[1][2][1][1:] == (str(tmp_path / "virtual" / "images" / "NUSCENES_000003_0001.png"), str(tmp_path / "real" / "images" / "NUSCENES_000003_0001.png"))


def test_future_frames_follow_the_annotation(tmp_path):
    from vista_amd import evaluate
    root = tmp_path / "data"
    root.mkdir()
    names = [f"f{i}.png" for i in range(7)]
    for n in names[:6]:
        (root / n).write_bytes(b"x")
    anno = tmp_path / "anno.json"
    anno.write_text(json.dumps([{"frames": names}, {"frames": names[:5]}]))
    kw = dict(data_root=str(root), anno_file=str(anno))
    assert evaluate.future_frames(0, 5, 7, **kw) == [str(root / "f5.png")], "f6 is listed but not on disk: ground truth ends before it"
    assert evaluate.future_frames(0, 5, 6, **kw) == [str(root / "f5.png")]
    assert evaluate.future_frames(1, 5, 7, **kw) == [] and evaluate.future_frames(0, 5, 5, **kw) == []
    assert evaluate.rollout_length(25, 1) == 25 and evaluate.rollout_length(25, 4) == 91 and evaluate.rollout_length(5, 2) == 7
    assert [evaluate.frame_round(i, 5) for i in range(9)] == [0, 0, 0, 0, 0, 1, 1, 2, 2]


def _report(psnr, ssim):
    from vista_amd.fidelity import FidelityReport
    n = len(psnr)
    return FidelityReport(sse=np.arange(3 * n, dtype=np.int64).reshape(n, 3), mse=np.zeros(n), psnr=np.array(psnr, dtype=np.float64),
                          ssim=np.array(ssim, dtype=np.float64))


def test_records_and_summary_from_hand_made_reports(tmp_path):
    from vista_amd import evaluate, frontdoor
    a = evaluate.make_record(4, ["a0.png", "a1.png"], _report([40.0, 30.0, 20.0, 10.0, 12.0, 8.0, 6.0], [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3]),
                             seed=23, action="traj", n_conds=1, n_rounds=2, n_frames=5, timings={"metrics": 0.123456})
    assert sorted(a) == sorted(["index", "frames", "seed", "action", "n_conds", "n_rounds", "frames_scored", "psnr", "ssim", "sse", "cond",
                                "mean_psnr", "mean_ssim", "rounds", "timings"])
    assert (a["index"], a["frames"], a["seed"], a["action"], a["n_conds"], a["n_rounds"], a["frames_scored"]) == (4, ["a0.png"], 23, "traj", 1, 2, 7)
    assert a["cond"] == [0] and a["sse"][1] == [3, 4, 5] and a["timings"] == {"metrics": 0.1235}
    assert a["mean_psnr"] == pytest.approx((30 + 20 + 10 + 12 + 8 + 6) / 6) and a["mean_ssim"] == pytest.approx((0.8 + 0.7 + 0.6 + 0.5 + 0.4 + 0.3) / 6)
    assert a["rounds"] == [{"round": 0, "frames": 4, "mean_psnr": pytest.approx(18.0), "mean_ssim": pytest.approx(0.65)},
                           {"round": 1, "frames": 2, "mean_psnr": pytest.approx(7.0), "mean_ssim": pytest.approx(0.35)}]
    # an identical predicted frame: its PSNR is infinite, written as null, and so is every mean it is part of
    b = evaluate.make_record(5, ["b0.png"], _report([math.inf, math.inf, 25.0], [1.0, 1.0, 0.5]), seed=23, action="free", n_conds=1, n_rounds=1,
                             n_frames=3)
    assert b["psnr"] == [None, None, 25.0] and b["mean_psnr"] is None and b["mean_ssim"] == pytest.approx(0.75) and b["timings"] == {}
    # conditioning frames only: means over nothing
    c = evaluate.make_record(6, ["c0.png"], _report([50.0, 45.0], [0.99, 0.98]), seed=23, action="free", n_conds=2, n_rounds=1, n_frames=2)
    assert c["cond"] == [0, 1] and c["mean_psnr"] is None and c["mean_ssim"] is None and c["rounds"] == []

    save = str(tmp_path / "out")
    assert frontdoor.start_records(save, evaluate.RECORDS_NAME) == os.path.join(save, "metrics.jsonl")
    for rec in (a, b):
        frontdoor.append_record(save, evaluate.RECORDS_NAME, rec)
    lines = open(os.path.join(save, "metrics.jsonl")).read().splitlines()
    assert [json.loads(line) for line in lines] == [json.loads(json.dumps(a)), json.loads(json.dumps(b))] and "Infinity" not in "".join(lines)
    frontdoor.start_records(save, evaluate.RECORDS_NAME)
    assert open(os.path.join(save, "metrics.jsonl")).read() == "", "a run starts its own file"

    s = evaluate.summarize([a, b, c])
    assert s["scenes"] == 3 and s["mean_psnr"] is None and s["mean_ssim"] == pytest.approx((a["mean_ssim"] + 0.75) / 2)
    assert s["horizon"]["frame"] == list(range(7)) and s["horizon"]["scenes"] == [0, 2, 2, 1, 1, 1, 1]
    assert s["horizon"]["psnr"] == [None, None, pytest.approx(22.5), 10.0, 12.0, 8.0, 6.0]
    assert s["horizon"]["ssim"] == [None, pytest.approx(0.9), pytest.approx(0.6), 0.6, 0.5, 0.4, 0.3]
    s2 = evaluate.summarize([a])
    assert s2["mean_psnr"] == a["mean_psnr"] and s2["horizon"]["psnr"][1:] == a["psnr"][1:] and s2["horizon"]["psnr"][0] is None
    path = frontdoor.write_summary(save, evaluate.SUMMARY_NAME, evaluate.summarize([a, b, c]))
    assert path == os.path.join(save, "metrics_summary.json") and json.load(open(path)) == json.loads(json.dumps(s))
    assert evaluate.summarize([]) == {"scenes": 0, "mean_psnr": None, "mean_ssim": None, "horizon": {"frame": [], "scenes": [], "psnr": [], "ssim": []}}


def test_report_from_sums_forms_psnr_and_ssim_in_float64():
    from vista_amd import fidelity
    H, W = 12, 13
    sse = np.array([[0, 0, 0], [1, 2, 3], [12 * 13 * 65025] * 3], dtype=np.int64)
    count = (H - 10) * (W - 10)
    rep = fidelity.report_from_sums(sse, np.array([[count] * 3, [count * 0.5, count * 0.25, 0.0], [0.0, 0.0, 0.0]]), H, W)
    assert rep.sse.dtype == np.int64 and rep.psnr.dtype == rep.ssim.dtype == rep.mse.dtype == np.float64
    assert rep.psnr[0] == math.inf and rep.psnr[2] == 0.0 and rep.psnr[1] == pytest.approx(10 * math.log10(65025 * 3 * H * W / 6), rel=1e-15)
    assert rep.mse.tolist() == [0.0, 6 / (3 * H * W), 65025.0] and rep.ssim.tolist() == [1.0, 0.25, 0.0]


def test_window_table():
    from vista_amd import fidelity, ops
    w = fidelity.WINDOW_F64
    assert w.dtype == np.float64 and w.shape == (11,) == (ops.FIDELITY_TAPS,) and abs(w.sum() - 1.0) <= 2e-16
    assert np.array_equal(w, w[::-1]) and w.argmax() == 5 and w[5] / w[4] == pytest.approx(math.exp(1 / 4.5), rel=1e-15)
    assert fidelity.WINDOW_F32.dtype == np.float32 and np.array_equal(fidelity.WINDOW_F32, w.astype(np.float32)), "rounded once"
    assert abs(float(fidelity.WINDOW_F32.astype(np.float64).sum()) - 1.0) <= 11 * 2.0 ** -25
    assert not fidelity.WINDOW_F32.flags.writeable
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vista_hip.h")).read()
    for name, value in (("TAPS", ops.FIDELITY_TAPS), ("TILE_H", ops.FIDELITY_TILE_H), ("TILE_W", ops.FIDELITY_TILE_W)):
        assert f"#define VK_FIDELITY_{name} {value}\n" in hdr, name


@pytest.fixture(scope="module")
def emulation_errors():
    """{(shape, content): (pivoted error, error without the pivot)} of the float32 emulations against float64, the largest frame of the entry."""
    out = {}
    for shape in R.SHAPES:
        for name in R.CONTENTS:
            a, b = R.make_case(name, shape)
            ref = R.ssim_ref64(a, b)
            out[shape, name] = (float(np.abs(R.ssim_emulated32(a, b, 128) - ref).max()), float(np.abs(R.ssim_emulated32(a, b, 0) - ref).max()))
            print(f"[emulation] {shape} {name}: pivot 128 {out[shape, name][0]:.3e}, no pivot {out[shape, name][1]:.3e}")
    return out


def test_the_bound_is_four_times_the_pivoted_emulation_error(emulation_errors):
    many = max(e[0] for (shape, _), e in emulation_errors.items() if shape[1:] != (11, 11))
    one = max(e[0] for (shape, _), e in emulation_errors.items() if shape[1:] == (11, 11))
    assert R.SSIM_BOUND == 4 * 3.70e-6 and R.SSIM_BOUND_ONE_WINDOW == 4 * 2.13e-5
    assert 3.6e-6 <= many <= 3.70e-6 and 2.1e-5 <= one <= 2.13e-5, (many, one)     # the figures the bound was taken from, rounded up
    for (shape, name), (with_pivot, _) in emulation_errors.items():
        assert with_pivot <= R.ssim_bound(*shape[1:]) / 4, (shape, name, with_pivot)
    assert all(e == (0.0, 0.0) for (_, name), e in emulation_errors.items() if name == "itself")


def test_the_bound_bites_without_the_pivot(emulation_errors):
    for shape in R.SHAPES:
        if shape[1:] == (11, 11):
            continue   # (one window: tests/_fidelity_ref.py says why its bound cannot tell the two forms apart)
        for name in ("flat255_vs_254", "bright_250_255"):
            assert emulation_errors[shape, name][1] > 2 * R.SSIM_BOUND, (shape, name, emulation_errors[shape, name])
    assert all(emulation_errors[shape, "flat255_vs_254"][1] > 6.6e-5 > 4 * R.SSIM_BOUND for shape in R.SHAPES)
