"""The evaluation front door on the MI355X: vk_frame_fidelity_u8 (csrc/fidelity.hip) against numpy -- the squared differences exactly, SSIM
against the float64 reference within the bound tests/_fidelity_ref.py derives from the float32 emulation -- and `evaluate.main` on the tiny
world of tests/test_frontdoor_gpu.py (5 frames, 128 x 256, 3 steps), online, as a rollout over 7 annotated frames, and offline."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import _fidelity_ref as R
from tests.test_frontdoor_gpu import H, STEPS, T, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)

pytestmark = pytest.mark.gpu


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_case_table_against_numpy(shape):
    from vista_amd import fidelity, ops
    n, Hh, Ww = shape
    bound = R.ssim_bound(Hh, Ww)
    count = (Hh - 10) * (Ww - 10)
    for name in R.CONTENTS:
        a, b = R.make_case(name, shape)
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        sse, ssim_sum = ops.frame_fidelity_u8(da, db)
        assert sse.shape == ssim_sum.shape == (n, 3) and sse.dtype == torch.int64 and ssim_sum.dtype == torch.float64 and sse.is_cuda
        want_sse = R.sse_ref(a, b)
        assert np.array_equal(sse.cpu().numpy(), want_sse), (name, sse.cpu().numpy() - want_sse)
        rep = fidelity.frame_metrics(da, db)
        want = R.ssim_ref64(a, b)
        err = float(np.abs(rep.ssim - want).max())
        print(f"[parity] frame_fidelity {shape} {name}: ssim {want.mean():.6f}, error against float64 {err:.3e} (bound {bound:.2e})")
        assert np.array_equal(rep.sse, want_sse) and np.array_equal(rep.ssim, (ssim_sum.cpu().numpy() / count).mean(axis=1))
        assert err <= bound, (name, err, bound)
        total = want_sse.sum(axis=1)
        with np.errstate(divide="ignore"):
            assert np.allclose(rep.psnr, 10 * np.log10(65025.0 * 3 * Hh * Ww / total), rtol=1e-14, atol=0)
        if name == "itself":
            assert not sse.any() and np.array_equal(rep.ssim, np.ones(n)) and np.all(rep.psnr == np.inf)
            assert torch.equal(ssim_sum, torch.full((n, 3), float(count), dtype=torch.float64, device="cuda")), "exactly 1 per window"
        # bitwise repeatable, and a frame's values do not depend on n or on the frames around it
        sse2, ssim2 = ops.frame_fidelity_u8(da, db)
        assert torch.equal(sse2, sse) and torch.equal(ssim2, ssim_sum), name
        lo, hi = min(1, n - 1), min(3, n)
        sse3, ssim3 = ops.frame_fidelity_u8(da[lo:hi], db[lo:hi])
        assert torch.equal(sse3, sse[lo:hi]) and torch.equal(ssim3, ssim_sum[lo:hi]), name


def test_float_frames_go_through_frames_to_u8():
    from vista_amd import fidelity, ops
    g = torch.Generator().manual_seed(5)
    pred, real = torch.rand(2, 3, 24, 40, generator=g).cuda(), (torch.rand(2, 3, 24, 40, generator=g) * 2 - 1).cuda()
    pu, ru = ops.frames_to_u8(pred, real=False), ops.frames_to_u8(real, real=True)
    want = fidelity.frame_metrics(pu, ru)
    for p, r in ((pred, real), (pu, real), (pred, ru)):
        got = fidelity.frame_metrics(p, r)
        assert np.array_equal(got.sse, want.sse) and np.array_equal(got.ssim, want.ssim) and np.array_equal(got.psnr, want.psnr)
    assert np.array_equal(want.sse, R.sse_ref(pu.cpu().numpy(), ru.cpu().numpy()))
    with pytest.raises(ValueError, match="pair up"):
        fidelity.frame_metrics(pred, real[:1])
    with pytest.raises(ValueError, match="window"):
        fidelity.frame_metrics(pred[:, :, :10], real[:, :, :10])
    with pytest.raises(TypeError):
        fidelity.frame_metrics(pred.double(), real)


def test_refusals():
    from vista_amd import _lib, fidelity, ops
    a = torch.zeros(2, 12, 16, 3, dtype=torch.uint8).cuda()
    with pytest.raises(TypeError):
        ops.frame_fidelity_u8(a.float(), a)
    with pytest.raises(TypeError):
        ops.frame_fidelity_u8(a, a.to(torch.int8))
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.frame_fidelity_u8(a.cpu(), a)
    with pytest.raises(_lib.VistaHipError, match="MI355X only"):
        ops.frame_fidelity_u8(a, a.cpu())
    for bad in (a[0], a[..., :2], a.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            ops.frame_fidelity_u8(bad, bad)
    with pytest.raises(ValueError):
        ops.frame_fidelity_u8(a, a[:1])
    for shape in ((1, 10, 16, 3), (1, 16, 10, 3)):
        with pytest.raises(_lib.VistaHipError, match="-22"):
            ops.frame_fidelity_u8(torch.zeros(shape, dtype=torch.uint8).cuda(), torch.zeros(shape, dtype=torch.uint8).cuda())
    lib, p, s, w = _lib.load(), ops._p, ops._stream(), fidelity.window_ptr()
    assert lib.vk_frame_fidelity_ws_bytes(10, 16) == -22 and lib.vk_frame_fidelity_ws_bytes(16, 10) == -22
    assert lib.vk_frame_fidelity_ws_bytes(11, 11) == 48
    tiles = -(-(576 - 10) // ops.FIDELITY_TILE_H) * -(-(1024 - 10) // ops.FIDELITY_TILE_W)
    assert lib.vk_frame_fidelity_ws_bytes(576, 1024) == 48 * tiles
    sse, ssim = torch.zeros(2, 3, dtype=torch.int64).cuda(), torch.zeros(2, 3, dtype=torch.float64).cuda()
    ws = torch.zeros(2 * lib.vk_frame_fidelity_ws_bytes(12, 16) // 8 + 1, dtype=torch.float64).cuda()
    args = [p(a), p(a), p(sse), p(ssim), p(ws), w]
    for i in range(6):
        holed = list(args)
        holed[i] = None
        assert lib.vk_frame_fidelity_u8(*holed, 2, 12, 16, s) == -22, i
    for n, Hh, Ww in ((0, 12, 16), (-1, 12, 16), (65536, 12, 16), (2, 10, 16), (2, 12, 10)):
        assert lib.vk_frame_fidelity_u8(*args, n, Hh, Ww, s) == -22, (n, Hh, Ww)
    odd_ws = C_void_p_plus(ws, 4)
    assert lib.vk_frame_fidelity_u8(p(a), p(a), p(sse), p(ssim), odd_ws, w, 2, 12, 16, s) == -22, "a misaligned workspace"
    assert lib.vk_frame_fidelity_u8(C_void_p_plus(a, 1), p(a), p(sse), p(ssim), p(ws), w, 1, 12, 16, s) == -22, "4-byte loads need 4-byte alignment"
    assert lib.vk_frame_fidelity_u8(*args, 2, 12, 16, s) == 0
    torch.cuda.synchronize()
    assert not sse.any() and torch.equal(ssim, torch.full((2, 3), 12.0, dtype=torch.float64, device="cuda"))


def C_void_p_plus(t, nbytes):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + nbytes)


# ---- evaluate.main on the tiny world ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(world):
    """Seven pictures (the world's five and two more) and an annotation of two scenes: one lists all seven, one the last five."""
    from PIL import Image
    root = world["dir"] / "fidelity_data"
    (root / "cam").mkdir(parents=True)
    names = []
    for i, src in enumerate(world["frames"]):
        names.append(f"cam/frame{i}.png")
        shutil.copy(src, root / names[-1])
    rng = np.random.default_rng(9)
    for i in (5, 6):
        yy, xx = np.mgrid[0:180, 0:320]
        img = np.stack([127 + 120 * np.sin(xx / (9.0 + i) + c) * np.cos(yy / (7.0 + c)) for c in range(3)], -1) + rng.normal(0, 6, (180, 320, 3))
        names.append(f"cam/frame{i}.png")
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(root / names[-1])
    traj = [0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 1.5, 0.1, 2.0, 0.2]
    anno = str(world["dir"] / "fidelity_anno.json")
    with open(anno, "w") as f:
        json.dump([{"frames": names, "traj": traj, "cmd": 1, "speed": [], "angle": [], "z": 1.0, "goal": [800.0, 450.0]},
                   {"frames": names[2:], "traj": traj, "cmd": 2, "speed": [], "angle": [], "z": 1.0, "goal": [800.0, 450.0]}], f)
    return {"data_root": str(root), "anno": anno, "names": names}


def _flags(world, scenes, save):
    return ["--config", world["config"], "--ckpt", world["ckpt"], "--dataset", "NUSCENES", "--data_root", scenes["data_root"], "--anno_file",
            scenes["anno"], "--action", "traj", "--n_frames", str(T), "--height", str(H), "--width", str(W), "--n_steps", str(STEPS),
            "--cond_aug", "0.02", "--rand_gen", "--save", save]


def _records(save):
    return [json.loads(line) for line in open(os.path.join(save, "metrics.jsonl")).read().splitlines()]


def _pictures(save, sub, index, count):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(save, sub, "images", f"NUSCENES_{index:06}_{i:04}.png"))) for i in range(count)])


def _check_against_the_pictures(save, records, frames):
    """Every number of the records against numpy over the PNGs the run wrote; means and the horizon curve against the per-frame lists.
    `frames`: how many frames every record must have scored."""
    from vista_amd import evaluate
    assert [rec["frames_scored"] for rec in records] == frames
    for rec in records:
        n = rec["frames_scored"]
        assert rec["cond"] == [0] and len(rec["psnr"]) == len(rec["ssim"]) == len(rec["sse"]) == n
        pred, real = _pictures(save, "virtual", rec["index"], n), _pictures(save, "real", rec["index"], n)
        assert pred.shape == real.shape == (n, H, W, 3)
        sse = R.sse_ref(pred, real)
        assert rec["sse"] == sse.tolist()
        want_ssim = R.ssim_ref64(pred, real)
        err = float(np.abs(np.array(rec["ssim"]) - want_ssim).max())
        print(f"[parity] evaluate scene {rec['index']}: {n} frames, ssim {want_ssim.min():.4f} ... {want_ssim.max():.4f}, error against float64 {err:.3e}")
        assert err <= R.SSIM_BOUND
        assert np.allclose(rec["psnr"], 10 * np.log10(65025.0 * 3 * H * W / sse.sum(axis=1)), rtol=1e-14, atol=0)
        pred_idx = list(range(1, n))
        assert rec["mean_psnr"] == math.fsum(rec["psnr"][i] for i in pred_idx) / len(pred_idx)
        assert rec["mean_ssim"] == math.fsum(rec["ssim"][i] for i in pred_idx) / len(pred_idx)
        for r in rec["rounds"]:
            members = [i for i in pred_idx if evaluate.frame_round(i, T) == r["round"]]
            assert r["frames"] == len(members) and r["mean_psnr"] == math.fsum(rec["psnr"][i] for i in members) / len(members)
            assert r["mean_ssim"] == math.fsum(rec["ssim"][i] for i in members) / len(members)
        assert sum(r["frames"] for r in rec["rounds"]) == n - 1
    summary = json.load(open(os.path.join(save, "metrics_summary.json")))
    assert summary["scenes"] == len(records)
    assert summary["mean_psnr"] == math.fsum(r["mean_psnr"] for r in records) / len(records)
    assert summary["mean_ssim"] == math.fsum(r["mean_ssim"] for r in records) / len(records)
    hz = summary["horizon"]
    assert hz["frame"] == list(range(max(frames))) and hz["scenes"] == [0] + [sum(i < f for f in frames) for i in range(1, max(frames))]
    assert hz["psnr"][0] is None and hz["ssim"][0] is None, "the conditioning frame is in no mean"
    for i in range(1, max(frames)):
        has = [r for r in records if i < r["frames_scored"]]
        assert hz["psnr"][i] == math.fsum(r["psnr"][i] for r in has) / len(has)
        assert hz["ssim"][i] == math.fsum(r["ssim"][i] for r in has) / len(has)
    return summary


def _per_frame(records):
    return [(r["index"], r["frames_scored"], r["psnr"], r["ssim"], r["sse"], r["cond"], r["mean_psnr"], r["mean_ssim"], r["rounds"]) for r in records]


def test_evaluate_two_scenes_online_then_offline(world, scenes, model, capsys):
    from vista_amd import evaluate, ops, sample
    from vista_amd import sample_utils as SU
    save = str(world["dir"] / "evaluate_out")
    assert evaluate.main(_flags(world, scenes, save)) == 0          # --n_scenes 0: the sequential walk to the end of the dataset
    out = capsys.readouterr().out
    assert "evaluate 0: 5 frames" in out and "evaluate 1: 5 frames" in out and "metrics" in out
    assert sorted(os.listdir(save)) == ["metrics.jsonl", "metrics_summary.json", "real", "virtual"]
    records = _records(save)
    assert [r["index"] for r in records] == [0, 1] and all(r["n_rounds"] == 1 and r["action"] == "traj" and r["seed"] == 23 for r in records)
    assert records[1]["frames"] == [os.path.join(scenes["data_root"], scenes["names"][2])]
    assert all(sorted(r["timings"]) == ["condition", "decode", "encode", "load", "metrics", "sample", "save"] for r in records)
    assert [r["round"] for r in records[0]["rounds"]] == [0]
    online = _check_against_the_pictures(save, records, [T, T])
    assert records[0]["ssim"] != records[1]["ssim"] and all(v < 1.0 for r in records for v in r["ssim"])
    # the pictures are the ones vista_amd.sample writes for the scene (same seeding, same kernels)
    sample.seed_everything(23)
    frame_list, index, total, action = SU.get_sample(1, "NUSCENES", T, "traj", data_root=scenes["data_root"], anno_file=scenes["anno"])
    samples, _, inputs = sample.run(model, frame_list, action, height=H, width=W, n_frames=T, n_steps=STEPS, cond_aug=0.02)
    assert np.array_equal(_pictures(save, "virtual", 1, T), ops.frames_to_u8(samples, real=False).cpu().numpy())
    assert np.array_equal(_pictures(save, "real", 1, T), ops.frames_to_u8(inputs, real=True).cpu().numpy())
    # offline over the same bytes: the same numbers, exactly
    assert evaluate.main(["--compare", save, "--n_conds", "1", "--n_frames", str(T), "--action", "traj"]) == 0
    offline = _records(save)
    assert _per_frame(offline) == _per_frame(records)
    assert json.load(open(os.path.join(save, "metrics_summary.json"))) == online
    assert all(sorted(r["timings"]) == ["load", "metrics"] for r in offline)
    # --n_scenes 1 --no_pictures: one record, the metrics files only
    save2 = str(world["dir"] / "evaluate_out_plain")
    assert evaluate.main(_flags(world, scenes, save2) + ["--n_scenes", "1", "--no_pictures"]) == 0
    assert sorted(os.listdir(save2)) == ["metrics.jsonl", "metrics_summary.json"]
    assert _per_frame(_records(save2)) == _per_frame(records[:1])


def test_evaluate_a_rollout_scores_the_frames_the_annotation_lists(world, scenes, model, monkeypatch):
    """Two rounds predict 7 frames. Scene 0 lists 7 real frames: all are scored, the two beyond the window loaded by evaluate itself. Scene 1
    lists the window's 5: the rollout is scored as far as there is ground truth."""
    from vista_amd import evaluate
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)        # (the fixture's pipeline: same config, same checkpoint)
    save = str(world["dir"] / "evaluate_rollout")
    assert evaluate.main(_flags(world, scenes, save) + ["--n_rounds", "2"]) == 0
    records = _records(save)
    assert len(records) == 2 and records[0]["frames_scored"] == 7 == evaluate.rollout_length(T, 2) and records[0]["n_rounds"] == 2
    assert [(r["round"], r["frames"]) for r in records[0]["rounds"]] == [(0, 4), (1, 2)]
    assert [(r["round"], r["frames"]) for r in records[1]["rounds"]] == [(0, 4)]
    assert len(os.listdir(os.path.join(save, "virtual", "images"))) == 14 and len(os.listdir(os.path.join(save, "real", "images"))) == 12
    online = _check_against_the_pictures(save, records, [7, T])
    assert evaluate.main(["--compare", save, "--n_conds", "1", "--n_frames", str(T), "--n_rounds", "2", "--action", "traj"]) == 0
    assert _per_frame(_records(save)) == _per_frame(records) and json.load(open(os.path.join(save, "metrics_summary.json"))) == online
