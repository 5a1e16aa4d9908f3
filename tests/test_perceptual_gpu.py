"""CLIP-space scores on the MI355X: the three kernels of csrc/perceptual.hip under guard bands (tests/_guard.py) -- the preprocessing from
bytes bit for bit against the fp32 kernel, the row statistics against float64, the MMD pair sums within the bound tests/_perceptual_ref.py
derives on the CPU -- then perceptual.embed_frames on the tiny tower, and `evaluate.main` with the VISTA_EVAL_CLIP hook on the tiny world of
tests/test_frontdoor_gpu.py: online, then offline over the saved pictures with the tower alone, the same numbers exactly."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import _perceptual_ref as R
from tests._guard import guarded, put, verify
from tests.test_fidelity_gpu import _flags, _per_frame, _records, scenes  # noqa: F401  (the two-scene dataset, by import)
from tests.test_frontdoor_gpu import H, STEPS, T, TINY_CLIP, W, _process_wide_graph_state_as_found, model, world  # noqa: F401  (fixtures, by import)

pytestmark = pytest.mark.gpu


# ---- (a) preprocessing from bytes --------------------------------------------------------------------------------------------------------------
def _byte_frames(Hh, Ww):
    """Two frames: seeded noise over all 256 values, and blocks of 0 and 255 (both ends of the range, hard edges under the blur)."""
    rng = np.random.default_rng(Hh * 1000 + Ww)
    noise = rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)
    noise[0, 0], noise[-1, -1] = 0, 255
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    blocks = (((yy // 5 + xx // 7) % 2) * 255).astype(np.uint8)[..., None].repeat(3, axis=2)
    blocks[..., 1] = 255 - blocks[..., 1]
    return torch.from_numpy(np.stack([noise, blocks]))


def _unit_frames(u8):
    """What a byte stands for: (float)b / 127.5f - 1.0f, an IEEE fp32 division and an fp32 subtraction, NCHW. Formed on the host, where
    torch divides (on the GPU it multiplies a tensor by the fp32 reciprocal of a scalar divisor, which rounds some bytes the other way)."""
    x = u8.cpu().permute(0, 3, 1, 2).float() / 127.5 - 1.0
    b = np.arange(256, dtype=np.float32)
    assert np.array_equal((torch.arange(256, dtype=torch.uint8).float() / 127.5 - 1.0).numpy(), b / np.float32(127.5) - np.float32(1.0))
    return x.contiguous()


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skew1"])
@pytest.mark.parametrize("geom", [(224, 14), (28, 14)], ids=lambda g: f"{g[0]}over{g[1]}")
@pytest.mark.parametrize("shape", [(128, 256), (37, 50), (300, 226)], ids=lambda s: "x".join(map(str, s)))
def test_preprocess_from_bytes_equals_the_fp32_kernel_bitwise(shape, geom, skew):
    """(128, 256): the dword path, both axes downscaled. (37, 50): the byte path; upscaling without a blur at 224. (300, 226): W % 4 != 0; at
    224 only H is downscaled (3 taps on both axes), at 28 the blur is 19 x 15 taps. A workgroup's tile is 16 outputs a side at 224 and for
    (37, 50); at 28 it is 8 for (128, 256) and 4 for (300, 226), whose source rectangles would not fit the LDS otherwise. A base skewed by
    one byte takes the byte path at every width."""
    from vista_amd import ops
    out_hw, patch = geom
    u8 = _byte_frames(*shape)
    with guarded(ops):
        got = ops.clip_preprocess_patches_u8(put(u8, skew=skew, label="frames_u8"), out_hw, patch)
        want = ops.clip_preprocess_patches(put(_unit_frames(u8), label="frames_f32"), out_hw, patch)
        verify()
    assert got.shape == want.shape == (2 * (1 + (out_hw // patch) ** 2), 640) and got.dtype == want.dtype
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    assert torch.equal(gi, wi), f"{int((gi != wi).sum())} of {gi.numel()} values differ, first at {(gi != wi).nonzero()[0].tolist()}"
    assert int((got.float().abs() > 0).sum()) >= 2 * 3 * out_hw * out_hw * 0.99, "the image columns are written"
    assert not got.view(2, -1, 640)[:, 0].any() and not got[:, 588:].any(), "class-token rows and the K padding stay zero"


def test_preprocess_from_bytes_refusals():
    from vista_amd import _lib, ops
    u8 = torch.zeros(2, 16, 20, 3, dtype=torch.uint8).cuda()
    for bad in (u8[0], u8[..., :2], u8.permute(0, 2, 1, 3), u8[:0]):
        with pytest.raises(ValueError):
            ops.clip_preprocess_patches_u8(bad, 28, 14)
    lib, p, s = _lib.load(), ops._p, ops._stream()
    out = torch.zeros(2 * 5, 640, dtype=ops.BF16).cuda()
    import ctypes
    m3, s3 = (ctypes.c_float * 3)(*ops.CLIP_MEAN), (ctypes.c_float * 3)(*ops.CLIP_STD)
    ok = [p(u8), p(out), 2, 16, 20, 28, 14, 640, 1.0, 1.0, 1, 1, m3, s3, s]
    for at, value in ((0, None), (1, None), (2, 0), (2, 65536), (3, 1), (5, 27), (6, 0), (7, 587), (10, 2), (10, 65), (10, 33), (9, 0.0), (12, None)):
        args = list(ok)
        args[at] = value
        assert lib.vk_clip_preprocess_patches_u8(*args) == -22, (at, value)   # (ks 33 on a side of 16: a reflected tap would leave the frame)
    assert lib.vk_clip_preprocess_patches_u8(*ok) == 0
    torch.cuda.synchronize()


# ---- (b) row statistics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.ROW_STATS_CASES, ids=lambda s: "x".join(map(str, s)))
def test_row_stats_against_float64(shape):
    from vista_amd import ops, perceptual
    n, d = shape
    rng = np.random.default_rng(n * 31 + d)
    a = (rng.standard_normal((n, d)) + 0.5).astype(np.float32)
    b = (rng.standard_normal((n, d)) + 0.5 * np.sign(a.astype(np.float64).sum(1, keepdims=True))).astype(np.float32)
    with guarded(ops):
        da, db = put(torch.from_numpy(a), label="a"), put(torch.from_numpy(b), label="b")
        got, again, same = ops.embed_row_stats(da, db), ops.embed_row_stats(da, db), ops.embed_row_stats(da, da)
        verify()
    assert got.shape == (n, 3) and got.dtype == torch.float64 and got.is_cuda
    want = R.row_stats_ref(a, b)
    err = float(np.abs(got.cpu().numpy() / want - 1.0).max())
    print(f"[parity] embed_row_stats {shape}: worst relative error against float64 {err:.3e}")
    assert err <= 1e-12, err
    assert torch.equal(got, again), "two calls, the same bits"
    s = same.cpu().numpy()
    assert np.array_equal(s[:, 0], s[:, 1]) and np.array_equal(s[:, 1], s[:, 2]), "a is b: three equal bit patterns"
    assert np.array_equal(perceptual.cosines(s), np.ones(n)), "and a cosine of exactly 1"


# ---- (c) MMD pair sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_mmd_sums_within_the_cpu_derived_bound(case):
    from vista_amd import ops
    x, y = R.make_sets(case)
    with guarded(ops):
        dx, dy = put(torch.from_numpy(x), label="x"), put(torch.from_numpy(y), label="y")
        got, again = ops.embed_mmd_sums(dx, dy, R.SIGMA), ops.embed_mmd_sums(dx, dy, R.SIGMA)
        twice = ops.embed_mmd_sums(dx, dx, R.SIGMA)
        verify()
    assert got.shape == (3,) and got.dtype == torch.float64 and got.is_cuda
    want, bound = R.mmd_sums_ref(x, y), R.mmd_bound(case)
    err = R.rel_errors(got.cpu().numpy(), want)
    print(f"[parity] embed_mmd_sums {R.case_id(case)}: sums {want[0]:.6e} {want[1]:.6e} {want[2]:.6e}, relative error against float64 "
          f"{err[0]:.2e} {err[1]:.2e} {err[2]:.2e} (bound {bound:.2e})")
    assert np.all(err <= bound), (err, bound)
    assert torch.equal(got, again), "two calls, the same bits"
    if x.shape[0] == 1:
        assert float(got[0]) == 0.0
    # x against itself: the full square is the strict triangle twice and a diagonal of zeros
    t = twice.cpu().numpy()
    assert t[0] == t[1] and R.rel_errors(t[2:], 2.0 * t[:1])[0] <= bound, t


def test_mmd_sums_of_equal_rows_are_exactly_zero_and_bad_rows_are_nan():
    from vista_amd import ops, perceptual
    row = np.random.default_rng(5).standard_normal((1, 1000)).astype(np.float32)
    with guarded(ops):
        x, y = put(torch.from_numpy(np.repeat(row, 65, 0)), label="x"), put(torch.from_numpy(np.repeat(row, 3, 0)), label="y")
        got = ops.embed_mmd_sums(x, y, R.SIGMA)
        bad = np.repeat(row, 4, 0)
        bad[1], bad[2, 7] = 0.0, np.inf
        nan = ops.embed_mmd_sums(put(torch.from_numpy(bad), label="bad"), y, R.SIGMA)
        stats = ops.embed_row_stats(put(torch.from_numpy(bad), label="bad2"), put(torch.from_numpy(np.repeat(row, 4, 0)), label="good"))
        verify()
    assert got.tolist() == [0.0, 0.0, 0.0] and not np.signbit(got.cpu().numpy()).any()
    assert math.isnan(float(nan[0])) and float(nan[1]) == 0.0 and math.isnan(float(nan[2])), "a zero row and an infinite one: NaN, no fault"
    cos = perceptual.cosines(stats.cpu().numpy())
    assert cos[0] == 1.0 and np.isnan(cos[1]) and np.isnan(cos[2]) and cos[3] == 1.0
    d = perceptual.mmd_json(perceptual.mmd_from_sums(nan.cpu().numpy(), 4, 3))
    assert d["biased"] is None and d["unbiased"] is None
    with pytest.raises(ValueError):
        ops.embed_mmd_sums(x, y, 0.0)
    with pytest.raises(ValueError):
        ops.embed_mmd_sums(x, y[:, :999].contiguous(), R.SIGMA)
    with pytest.raises(ValueError):
        ops.embed_row_stats(x, y)


# ---- embed_frames on the tiny tower ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tower():
    from vista_amd import synth
    from vista_amd.modules.encoders.modules import FrozenOpenCLIPImageEmbedder
    emb = FrozenOpenCLIPImageEmbedder(arch=dict(TINY_CLIP))
    emb.load_state_dict(synth.seeded_state_dict({k: tuple(v.shape) for k, v in emb.state_dict().items()}, 11), strict=True)
    return emb.cuda().eval()


def test_embed_frames_equals_the_towers_forward_and_is_chunked(tower):
    from vista_amd import perceptual
    n = perceptual.EMBED_CHUNK + 1
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:40, 0:52]
    frames = np.stack([np.clip(127 + 110 * np.sin(xx / (3.0 + i) + c) * np.cos(yy / (4.0 + c)) + rng.normal(0, 5, (40, 52)), 0, 255)
                       for i in range(n) for c in range(3)]).reshape(n, 3, 40, 52).transpose(0, 2, 3, 1).astype(np.uint8)
    u8 = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    got = perceptual.embed_frames(tower, u8)
    assert got.shape == (n, TINY_CLIP["embed"]) and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
    unit = _unit_frames(u8).cuda()
    want = torch.cat([tower(unit[i:i + 1]) for i in range(n)]).float()   # (one frame a call: forward runs equal frames once)
    rel = float((got - want).norm() / want.norm())
    print(f"[parity] embed_frames, {n} frames on the tiny tower: rel-L2 against forward on the converted frames {rel:.3e}")
    assert rel <= 5e-3, rel
    assert torch.equal(perceptual.embed_frames(tower, u8), got), "the same bytes, the same bits"
    # the stack is cut every EMBED_CHUNK frames: the last frame is a chunk of its own, the first EMBED_CHUNK one launch
    assert torch.equal(perceptual.embed_frames(tower, u8[-1:]), got[-1:]) and torch.equal(perceptual.embed_frames(tower, u8[:-1]), got[:-1])
    rep = perceptual.frame_scores(got, perceptual.embed_frames(tower, u8.clone()))
    assert np.array_equal(rep.sim, np.ones(n)), "equal frames: a similarity of exactly 1"
    assert np.isnan(rep.step[0]) and np.array_equal(rep.step, rep.step_real, equal_nan=True) and np.all(rep.step[1:] < 1.0)
    ref = R.frame_scores_ref(got.cpu().numpy(), got.cpu().numpy())
    assert np.allclose(rep.step[1:], ref["step"][1:], rtol=1e-12, atol=0)
    d = perceptual.mmd(got[:5], got[5:])
    w = R.mmd_ref(got[:5].cpu().numpy(), got[5:].cpu().numpy())
    # 1000 times a combination, with weights that add up to 4, of means of terms of at most 0.02 that each hold the kernel's bound (of the
    # near class: frames of one sequence)
    assert abs(d["biased"] - w["biased"]) <= 1000 * 4 * 0.02 * R.MMD_REL_BOUND_NEAR and (d["m"], d["n"]) == (5, n - 5)
    assert perceptual.tower_info(tower) == {"embed": 1024, "image": 224, "patch": 14, "sigma": 10.0, "scale": 1000.0}


# ---- the front door ----------------------------------------------------------------------------------------------------------------------------
CLIP_KEYS = ["clip_sim", "clip_step", "clip_step_real", "mean_clip_sim", "mean_clip_step", "mean_clip_step_real", "clip_mmd"]
PARENT_KEYS = ["index", "frames", "seed", "action", "n_conds", "n_rounds", "frames_scored", "psnr", "ssim", "sse", "cond", "mean_psnr", "mean_ssim",
               "rounds", "timings"]


def _clip_part(records):
    return [[r[k] for k in CLIP_KEYS] + [[x["mean_clip_sim"] for x in r["rounds"]]] for r in records]


def test_evaluate_with_the_hook_online_then_offline(world, scenes, model, monkeypatch, capsys):  # noqa: F811
    from vista_amd import evaluate, perceptual
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda spec: model)        # (the fixture's pipeline: same config, same checkpoint)
    monkeypatch.setenv("VISTA_EVAL_CLIP", "1")
    save = str(world["dir"] / "evaluate_clip")
    assert evaluate.main(_flags(world, scenes, save)) == 0
    out = capsys.readouterr().out
    assert "mean_clip_sim" in out and "clip " in out
    records = _records(save)
    assert len(records) == 2 and all(list(r) == PARENT_KEYS[:-1] + CLIP_KEYS + ["timings"] for r in records)
    assert all(sorted(r["timings"]) == ["clip", "condition", "decode", "encode", "load", "metrics", "sample", "save"] for r in records)
    for r in records:
        n = r["frames_scored"]
        assert n == T and len(r["clip_sim"]) == len(r["clip_step"]) == len(r["clip_step_real"]) == n, "one value per scored frame"
        assert r["clip_step"][0] is None and r["clip_step_real"][0] is None and all(v is not None and -1.0 <= v <= 1.0 + 1e-12 for v in r["clip_sim"])
        pred = list(range(1, n))
        for key in ("clip_sim", "clip_step", "clip_step_real"):
            assert r["mean_" + key] == math.fsum(r[key][i] for i in pred) / len(pred), "the conditioning frame is in no mean"
        assert r["clip_mmd"]["m"] == r["clip_mmd"]["n"] == n - 1 and r["clip_mmd"]["biased"] is not None and r["clip_mmd"]["unbiased"] is not None
        assert [x["mean_clip_sim"] for x in r["rounds"]] == [r["mean_clip_sim"]]
    online = json.load(open(os.path.join(save, "metrics_summary.json")))
    assert online["clip_mmd"]["m"] == online["clip_mmd"]["n"] == 2 * (T - 1), "all predicted frames of the run"
    assert online["clip"] == {"embed": 1024, "image": 224, "patch": 14, "sigma": 10.0, "scale": 1000.0}
    assert online["mean_clip_sim"] == math.fsum(r["mean_clip_sim"] for r in records) / 2
    hz = online["horizon"]
    assert hz["clip_sim"][0] is None and hz["clip_step"][0] is None
    assert hz["clip_sim"][1:] == [math.fsum(r["clip_sim"][i] for r in records) / 2 for i in range(1, T)]
    # the records' numbers are the module's on the saved pictures
    from tests.test_fidelity_gpu import _pictures
    tower = perceptual.find_tower(model)
    e_pred = perceptual.embed_frames(tower, torch.from_numpy(_pictures(save, "virtual", 1, T)).cuda())
    e_real = perceptual.embed_frames(tower, torch.from_numpy(_pictures(save, "real", 1, T)).cuda())
    rep = perceptual.frame_scores(e_pred, e_real)
    assert records[1]["clip_sim"] == rep.sim.tolist() and records[1]["clip_step"][1:] == rep.step[1:].tolist()
    assert np.allclose(rep.sim, R.cosines_ref(e_pred.cpu().numpy(), e_real.cpu().numpy()), rtol=1e-12, atol=0)
    # offline, with the tower alone from --config / --ckpt: the same bytes, the same launches, the same numbers exactly
    monkeypatch.setattr(SU, "init_model", None)   # (no pipeline is built)
    assert evaluate.main(["--compare", save, "--n_conds", "1", "--n_frames", str(T), "--action", "traj", "--config", world["config"],
                          "--ckpt", world["ckpt"]]) == 0
    offline = _records(save)
    assert _clip_part(offline) == _clip_part(records) and _per_frame(offline) == _per_frame(records)
    assert all(sorted(r["timings"]) == ["clip", "load", "metrics"] for r in offline)
    assert json.load(open(os.path.join(save, "metrics_summary.json"))) == online
    # without the hook the records are the parent's, key for key, and hold the same fidelity numbers
    monkeypatch.setattr(SU, "init_model", lambda spec: model)
    monkeypatch.delenv("VISTA_EVAL_CLIP")
    plain = str(world["dir"] / "evaluate_clip_unset")
    capsys.readouterr()
    assert evaluate.main(_flags(world, scenes, plain) + ["--no_pictures"]) == 0
    assert "clip" not in capsys.readouterr().out
    unset = _records(plain)
    assert all(list(r) == PARENT_KEYS for r in unset) and all(list(x) == ["round", "frames", "mean_psnr", "mean_ssim"] for r in unset for x in r["rounds"])
    assert all(sorted(r["timings"]) == ["condition", "decode", "encode", "load", "metrics", "sample"] for r in unset)
    fidelity_part = lambda rs: [(r["index"], r["psnr"], r["ssim"], r["sse"], r["cond"], r["mean_psnr"], r["mean_ssim"]) for r in rs]   # noqa: E731
    assert fidelity_part(unset) == fidelity_part(records)
    summary = json.load(open(os.path.join(plain, "metrics_summary.json")))
    assert list(summary) == ["scenes", "mean_psnr", "mean_ssim", "horizon"] and list(summary["horizon"]) == ["frame", "scenes", "psnr", "ssim"]
