"""Motion-JPEG output, the host side (no GPU): the tables against libjpeg's, the float64 reference (tests/_jpeg_ref.py) against Pillow's decoder and
encoder, the AVI writer against an independent struct-based parser, and the environment hook in every CLI that writes videos."""
import json
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _jpeg_ref as R  # noqa: E402

HOOKS = ("VISTA_VIDEO", "VISTA_VIDEO_QUALITY")


# ---- tables -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 100])
def test_tables_equal_what_libjpeg_writes(quality):
    from vista_amd import video
    dqt, dht = R.pillow_tables(quality)
    t = video.jpeg_tables(quality)
    assert set(dqt) == {0, 1} and set(dht) == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for i, table in enumerate(t["quant"]):
        assert tuple(table[video.ZIGZAG[k]] for k in range(64)) == dqt[i], f"quantiser table {i}"
    for key, (bits, vals) in zip(((0, 0), (1, 0), (0, 1), (1, 1)), t["huff"]):   # DC0, AC0, DC1, AC1
        assert (tuple(bits), tuple(vals)) == dht[key], key
    assert tuple(int(k) for k in R.ZZ) == video.ZIGZAG
    assert video.jpeg_header(40, 24, quality) == R.header(40, 24, quality), "the two header writers agree byte for byte"
    for bad in (0, 101, -3, 50.0, "90", True):
        with pytest.raises(ValueError, match="quality"):
            video.jpeg_tables(bad)


def test_header_segments_are_the_ones_named_and_in_order():
    from vista_amd import video
    segs, end = R.segments(video.jpeg_header(1024, 576, 90) + b"\x00")
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA] and end == len(video.jpeg_header(1024, 576, 90))
    p = dict((m, v) for m, v in segs if m != 0xC4)
    assert p[0xE0] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert len(p[0xDB]) == 130 and p[0xDB][0] == 0 and p[0xDB][65] == 1
    assert p[0xC0] == bytes([8]) + struct.pack(">HH", 576, 1024) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [v[0] for m, v in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    assert p[0xDD] == struct.pack(">H", 64) and p[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


# ---- the reference is a JPEG as the world encodes it --------------------------------------------------------------------------------------------
PICTURES = {"smooth_noise": lambda: R.smooth_noise(1, 40, 56)[0], "noise": lambda: R.noise(1, 40, 56)[0]}


@pytest.mark.parametrize("name", sorted(PICTURES))
@pytest.mark.parametrize("quality", [25, 50, 75, 90])
def test_reference_streams_decode_and_match_pillows_own_encoder(name, quality):
    frame = PICTURES[name]()
    jpeg = R.encode(frame[None], quality)[0]
    got = R.decode(jpeg)
    assert got.shape == frame.shape
    ours, theirs = R.psnr(got, frame), R.pillow_psnr(frame, quality)
    print(f"MJPEGREF {name} q={quality} bytes={len(jpeg)} psnr={ours:.3f} pillow={theirs:.3f}")
    assert ours >= theirs - 0.25


@pytest.mark.parametrize("quality", [1, 95, 100])
def test_reference_streams_decode_at_the_edges(quality):
    for frames in (R.noise(1, 1, 1), R.noise(1, 40, 1), R.checkerboard(1, 16, 16), R.mcu_checker(1, 32, 48), R.step(1, 32, 48),
                   np.zeros((1, 16, 16, 3), np.uint8), np.full((1, 16, 16, 3), 255, np.uint8), R.noise(1, 160, 16)):
        assert R.decode(R.encode(frames, quality)[0]).shape == frames.shape[1:]


def test_the_tie_share_of_a_float32_evaluation_stays_under_the_cap():
    """The condition behind the GPU test's cap of 1 %: a float32 evaluation of the reference differs from float64 in at most that share of the
    coefficients on the GPU test's inputs, only next to half-integer quotients, and by 1."""
    cases = [(R.step(1, 32, 48), 95), (R.smooth_noise(2, 24, 40), 50), (R.noise(1, 16, 16), 100), (R.checkerboard(1, 16, 16), 100)]
    for frames, q in cases:
        c64, quot = R.coefficients(frames, q)
        c32, _ = R.coefficients(frames, q, np.float32)
        d = c64 != c32
        print(f"MJPEGTIES q={q} shape={frames.shape} differ={int(d.sum())} of {d.size}")
        assert d.mean() <= 0.01
        frac = np.abs(np.abs(quot[d]) % 1.0 - 0.5)
        assert (frac < 1e-3).all() and (np.abs(c64[d].astype(int) - c32[d].astype(int)) == 1).all()
    _, quot = R.coefficients(R.step(1, 32, 48), 95)
    assert (np.abs(np.abs(quot) % 1.0 - 0.5) < 1e-9).sum() >= 4, "the step picture holds ties"


# ---- AVI ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    frames = R.smooth_noise(3, 24, 40)
    return frames, R.encode(frames, 75)


def test_avi_round_trip_and_every_pinned_field(clip, tmp_path):
    from vista_amd import video
    frames, jpegs = clip
    jpegs = [jpegs[0], jpegs[1] + b"\x00" * (1 - len(jpegs[1]) % 2), jpegs[2]]     # one odd length among them: a pad byte must follow it
    assert any(len(j) % 2 for j in jpegs)
    path = video.write_avi(str(tmp_path / "a.avi"), jpegs, 40, 24, fps=10)
    assert path.endswith("a.avi") and video.read_avi(path) == jpegs
    data = open(path, "rb").read()
    a = R.parse_avi(data)
    n = len(jpegs)
    assert a["form"] == b"AVI " and a["riff_size"] == len(data) - 8 and a["n_strl"] == 1
    assert a["avih"][0] == 100000 and a["avih"][4] == n and a["avih"][6] == 1 and a["avih"][8:10] == (40, 24) and a["avih"][3] & 0x10
    s = a["strh"]
    assert (s["type"], s["handler"], s["scale"], s["rate"], s["length"], s["size"]) == (b"vids", b"MJPG", 1, 10, n, 56) and s["frame"] == (0, 0, 40, 24)
    f = a["strf"]
    assert (f["size"], f["chunk_size"], f["width"], f["height"], f["planes"], f["bits"], f["compression"]) == (40, 40, 40, 24, 1, 24, b"MJPG")
    assert [c[0] for c in a["chunks"]] == [b"00dc"] * n and [c[2] for c in a["chunks"]] == [len(j) for j in jpegs]
    assert all(at % 2 == 0 for _, at, _ in a["chunks"])
    assert a["idx1"] == [(b"00dc", 0x10, at - a["movi_at"], size) for _, at, size in a["chunks"]]
    for (_, at, size), j in zip(a["chunks"], jpegs):
        assert data[at + 8:at + 8 + size] == j
    assert R.parse_avi(open(video.write_avi(str(tmp_path / "b.avi"), jpegs, 40, 24, fps=3), "rb").read())["avih"][0] == 333333


def test_read_video_frames_decodes_an_avi_to_the_references_frames(clip, tmp_path):
    from vista_amd import sample_utils as SU
    from vista_amd import video
    frames, jpegs = clip
    path = video.write_avi(str(tmp_path / "clip.avi"), jpegs, 40, 24)
    got = SU.read_video_frames(path)
    assert got.dtype == np.uint8 and got.shape == frames.shape
    assert np.array_equal(got, np.stack([R.decode(j) for j in jpegs]))


def test_a_file_beyond_two_gib_is_refused_before_anything_is_written(tmp_path):
    from vista_amd import video

    class Big(bytes):
        def __len__(self):
            return 2 ** 30
    path = str(tmp_path / "big.avi")
    with pytest.raises(ValueError, match=r"big\.avi would take \d+ bytes.*2\^31 - 1"):
        video.write_avi(path, [Big(), Big()], 1024, 576)
    assert not os.path.exists(path)
    with pytest.raises(ValueError, match="no frames"):
        video.write_avi(path, [], 16, 16)
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        (tmp_path / "x.avi").write_bytes(b"RIFX0000AVI ")
        video.read_avi(str(tmp_path / "x.avi"))


# ---- the hook -----------------------------------------------------------------------------------------------------------------------------------
def test_video_format_reads_the_two_hooks(monkeypatch):
    from vista_amd import sample_utils as SU
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    assert SU.video_format() == ("apng", 90)
    monkeypatch.setenv("VISTA_VIDEO", "")
    assert SU.video_format() == ("apng", 90)
    monkeypatch.setenv("VISTA_VIDEO", "mjpeg")
    monkeypatch.setenv("VISTA_VIDEO_QUALITY", "1")
    assert SU.video_format() == ("mjpeg", 1)
    monkeypatch.setenv("VISTA_VIDEO_QUALITY", "100")
    assert SU.video_format() == ("mjpeg", 100)
    monkeypatch.setenv("VISTA_VIDEO", "apng")
    assert SU.video_format() == ("apng", 100)


@pytest.mark.parametrize("env,match", [({"VISTA_VIDEO": "webm"}, "Unknown video format webm.*VISTA_VIDEO"),
                                       ({"VISTA_VIDEO": "mjpeg", "VISTA_VIDEO_QUALITY": "0"}, "Bad JPEG quality 0.*VISTA_VIDEO_QUALITY"),
                                       ({"VISTA_VIDEO_QUALITY": "101"}, "Bad JPEG quality 101.*VISTA_VIDEO_QUALITY"),
                                       ({"VISTA_VIDEO": "mjpeg", "VISTA_VIDEO_QUALITY": "abc"}, "Bad JPEG quality abc.*VISTA_VIDEO_QUALITY")])
def test_every_cli_that_writes_videos_refuses_a_bad_hook_before_building_anything(env, match, monkeypatch, tmp_path):
    from vista_amd import drive, evaluate, plan, reward, sample
    from vista_amd import sample_utils as SU
    monkeypatch.setattr(SU, "init_model", lambda *a, **k: pytest.fail("the model must not be built for a refused video format"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cand = tmp_path / "c.json"
    cand.write_text(json.dumps({"candidates": [{}, {"command": 1}]}))
    small = ["--height", "128", "--width", "256", "--n_frames", "5"]
    for module, argv in ((sample, small), (reward, small), (evaluate, small), (drive, small), (plan, small + ["--candidates", str(cand)])):
        with pytest.raises(ValueError, match=match):
            module.main(argv)


def _parents_save_video(path_stem, frames_u8, fps=10):
    """save_video's animated-PNG branch as it stood before the hook existed."""
    from PIL import Image
    path = path_stem + ".apng"
    images = [Image.fromarray(f) for f in frames_u8]
    images[0].save(path, format="PNG", save_all=True, append_images=images[1:], duration=int(round(1000 / fps)), loop=0,
                   disposal=[i & 1 for i in range(len(images))], blend=0)
    return path


def test_with_the_hook_unset_save_video_writes_the_parents_bytes(monkeypatch, tmp_path):
    from vista_amd import sample_utils as SU
    monkeypatch.setitem(sys.modules, "imageio", None)    # (where imageio is importable the unset hook writes an mp4 through it, as before)
    frames = R.smooth_noise(4, 24, 40)
    frames[2] = frames[1]                                # (a repeated frame: the disposal trick is part of the bytes)
    for value in (None, "apng"):
        monkeypatch.delenv("VISTA_VIDEO", raising=False)
        if value:
            monkeypatch.setenv("VISTA_VIDEO", value)
        got = SU.save_video(str(tmp_path / f"got{value}"), frames, 10)
        want = _parents_save_video(str(tmp_path / f"want{value}"), frames, 10)
        assert got.endswith(".apng") and open(got, "rb").read() == open(want, "rb").read()
        assert np.array_equal(SU.read_video_frames(got), frames)
