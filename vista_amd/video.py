"""Motion-JPEG video output: baseline JPEG frames whose scans come from the GPU (csrc/jpeg.hip through ops.jpeg_dct_quant / ops.jpeg_entropy), and
this package's own AVI writer and reader. No dependency beyond torch and numpy; Pillow is used by `pipeline.read_video_frames` to decode only.

A frame is a baseline sequential JFIF file (ITU-T T.81): 8 bit, YCbCr 4:2:0, the Annex K "typical" quantiser tables scaled by libjpeg's quality
rule, the Annex K Huffman tables, one restart interval per MCU row. A video is a plain RIFF `AVI ` with one `vids` / `MJPG` stream, one `00dc`
chunk per frame and an `idx1` index in which every frame is a key frame -- the common MJPG-in-AVI layout. Not built: audio, 4:4:4 or 4:2:2
sampling, optimised Huffman tables, progressive JPEG, files of 2 GiB and more (OpenDML), mp4 / H.264.
"""
import struct

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# T.81 Annex K, tables K.1 and K.2 (row-major)
_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# T.81 Annex K, tables K.3 - K.6: BITS (the number of codes of each length 1 .. 16) and HUFFVAL
_DC_VALS = tuple(range(12))
_DC0_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
_DC1_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
_AC0_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)
_AC1_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
_AC0_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC1_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")

MAX_AVI_BYTES = 2 ** 31 - 1


def check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality must be an integer from 1 to 100, got {quality!r}")
    return quality


def jpeg_tables(quality):
    """-> {"quant": (luma, chroma), "huff": ((bits, huffval) for DC0, AC0, DC1, AC1)}. The quantiser tables are 64 ints in row-major order: Annex K
    scaled by libjpeg's rule, s = 5000 // q below 50 else 200 - 2 q, Q = clamp((base * s + 50) // 100, 1, 255). The Huffman tables are Annex K's."""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    quant = tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (_LUMA, _CHROMA))
    huff = ((_DC0_BITS, _DC_VALS), (_AC0_BITS, tuple(_AC0_VALS)), (_DC1_BITS, _DC_VALS), (_AC1_BITS, tuple(_AC1_VALS)))
    return {"quant": quant, "huff": huff}


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(width, height, quality):
    """Everything of a frame's file in front of its scan: SOI, APP0 (JFIF 1.01, no units, 1:1), one DQT with both tables (8 bit, zigzag order), SOF0
    (Y 2x2 table 0, Cb and Cr 1x1 table 1), DHT x 4 (DC0, AC0, DC1, AC1), DRI (one MCU row), SOS (Ss 0, Se 63)."""
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"a JPEG frame is 1 .. 65535 pixels wide and high, got {width} x {height}")
    t = jpeg_tables(quality)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    out.append(_segment(0xDB, b"".join(bytes([i]) + bytes(tab[ZIGZAG[k]] for k in range(64)) for i, tab in enumerate(t["quant"]))))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), t["huff"]):
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", (width + 15) // 16)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def encode_jpeg(frames_u8, quality=90):
    """(n, H, W, 3) uint8 frames -- a GPU tensor, taken where it lies, or a numpy array, uploaded -- -> n complete JFIF files (bytes). The scans
    are coded on the GPU (ops.jpeg_dct_quant, ops.jpeg_entropy); their bytes and byte counts come to the host in one transfer each."""
    import torch
    from . import ops
    check_quality(quality)
    if not torch.is_tensor(frames_u8):
        import numpy as np
        arr = np.ascontiguousarray(frames_u8)
        if arr.dtype != np.uint8:
            raise ValueError(f"encode_jpeg: frames must be uint8, got {arr.dtype}")
        frames_u8 = torch.from_numpy(arr).cuda()
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"encode_jpeg: expected (n, H, W, 3) uint8 frames, got {tuple(frames_u8.shape)}")
    n, H, W, _ = frames_u8.shape
    mcu_h, mcu_w = (H + 15) // 16, (W + 15) // 16
    coef = ops.jpeg_dct_quant(frames_u8, quality)
    scan, offsets = ops.jpeg_entropy(coef, mcu_h, mcu_w)
    data = scan.cpu().numpy().tobytes()
    header = jpeg_header(W, H, quality)
    return [header + data[offsets[i * mcu_h]:offsets[(i + 1) * mcu_h]] + b"\xff\xd9" for i in range(n)]


# ---- AVI --------------------------------------------------------------------------------------------------------------------------------------
def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def _list(kind, payload):
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


def write_avi(path, jpegs, width, height, fps=10):
    """A list of JPEG files (bytes) -> a RIFF `AVI ` at `path`: hdrl (avih; one strl: strh vids / MJPG, scale 1, rate fps; strf BITMAPINFOHEADER,
    MJPG, 24 bit), movi (one `00dc` chunk per frame, padded to even length), idx1 (every frame a key frame, offsets relative to `movi`). A file
    of more than 2^31 - 1 bytes is refused before anything is written. Returns the path."""
    if not jpegs:
        raise ValueError("write_avi: no frames")
    if isinstance(fps, bool) or not isinstance(fps, int) or fps < 1:
        raise ValueError(f"write_avi: fps must be a positive integer (the stream's rate over a scale of 1), got {fps!r}")
    n = len(jpegs)
    padded = [len(j) + (len(j) & 1) for j in jpegs]
    biggest = min(max(len(j) for j in jpegs), 0xFFFFFFFF)   # (a frame that large is refused below, by the file's size)
    avih = struct.pack("<14I", int(round(1e6 / fps)), min(biggest * fps, 0xFFFFFFFF), 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)   # 0x10: AVIF_HASINDEX
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, fps, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi_bytes = 4 + sum(8 + p for p in padded)
    total = 12 + len(hdrl) + 8 + movi_bytes + 8 + 16 * n
    if total > MAX_AVI_BYTES:
        raise ValueError(f"write_avi: {path} would take {total} bytes; a plain AVI holds at most 2^31 - 1 (OpenDML is not built): write fewer frames "
                         "per file or lower VISTA_VIDEO_QUALITY")
    index, at = [], 4                                   # offsets count from the `movi` fourcc
    for j, p in zip(jpegs, padded):
        index.append(b"00dc" + struct.pack("<III", 0x10, at, len(j)))   # 0x10: AVIIF_KEYFRAME
        at += 8 + p
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI ")
        f.write(hdrl)
        f.write(b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        for j in jpegs:
            f.write(_chunk(b"00dc", j))
        f.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(index))
    return path


def read_avi(path):
    """The `00dc` chunks of an AVI's `movi` list, in file order -> a list of bytes (the JPEG files write_avi was given)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    frames = []

    def walk(at, end, in_movi):
        while at + 8 <= end:
            fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
            body = at + 8
            if body + size > end:
                raise ValueError(f"{path}: chunk {fourcc!r} at {at} runs past its container")
            if fourcc == b"LIST":
                walk(body + 4, body + size, data[body:body + 4] == b"movi")
            elif in_movi and fourcc == b"00dc":
                frames.append(data[body:body + size])
            at = body + size + (size & 1)

    walk(12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0]), False)
    return frames
