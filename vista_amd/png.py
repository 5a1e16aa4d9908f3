"""PNG output whose pixel data is coded on the GPU (csrc/png.hip through ops.png_filter / ops.png_deflate), and this package's own PNG and APNG
writers. No dependency beyond torch and numpy; Pillow is used by `pipeline.read_video_frames` to decode only.

A picture is an 8-bit RGB PNG (colour type 2, no interlace): signature, IHDR, ONE IDAT, IEND. The IDAT payload is a zlib stream: the fixed header
ZLIB_HEADER, the deflate data -- per segment of SEG_ROWS filtered rows one dynamic-Huffman block, zlib's Z_RLE tokens (literals and distance-1 runs)
-- and the Adler-32. The rows are filtered, tokenised, Huffman-coded and written by the GPU. Two things run on the HOST: the frame's Adler-32 is
combined from the per-segment sums the GPU computed (adler32_combine), and the chunk CRCs come from zlib.crc32. An animated PNG holds the same
streams: acTL, then per frame fcTL and IDAT (the first) or fdAT, full frames, no blending. Not built: general LZ77 (distances other than 1),
stored blocks for incompressible segments, 16-bit / palette / alpha / interlaced pictures, decoding.
"""
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x01"   # CM 8 (deflate), CINFO 7 (32 KiB window), FLEVEL 0 (fastest: no match search), FDICT 0, FCHECK 1: 0x7801 = 31 * 991
SEG_ROWS = 16
ADLER_BASE = 65521


def adler32_combine(adler1, adler2, len2):
    """The Adler-32 of A + B from the Adler-32 of A, that of B alone and B's length. With s1 = 1 + sum of bytes and s2 = the sum of the running
    s1 values (both mod 65521): s1(AB) = s1(A) + s1(B) - 1, s2(AB) = s2(A) + s2(B) + len(B) * (s1(A) - 1)."""
    s1a, s2a, s1b, s2b = adler1 & 0xFFFF, (adler1 >> 16) & 0xFFFF, adler2 & 0xFFFF, (adler2 >> 16) & 0xFFFF
    s1 = (s1a + s1b - 1) % ADLER_BASE
    s2 = (s2a + s2b + (len2 % ADLER_BASE) * (s1a - 1)) % ADLER_BASE
    return (s2 << 16) | s1


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def _ihdr(width, height):
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))


def _frames(frames_u8, who):
    """-> the frames as (n, H, W, 3): one (H, W, 3) picture becomes a batch of one; numpy stays numpy here (zlib_streams uploads it)."""
    if not hasattr(frames_u8, "shape") or not hasattr(frames_u8, "dtype"):
        raise ValueError(f"{who}: expected a uint8 GPU tensor or numpy array, got {type(frames_u8).__name__}")
    if len(frames_u8.shape) == 3 and frames_u8.shape[2] == 3:
        frames_u8 = frames_u8[None]
    if len(frames_u8.shape) != 4 or frames_u8.shape[3] != 3 or "uint8" not in str(frames_u8.dtype):
        raise ValueError(f"{who}: expected (n, H, W, 3) uint8 frames, got {tuple(frames_u8.shape)} {frames_u8.dtype}")
    return frames_u8


def zlib_streams(frames_u8):
    """(n, H, W, 3) uint8 frames -- a GPU tensor, taken where it lies, or a numpy array, uploaded -- -> n zlib streams (bytes) of the frames'
    filtered rows. The deflate data and the per-segment Adler sums are the GPU's; the streams' bytes come to the host in one transfer."""
    import torch
    from . import ops
    frames_u8 = _frames(frames_u8, "zlib_streams")
    if not torch.is_tensor(frames_u8):
        import numpy as np
        frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8)).cuda()
    n, H, W, _ = frames_u8.shape
    row_bytes = 1 + 3 * W
    stream, offsets, adler = ops.png_deflate(ops.png_filter(frames_u8), SEG_ROWS)
    data = stream.cpu().numpy().tobytes()
    offsets, adler = offsets.tolist(), adler.tolist()
    segs = (H + SEG_ROWS - 1) // SEG_ROWS
    out = []
    for i in range(n):
        total = 1
        for k in range(segs):
            s1, s2 = adler[i * segs + k]
            total = adler32_combine(total, (s2 << 16) | s1, min(SEG_ROWS, H - k * SEG_ROWS) * row_bytes)
        out.append(ZLIB_HEADER + data[offsets[i * segs]:offsets[(i + 1) * segs]] + struct.pack(">I", total))
    return out


def encode_png(frames_u8):
    """(n, H, W, 3) uint8 frames (or one (H, W, 3) picture) -> n complete PNG files (bytes): signature, IHDR, one IDAT, IEND."""
    frames_u8 = _frames(frames_u8, "encode_png")
    H, W = int(frames_u8.shape[1]), int(frames_u8.shape[2])
    head, tail = SIGNATURE + _ihdr(W, H), _chunk(b"IEND", b"")
    return [head + _chunk(b"IDAT", z) + tail for z in zlib_streams(frames_u8)]


def write_apng(path, frames_u8, fps=10):
    """(t, H, W, 3) uint8 frames -> an animated PNG at `path`: IHDR, acTL (t frames, looping for ever), then per frame fcTL (the full frame at
    1000 / fps ms, dispose none, blend source) and its stream -- IDAT for the first, fdAT for the others, sequence numbers running over fcTL and
    fdAT --, IEND. Every frame is a frame of its own: a still clip reads back with all its frames. Returns the path."""
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or fps <= 0:
        raise ValueError(f"write_apng: fps must be positive, got {fps!r}")
    frames_u8 = _frames(frames_u8, "write_apng")
    n, H, W = int(frames_u8.shape[0]), int(frames_u8.shape[1]), int(frames_u8.shape[2])
    if n < 1:
        raise ValueError("write_apng: no frames")
    out, seq = [SIGNATURE, _ihdr(W, H), _chunk(b"acTL", struct.pack(">II", n, 0))], 0
    for i, z in enumerate(zlib_streams(frames_u8)):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, int(round(1000 / fps)), 1000, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_chunk(b"IDAT", z))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + z))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return path
