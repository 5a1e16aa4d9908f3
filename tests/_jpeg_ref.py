"""An independent restatement of the Motion-JPEG output path, written for the tests: plain numpy / Python, float64 unless asked otherwise.

  coefficients(frames, quality)  colour conversion, edge-replicated padding, 2 x 2 chroma means, level shift, 8 x 8 DCT-II, quantiser
                                 -> (int16 coefficients (n, blocks, 64) in zigzag order, the unrounded quotients)
  intervals(coef, mcu_h, mcu_w)  a bit-serial Huffman coder: per restart interval the stuffed, 1-padded bytes and the RSTm marker
  jpeg_file(...)                 headers + scan + EOI
  parse_avi(bytes)               a struct-based RIFF walk that returns every field the tests pin
  psnr, decode                   Pillow decodes; nothing here encodes with it

It shares no code and no table with vista_amd/video.py or csrc/jpeg.hip: the quantiser base tables are typed from T.81 Annex K.1 / K.2 in the
rows of the standard, and the Huffman tables are read out of a JPEG that Pillow (libjpeg) writes with optimize=False -- the tables the world's
decoders call "typical"."""
import functools
import io
import struct

import numpy as np

K1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
               [12, 12, 14, 19, 26, 58, 60, 55],
               [14, 13, 16, 24, 40, 57, 69, 56],
               [14, 17, 22, 29, 51, 87, 80, 62],
               [18, 22, 37, 56, 68, 109, 103, 77],
               [24, 35, 55, 64, 81, 104, 113, 92],
               [49, 64, 78, 87, 103, 121, 120, 101],
               [72, 92, 95, 98, 112, 100, 103, 99]])
K2 = np.full((8, 8), 99)
K2[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def zigzag_order():
    """Natural index of zigzag position k, walked along the anti-diagonals (T.81 figure A.6)."""
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += [y * 8 + x for y, x in (cells if s % 2 else reversed(cells))]
    return np.array(order)


ZZ = zigzag_order()


def quant_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (K1, K2))


def segments(jpeg):
    """[(marker, payload)] of a JPEG file's header segments up to and including SOS."""
    out, at = [], 2
    assert jpeg[:2] == b"\xff\xd8"
    while True:
        assert jpeg[at] == 0xFF, at
        marker, size = jpeg[at + 1], struct.unpack_from(">H", jpeg, at + 2)[0]
        out.append((marker, jpeg[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xDA:
            return out, at


def pillow_tables(quality):
    """(DQT payloads {id: 64 zigzag bytes}, DHT payloads {(class, id): (bits, huffval)}) of what Pillow writes at `quality`, 4:2:0, optimize=False."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", quality=quality, optimize=False, subsampling=2)
    dqt, dht = {}, {}
    for marker, p in segments(buf.getvalue())[0]:
        at = 0
        while marker == 0xDB and at < len(p):
            assert p[at] >> 4 == 0
            dqt[p[at] & 15] = tuple(p[at + 1:at + 65])
            at += 65
        while marker == 0xC4 and at < len(p):
            bits = tuple(p[at + 1:at + 17])
            dht[(p[at] >> 4, p[at] & 15)] = (bits, tuple(p[at + 17:at + 17 + sum(bits)]))
            at += 17 + sum(bits)
    return dqt, dht


@functools.lru_cache(maxsize=None)
def huffman_codes():
    """{(class, id): {symbol: (code, length)}} from libjpeg's standard tables, codes assigned as T.81 Annex C."""
    out = {}
    for key, (bits, vals) in pillow_tables(75)[1].items():
        code, k, table = 0, 0, {}
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                table[vals[k]] = (code, length)
                code += 1
                k += 1
            code *= 2
        out[key] = table
    return out


# ---- stage A ----------------------------------------------------------------------------------------------------------------------------------
def dct_matrix(dtype=np.float64):
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    m = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    m[0] /= np.sqrt(2.0)
    return m.astype(dtype)


def coefficients(frames, quality, dtype=np.float64):
    """frames (n, H, W, 3) uint8 -> (coef int16 (n, 6 mcu_h mcu_w, 64), quotient `dtype` of the same shape): zigzag order, blocks in scan order."""
    f = dtype
    n, H, W, _ = frames.shape
    mh, mw = -(-H // 16), -(-W // 16)
    x = np.pad(frames, ((0, 0), (0, mh * 16 - H), (0, mw * 16 - W), (0, 0)), mode="edge").astype(f)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Y = f(0.299) * R + f(0.587) * G + f(0.114) * B
    Cb = f(-0.168736) * R - f(0.331264) * G + f(0.5) * B + f(128)
    Cr = f(0.5) * R - f(0.418688) * G - f(0.081312) * B + f(128)
    sub = lambda p: p.reshape(n, mh * 8, 2, mw * 8, 2).mean(axis=(2, 4), dtype=f)   # noqa: E731
    m = dct_matrix(f)
    ql, qc = (t.reshape(64)[ZZ].astype(f) for t in quant_tables(quality))

    def blocks(plane, by, bx):     # (n, by * 8, bx * 8) -> (n, by, bx, 64) quotients before the division, zigzag order
        b = (plane - f(128)).reshape(n, by, 8, bx, 8).transpose(0, 1, 3, 2, 4)
        return np.einsum("vy,nabyx,ux->nabvu", m, b, m).reshape(n, by, bx, 64)[..., ZZ]
    y = blocks(Y, mh * 2, mw * 2) / ql
    cb, cr = blocks(sub(Cb), mh, mw) / qc, blocks(sub(Cr), mh, mw) / qc
    y = y.reshape(n, mh, 2, mw, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(n, mh, mw, 4, 64)
    quot = np.concatenate([y, cb[:, :, :, None], cr[:, :, :, None]], axis=3).reshape(n, mh * mw * 6, 64)
    r = np.sign(quot) * np.floor(np.abs(quot) + f(0.5))        # half away from zero
    r[..., 0] = np.clip(r[..., 0], -1024, 1023)
    r[..., 1:] = np.clip(r[..., 1:], -1023, 1023)
    return r.astype(np.int16), quot


# ---- stage B: bit-serial ------------------------------------------------------------------------------------------------------------------------
def _value_bits(v):
    size = int(abs(v)).bit_length()
    return size, (format(v if v >= 0 else v + (1 << size) - 1, f"0{size}b") if size else "")


def block_bits(block, pred, dc, ac):
    size, extra = _value_bits(int(block[0]) - pred)
    code, length = dc[size]
    out = [format(code, f"0{length}b"), extra]
    run = 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(format(ac[0xF0][0], f"0{ac[0xF0][1]}b"))
            run -= 16
        size, extra = _value_bits(v)
        code, length = ac[run * 16 + size]
        out += [format(code, f"0{length}b"), extra]
        run = 0
    if run:
        out.append(format(ac[0][0], f"0{ac[0][1]}b"))
    return "".join(out)


def intervals(coef, mcu_h, mcu_w):
    """coef (6 mcu_h mcu_w, 64) of ONE frame -> a list of mcu_h byte strings: each restart interval's data, stuffed, its last byte padded with
    1-bits, followed by RSTm (m = row mod 8) for every row but the last."""
    h = huffman_codes()
    out = []
    for row in range(mcu_h):
        pred, bits = [0, 0, 0], []
        for mcu in range(mcu_w):
            for k in range(6):
                comp = 0 if k < 4 else k - 3
                block = coef[(row * mcu_w + mcu) * 6 + k]
                bits.append(block_bits(block, pred[comp], h[(0, min(comp, 1))], h[(1, min(comp, 1))]))
                pred[comp] = int(block[0])
        s = "".join(bits)
        s += "1" * (-len(s) % 8)
        data = bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8)).replace(b"\xff", b"\xff\x00")
        out.append(data + (bytes([0xFF, 0xD0 + row % 8]) if row < mcu_h - 1 else b""))
    return out


def header(width, height, quality):
    seg = lambda marker, p: bytes([0xFF, marker]) + struct.pack(">H", len(p) + 2) + p   # noqa: E731
    dqt = b"".join(bytes([i]) + bytes(int(v) for v in t.reshape(64)[ZZ]) for i, t in enumerate(quant_tables(quality)))
    parts = [b"\xff\xd8", seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"), seg(0xDB, dqt),
             seg(0xC0, b"\x08" + struct.pack(">HH", height, width) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")]
    dht = pillow_tables(75)[1]
    for key in ((0, 0), (1, 0), (0, 1), (1, 1)):
        parts.append(seg(0xC4, bytes([key[0] * 16 + key[1]]) + bytes(dht[key][0]) + bytes(dht[key][1])))
    parts += [seg(0xDD, struct.pack(">H", -(-width // 16))), seg(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")]
    return b"".join(parts)


def jpeg_file(coef, width, height, quality):
    """One frame's coefficients (blocks, 64) -> the complete JFIF file."""
    return header(width, height, quality) + b"".join(intervals(coef, -(-height // 16), -(-width // 16))) + b"\xff\xd9"


def encode(frames, quality):
    coef, _ = coefficients(frames, quality)
    return [jpeg_file(c, frames.shape[2], frames.shape[1], quality) for c in coef]


def decode(jpeg):
    from PIL import Image
    with Image.open(io.BytesIO(jpeg)) as im:
        im.load()
        return np.array(im.convert("RGB"), dtype=np.uint8)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def pillow_psnr(frame, quality):
    """PSNR of Pillow's own encoder on `frame` (4:2:0, optimize=False)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, optimize=False, subsampling=2)
    return psnr(decode(buf.getvalue()), frame)


# ---- AVI ----------------------------------------------------------------------------------------------------------------------------------------
def parse_avi(data):
    """A RIFF walk with struct alone -> dict: riff_size, form, avih (14 dwords), strh (dict), strf (dict), chunks [(offset of the chunk header in
    the file, length)], movi_at (offset of the `movi` fourcc), idx1 [(fourcc, flags, offset, length)], n_strl."""
    out = {"chunks": [], "idx1": [], "n_strl": 0}
    tag, out["riff_size"], out["form"] = struct.unpack_from("<4sI4s", data, 0)
    assert tag == b"RIFF"

    def walk(at, end, where):
        while at < end:
            fourcc, size = struct.unpack_from("<4sI", data, at)
            body = at + 8
            assert body + size <= end, (fourcc, at)
            if fourcc == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    out["movi_at"] = body
                if kind == b"strl":
                    out["n_strl"] += 1
                walk(body + 4, body + size, kind)
            elif fourcc == b"avih":
                out["avih"] = struct.unpack_from("<14I", data, body)
                assert size == 56
            elif fourcc == b"strh":
                v = struct.unpack_from("<4s4sIHHIIIIIIII4h", data, body)
                out["strh"] = dict(zip(("type", "handler", "flags", "priority", "language", "initial", "scale", "rate", "start", "length", "buffer",
                                        "quality", "sample_size"), v[:13]), frame=v[13:], size=size)
            elif fourcc == b"strf":
                v = struct.unpack_from("<IiiHH4sIiiII", data, body)
                out["strf"] = dict(zip(("size", "width", "height", "planes", "bits", "compression", "image_bytes"), v[:7]), chunk_size=size)
            elif fourcc == b"idx1":
                out["idx1"] = [struct.unpack_from("<4sIII", data, body + 16 * i) for i in range(size // 16)]
            elif where == b"movi":
                out["chunks"].append((fourcc, at, size))
            at = body + size + (size & 1)
        assert at == end or at == end + 1, (where, at, end)
    walk(12, 8 + out["riff_size"], b"AVI ")
    return out


# ---- test pictures ------------------------------------------------------------------------------------------------------------------------------
def smooth_noise(n, H, W, seed=0):
    """Frames with different content: low-frequency colour gradients plus mild noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        ph = rng.uniform(0, 6.28, 6)
        base = [127 + 90 * np.sin(x / (7.0 + c + i) + ph[c]) * np.cos(y / (5.0 + 2 * c) + ph[3 + c]) for c in range(3)]
        out.append(np.clip(np.stack(base, -1) + rng.normal(0, 6, (H, W, 3)), 0, 255))
    return np.stack(out).astype(np.uint8)


def noise(n, H, W, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def checkerboard(n, H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, 3).repeat(n, 0)


def mcu_checker(n, H, W):
    """MCUs alternating black and white: DC differences of +-2040 / Q."""
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((((x >> 4) + (y >> 4)) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, 3).repeat(n, 0)


def step(n, H, W):
    """A grey vertical edge three pixels into a block (W // 2 a multiple of 8). At quality 95 the luminance DC quantiser is 2, so a block's DC
    quotient is (sum of its 64 levels - 8192) / 16: the edge blocks hold 8 (3 * 41 + 5 * 200) = 8984, quotient 49.5 -- a tie in every one."""
    out = np.full((n, H, W, 3), 41, np.uint8)
    out[:, :, W // 2 + 3:] = 200
    return out
