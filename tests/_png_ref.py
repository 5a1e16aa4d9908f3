"""A plain Python / numpy restatement of the PNG coder of csrc/png.hip: the filter choice, the Z_RLE tokens, the length-limited Huffman construction,
the run-length coded tree description and the bit stream, exactly as include/vista_hip.h states them. The GPU tests compare the kernels with this
byte for byte; the CPU tests let zlib's inflate and Pillow's PNG reader judge it. Nothing here imports vista_amd.

A frame's zlib stream: ZLIB_HEADER, then per segment of `seg_rows` filtered rows ONE dynamic-Huffman block (BFINAL on the frame's last) followed,
on every segment but the last, by an empty stored block that pads to a byte -- every segment starts on a byte boundary --, then the Adler-32."""
import struct
import zlib

import numpy as np

ZLIB_HEADER = b"\x78\x01"         # CM 8, 32 KiB window, FLEVEL 0 ("fastest": no match search), FCHECK 1: 0x7801 = 31 * 991
SIGNATURE = b"\x89PNG\r\n\x1a\n"
ADLER = 65521
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- filter -----------------------------------------------------------------------------------------------------------------------------------
def filter_rows(frames):
    """frames (n, H, W, 3) uint8 -> rows (n, H, 1 + 3 W) uint8: per row the filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; bpp 3; the row
    above a frame's first is zero) with the smallest sum of |byte as int8|, the lowest type on a tie, followed by the filtered bytes."""
    n, H, W, _ = frames.shape
    cur = frames.reshape(n, H, 3 * W).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, :, 3:] = cur[:, :, :-3]
    b = np.zeros_like(cur)
    b[:, 1:] = cur[:, :-1]
    c = np.zeros_like(cur)
    c[:, :, 3:] = b[:, :, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cands = np.stack([cur, cur - a, cur - b, cur - ((a + b) >> 1), cur - paeth]) & 255          # (5, n, H, 3 W)
    cost = np.where(cands < 128, cands, 256 - cands).sum(-1)                                   # (5, n, H)
    best = cost.argmin(0)                                                                      # (argmin: the first, so the lowest type, on a tie)
    out = np.empty((n, H, 1 + 3 * W), np.uint8)
    out[:, :, 0] = best
    out[:, :, 1:] = np.take_along_axis(cands, best[None, :, :, None], 0)[0]
    return out


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------------
def tokens(data):
    """bytes of ONE segment -> [(0, byte) | (1, length)]: at position i >= 1, if bytes i, i + 1, i + 2 equal byte i - 1, a match of distance 1 and
    length min(rest of the run, 258); otherwise a literal."""
    out, i, n = [], 0, len(data)
    while i < n:
        if i >= 1 and i + 2 < n and data[i] == data[i - 1] and data[i + 1] == data[i - 1] and data[i + 2] == data[i - 1]:
            m = 3
            while m < 258 and i + m < n and data[i + m] == data[i - 1]:
                m += 1
            out.append((1, m))
            i += m
        else:
            out.append((0, data[i]))
            i += 1
    return out


def length_symbol(m):
    """match length 3 .. 258 -> (literal/length symbol, extra bits, extra value)"""
    k = max(j for j in range(29) if LEN_BASE[j] <= m)
    return 257 + k, LEN_EXTRA[k], m - LEN_BASE[k]


# ---- code construction ------------------------------------------------------------------------------------------------------------------------
def code_lengths(freq, limit):
    """The builder's rule, a pure function of the histogram. Fewer than two used symbols: symbols 0, then 1, are counted once until two are.
    Repeat: sort the used symbols by (count, symbol) ascending; Huffman by two queues (leaves in that order, internal nodes in order of creation),
    taking the lighter front each time and the LEAF on a tie; a symbol's length is its leaf's depth. If the longest exceeds `limit`, every used
    count becomes (count + 1) >> 1 and the construction is repeated."""
    f = [int(v) for v in freq]
    for s in (0, 1):
        if sum(1 for v in f if v) < 2 and f[s] == 0:
            f[s] = 1
    while True:
        order = sorted((s for s in range(len(f)) if f[s]), key=lambda s: (f[s], s))
        m = len(order)
        lw = [f[s] for s in order]
        iw, leaf_parent, node_parent = [], [0] * m, [0] * (m - 1)
        li = ni = 0
        for k in range(m - 1):
            w = 0
            for _ in range(2):
                if li < m and (ni >= len(iw) or lw[li] <= iw[ni]):
                    w += lw[li]
                    leaf_parent[li] = k
                    li += 1
                else:
                    w += iw[ni]
                    node_parent[ni] = k
                    ni += 1
            iw.append(w)
        depth = [0] * (m - 1)
        for k in range(m - 3, -1, -1):
            depth[k] = depth[node_parent[k]] + 1
        lengths = [0] * len(f)
        for i, s in enumerate(order):
            lengths[s] = depth[leaf_parent[i]] + 1
        if max(lengths) <= limit:
            return lengths
        f = [(v + 1) >> 1 for v in f]


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> the codes, MSB first, as ints"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


def tree_symbols(lengths):
    """The code-length sequence -> [(symbol, extra bits, extra value)]. A run of r zeros: 18 (11 .. 138) while r >= 11, then 17 (3 .. 10) if r >= 3,
    else r times 0. A run of r equal lengths v > 0: v, then 16 (3 .. 6) while at least 3 remain, then v for each that is left."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, r = lengths[i], 1
        while i + r < n and lengths[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, 7, k - 11))
                r -= k
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, 2, k - 3))
                r -= k
            out += [(v, 0, 0)] * r
    return out


# ---- the bit stream ---------------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.bits = []

    def put(self, value, n):          # n bits, least significant first
        self.bits += [(value >> k) & 1 for k in range(n)]

    def code(self, code, n):          # a Huffman code: most significant bit first
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]

    def pad(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        return np.packbits(np.array(self.bits, np.uint8), bitorder="little").tobytes()


def segment_tables(data):
    """ONE segment's bytes -> dict: the tokens, the two histograms and every table of its dynamic block."""
    toks = tokens(data)
    lit_hist, n_match = [0] * 286, 0
    for kind, v in toks:
        if kind:
            lit_hist[length_symbol(v)[0]] += 1
            n_match += 1
        else:
            lit_hist[v] += 1
    lit_hist[256] = 1
    lit_len = code_lengths(lit_hist, 15)
    dist_len = 1 if n_match else 0        # the one distance code (distance 1) when a run exists; a single zero length when none does
    hlit = max(s for s in range(286) if lit_len[s]) + 1
    tree = tree_symbols(lit_len[:hlit]) + [(dist_len, 0, 0)]
    cl_hist = [0] * 19
    for s, _, _ in tree:
        cl_hist[s] += 1
    cl_len = code_lengths(cl_hist, 7)
    hclen = max(k for k in range(19) if cl_len[CL_ORDER[k]]) + 1
    return dict(tokens=toks, lit_hist=lit_hist, n_match=n_match, lit_len=lit_len, dist_len=dist_len, hlit=hlit, tree=tree, cl_hist=cl_hist,
                cl_len=cl_len, hclen=max(hclen, 4))


def deflate_segment(data, final):
    """ONE segment -> its bytes: a dynamic-Huffman block, and where it is not the frame's last the empty stored block behind it."""
    t = segment_tables(data)
    lit_code, cl_code = canonical_codes(t["lit_len"]), canonical_codes(t["cl_len"])
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(t["hlit"] - 257, 5)
    b.put(0, 5)
    b.put(t["hclen"] - 4, 4)
    for k in range(t["hclen"]):
        b.put(t["cl_len"][CL_ORDER[k]], 3)
    for s, nbits, extra in t["tree"]:
        b.code(cl_code[s], t["cl_len"][s])
        b.put(extra, nbits)
    for kind, v in t["tokens"]:
        if kind:
            s, nbits, extra = length_symbol(v)
            b.code(lit_code[s], t["lit_len"][s])
            b.put(extra, nbits)
            b.put(0, t["dist_len"])       # the one distance code, of length 1, is 0
        else:
            b.code(lit_code[v], t["lit_len"][v])
    b.code(lit_code[256], t["lit_len"][256])
    if not final:
        b.put(0, 3)
        b.pad()
        return b.tobytes() + b"\x00\x00\xff\xff"
    b.pad()
    return b.tobytes()


def adler_pair(data):
    """(s1, s2) of zlib's Adler-32 over `data` alone"""
    a = zlib.adler32(bytes(data))
    return a & 0xFFFF, a >> 16


def deflate_rows(rows, seg_rows=16):
    """rows (n, H, row_bytes) uint8 -> per frame a list of (segment bytes, (s1, s2), segment length)"""
    out = []
    for frame in rows:
        H = frame.shape[0]
        segs = []
        for r0 in range(0, H, seg_rows):
            data = frame[r0:r0 + seg_rows].tobytes()
            segs.append((deflate_segment(data, r0 + seg_rows >= H), adler_pair(data), len(data)))
        out.append(segs)
    return out


def adler32_combine(a1, a2, len2):
    """Adler-32 of A + B from those of A and of B and B's length (zlib's adler32_combine, restated from the definition)."""
    s1a, s2a, s1b, s2b = a1 & 0xFFFF, a1 >> 16, a2 & 0xFFFF, a2 >> 16
    s1 = (s1a + s1b - 1) % ADLER
    s2 = (s2a + s2b + (len2 % ADLER) * (s1a - 1)) % ADLER
    return (s2 << 16) | s1


def zlib_stream(rows_frame, seg_rows=16):
    """ONE frame's rows (H, row_bytes) -> its zlib stream"""
    segs = deflate_rows(rows_frame[None], seg_rows)[0]
    adler = 1
    for _, (s1, s2), size in segs:
        adler = adler32_combine(adler, (s2 << 16) | s1, size)
    return ZLIB_HEADER + b"".join(s for s, _, _ in segs) + struct.pack(">I", adler)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def ihdr(W, H):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))


def png_file(frame, seg_rows=16):
    H, W, _ = frame.shape
    return SIGNATURE + ihdr(W, H) + chunk(b"IDAT", zlib_stream(filter_rows(frame[None])[0], seg_rows)) + chunk(b"IEND", b"")


def apng_file(frames, fps=10, seg_rows=16):
    n, H, W, _ = frames.shape
    out, seq = [SIGNATURE, ihdr(W, H), chunk(b"acTL", struct.pack(">II", n, 0))], 0
    rows = filter_rows(frames)
    for i in range(n):
        out.append(chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, int(round(1000 / fps)), 1000, 0, 0)))
        seq += 1
        z = zlib_stream(rows[i], seg_rows)
        if i == 0:
            out.append(chunk(b"IDAT", z))
        else:
            out.append(chunk(b"fdAT", struct.pack(">I", seq) + z))
            seq += 1
    return b"".join(out + [chunk(b"IEND", b"")])


def parse_chunks(data):
    """An independent parser: [(kind, payload)], every length and CRC checked"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        size, kind = struct.unpack_from(">I4s", data, at)
        payload = data[at + 8:at + 8 + size]
        assert len(payload) == size, (kind, at)
        assert struct.unpack_from(">I", data, at + 8 + size)[0] == zlib.crc32(kind + payload), (kind, at)
        out.append((kind, payload))
        at += 12 + size
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


# ---- test data --------------------------------------------------------------------------------------------------------------------------------
def scalar_filter_rows(frame):
    """ONE frame (H, W, 3) -> rows (H, 1 + 3 W): the PNG specification's five filters and libpng's choice, byte by byte in plain Python --
    written apart from filter_rows, which it judges."""
    H, W, _ = frame.shape
    raw = [bytes(frame[y].reshape(-1).tolist()) for y in range(H)]
    out = np.zeros((H, 1 + 3 * W), np.uint8)
    for y in range(H):
        prior = raw[y - 1] if y else bytes(3 * W)
        coded = [[], [], [], [], []]
        for x in range(3 * W):
            left = raw[y][x - 3] if x >= 3 else 0
            above = prior[x]
            corner = prior[x - 3] if x >= 3 else 0
            est = left + above - corner
            dl, da, dc = abs(est - left), abs(est - above), abs(est - corner)
            if dl <= da and dl <= dc:
                nearest = left
            elif da <= dc:
                nearest = above
            else:
                nearest = corner
            for kind, predicted in enumerate((0, left, above, (left + above) // 2, nearest)):
                coded[kind].append((raw[y][x] - predicted) % 256)
        weight = [sum(v if v < 128 else 256 - v for v in row) for row in coded]
        kind = weight.index(min(weight))
        out[y, 0] = kind
        out[y, 1:] = coded[kind]
    return out


def showcase(H=40, W=56, seed=4):
    """A frame in which every filter type wins some row, with ties: rows 0 - 1 zero (all five sums equal: None), row 2 a ramp under a zero row
    (Sub = Paeth, Up = None: Sub), then per group of four rows a noise row and a row built so that None / Sub / Up / Average / Paeth codes it
    best; the rest is noise."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (H, 3 * W)).astype(np.int64)
    f[0:2] = 0
    f[2] = (np.arange(3 * W) // 3 * 2 + 7) % 256
    f[3] = 0
    y = 5
    f[y] = rng.choice([254, 255, 0, 1, 2], 3 * W)                                  # None
    y += 2
    f[y, :3] = 100                                                                   # Sub: every byte within 1 of the pixel to its left
    for x in range(3, 3 * W):
        f[y, x] = (f[y, x - 3] + rng.integers(-1, 2)) % 256
    y += 2
    f[y] = f[y - 1]                                                                  # Up, tied with Paeth (a == c, so it predicts b): the lower type
    y += 2
    for x in range(3 * W):                                                           # Average
        f[y, x] = ((f[y, x - 3] if x >= 3 else 0) + f[y - 1, x]) // 2
    y += 2
    f[y, :3] = (f[y - 1, :3] + 128) % 256                                            # Paeth (a first pixel far from the one above: a != c behind it)
    for x in range(3, 3 * W):
        a, b, c = (f[y, x - 3] if x >= 3 else 0), f[y - 1, x], (f[y - 1, x - 3] if x >= 3 else 0)
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        f[y, x] = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
    return f.astype(np.uint8).reshape(H, W, 3)


CL_LIMIT_LENGTHS = (2, 3, 5, 6, 7, 7, 10, 8, 8, 11, 12, 9, 11, 12, 9, 9, 12, 7, 9, 8, 8, 12, 12, 12, 12, 12, 12, 11, 11, 10, 10, 8, 12, 12, 12, 12, 9, 9,
                    12, 12, 12, 12, 12, 12, 12, 12, 12, 8, 8, 12, 11, 11, 12, 9, 9)


def spread(counts):
    """{byte: count} -> bytes with those counts and no two equal neighbours where that can be avoided (no runs: the histogram is the counts)"""
    import heapq
    out, prev = [], -1
    h = [(-c, s) for s, c in counts.items()]
    heapq.heapify(h)
    while h:
        c, s = heapq.heappop(h)
        if s == prev and h:
            c2, s2 = heapq.heappop(h)
            out.append(s2)
            prev = s2
            if c2 + 1 < 0:
                heapq.heappush(h, (c2 + 1, s2))
            heapq.heappush(h, (c, s))
        else:
            out.append(s)
            prev = s
            if c + 1 < 0:
                heapq.heappush(h, (c + 1, s))
    return bytes(out)


def runs(lengths):
    """runs of the given lengths, neighbours of different value"""
    return b"".join(bytes([(37 * i + 1) % 251]) * n for i, n in enumerate(lengths))


def byte_cases():
    """name -> (rows (n, H, row_bytes) uint8, seg_rows): the deflate cases of the GPU test, arbitrary byte rows"""
    rng = np.random.default_rng(12)

    def mixed(n, H, rb):                                   # noise, flat stretches and short runs, rows that end as the next begins
        a = rng.integers(0, 256, (n, H, rb), dtype=np.uint8)
        a[:, :, rb // 3: rb // 3 + 9] = 7
        a[:, ::3, : rb // 4] = rng.integers(0, 4, (n, (H + 2) // 3, rb // 4), dtype=np.uint8)
        a[:, ::2, -2:] = 9
        a[:, 1::2, :3] = 9
        return a
    row = lambda b: np.frombuffer(b, np.uint8).reshape(1, 1, -1)   # noqa: E731
    cases = {}
    for H in (1, 15, 16, 17, 33):
        cases[f"mixed_H{H}_seg16"] = (mixed(2, H, 37), 16)
        cases[f"mixed_H{H}_seg1"] = (mixed(1, H, 37), 1)
        cases[f"mixed_H{H}_segH"] = (mixed(1, H, 37), H)
    cases["run_lengths"] = (row(runs([1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 1, 263, 5, 517, 518, 519, 520, 2])), 16)
    cases["run_across_rows"] = (np.tile(np.array([9, 9, 1, 2, 3, 4, 5, 9, 9, 9], np.uint8), (1, 6, 1)), 16)
    cases["run_across_segments"] = (np.full((2, 5, 40), 77, np.uint8), 2)
    cases["every_match_length"] = (row(runs([m + 1 for m in range(3, 259)])), 16)
    cases["no_run_at_all"] = (row(bytes((i * 7) % 256 for i in range(3000))), 16)
    cases["one_repeated_byte"] = (np.full((1, 4, 1250), 0x55, np.uint8), 16)
    fib = [2, 2]                                           # twice the Fibonacci series, 16 terms, 5166 bytes: with the end of block counted once
    while len(fib) < 16:                                   # the unlimited tree is 16 deep (1, 1, 2, 3 ... would tie its way down to 10)
        fib.append(fib[-1] + fib[-2])
    cases["fibonacci_15_bit_limit"] = (row(spread({(i * 11 + 3) % 256: c for i, c in enumerate(fib)})), 16)
    top = max(CL_LIMIT_LENGTHS)
    cases["code_length_7_bit_limit"] = (row(spread({(i * 37 + 11) % 256: 2 ** (top - n) for i, n in enumerate(CL_LIMIT_LENGTHS)})), 16)
    cases["long_zero_stretches"] = (row(spread({0: 40, 5: 30, 255: 20, 19: 10, 20: 9, 21: 8, 22: 8, 23: 8, 24: 8, 25: 8, 26: 8})), 16)
    cases["uniform_noise"] = (rng.integers(0, 256, (1, 16, 256), dtype=np.uint8), 16)
    cases["two_chunks_and_a_tail"] = (mixed(2, 3, 300), 2)
    return cases


# ---- size, beside zlib run the same way -------------------------------------------------------------------------------------------------------
def zlib_rle_size(rows_frame, seg_rows=16):
    """The bytes zlib writes for ONE frame's rows (H, row_bytes) cut the same way: raw deflate per segment, Z_RLE, level 6, memLevel 9, ended by
    Z_SYNC_FLUSH (Z_FINISH on the last) -- the same token rule, zlib's own trees, block choice and stored-block fallback."""
    total, H = 0, rows_frame.shape[0]
    for r0 in range(0, H, seg_rows):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        total += len(c.compress(rows_frame[r0:r0 + seg_rows].tobytes()) + c.flush(zlib.Z_FINISH if r0 + seg_rows >= H else zlib.Z_SYNC_FLUSH))
    return total


def size_parity(frame, seg_rows=16):
    """ONE frame (H, W, 3) -> (the reference's deflate bytes, zlib's on the same filtered rows, the reference's PNG file, Pillow's default file)"""
    import io
    from PIL import Image
    rows = filter_rows(frame[None])[0]
    ours = sum(len(s) for s, _, _ in deflate_rows(rows[None], seg_rows)[0])
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    return ours, zlib_rle_size(rows, seg_rows), len(SIGNATURE) + 25 + 12 + 2 + ours + 4 + 12, len(buf.getvalue())
