"""The block-matching flow of include/vista_hip.h ("motion scores") restated in plain numpy, clarity over speed, and the frames its tests use.

    luma      Y = (77 R + 150 G + 29 B + 128) >> 8
    pyramid   three levels, level l + 1 the 2 x 2 mean (a + b + c + d + 2) >> 2 of level l
    blocks    8 x 8 at every level; block (by, bx) has the parent (by >> 1, bx >> 1) one level up
    cost      SAD of the block against the next frame at (y + vy, x + vx), coordinates clamped to the image
    search    level 2: [-7, 7]^2 around zero; levels 1 and 0: twice the parent's vector plus an increment in [-2, 2]^2
    choice    the smallest (SAD, |dy| + |dx| of the increment, dy, dx)

Everything is an integer; the kernels are held to this bit for bit. Nothing here imports vista_amd or touches a GPU."""
import functools

import numpy as np

BLOCK, LEVELS, COARSE, REFINE = 8, 3, 7, 2


def luma(frames):
    f = np.asarray(frames).astype(np.int64)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).astype(np.uint8)


def halve(level):
    a = level.astype(np.int64)
    return ((a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(frames):
    """(n, H, W, 3) uint8 -> [level 0 (n, H, W), level 1 (n, H/2, W/2), level 2 (n, H/4, W/4)] uint8."""
    levels = [luma(frames)]
    for _ in range(LEVELS - 1):
        levels.append(halve(levels[-1]))
    return levels


def block_sad(cur, nxt, by, bx, vy, vx):
    """SAD of block (by, bx) of `cur` against `nxt` displaced by (vy, vx), edge replicate."""
    Hl, Wl = cur.shape
    ys = np.clip(np.arange(BLOCK * by, BLOCK * by + BLOCK) + vy, 0, Hl - 1)
    xs = np.clip(np.arange(BLOCK * bx, BLOCK * bx + BLOCK) + vx, 0, Wl - 1)
    a = cur[BLOCK * by:BLOCK * by + BLOCK, BLOCK * bx:BLOCK * bx + BLOCK].astype(np.int64)
    return int(np.abs(a - nxt[np.ix_(ys, xs)].astype(np.int64)).sum())


def search(cur, nxt, by, bx, base, rng):
    """-> (vector, SAD): base plus the increment of the smallest (SAD, |dy| + |dx|, dy, dx) over [-rng, rng]^2."""
    best = None
    for dy in range(-rng, rng + 1):
        for dx in range(-rng, rng + 1):
            key = (block_sad(cur, nxt, by, bx, base[0] + dy, base[1] + dx), abs(dy) + abs(dx), dy, dx)
            if best is None or key < best:
                best = key
    return (base[0] + best[2], base[1] + best[3]), best[0]


def pair_flow(cur_levels, nxt_levels):
    """The three levels of frames i and i + 1 -> (flow (H/8, W/8, 2) int16, sad (H/8, W/8, 2) uint16: at the vector, at zero)."""
    vectors = None
    for lvl in range(LEVELS - 1, -1, -1):
        cur, nxt = cur_levels[lvl], nxt_levels[lvl]
        gy, gx = cur.shape[0] // BLOCK, cur.shape[1] // BLOCK
        out = np.zeros((gy, gx, 2), np.int64)
        sads = np.zeros((gy, gx), np.int64)
        for by in range(gy):
            for bx in range(gx):
                if vectors is None:
                    base, rng = (0, 0), COARSE
                else:
                    base, rng = (2 * int(vectors[by >> 1, bx >> 1, 0]), 2 * int(vectors[by >> 1, bx >> 1, 1])), REFINE
                out[by, bx], sads[by, bx] = search(cur, nxt, by, bx, base, rng)
        vectors = out
    cur, nxt = cur_levels[0], nxt_levels[0]
    zero = np.array([[block_sad(cur, nxt, by, bx, 0, 0) for bx in range(vectors.shape[1])] for by in range(vectors.shape[0])], np.int64)
    return vectors.astype(np.int16), np.stack([sads, zero], -1).astype(np.uint16)


def block_flow(frames):
    """(n, H, W, 3) uint8 -> (flow (n - 1, H/8, W/8, 2) int16, sad (n - 1, H/8, W/8, 2) uint16)."""
    frames = np.asarray(frames)
    n, H, W, _ = frames.shape
    levels = pyramid(frames)
    flow = np.zeros((max(n - 1, 0), H // BLOCK, W // BLOCK, 2), np.int16)
    sad = np.zeros((max(n - 1, 0), H // BLOCK, W // BLOCK, 2), np.uint16)
    for i in range(n - 1):
        flow[i], sad[i] = pair_flow([lv[i] for lv in levels], [lv[i + 1] for lv in levels])
    return flow, sad


def pair_sums(flow, sad, flow_ref=None):
    """-> (pairs, 5) int64: non-zero blocks, sum |v|^2, sum SAD, sum SAD at zero, sum |v - v_ref|^2 (0 without flow_ref)."""
    f = flow.astype(np.int64).reshape(flow.shape[0], -1, 2)
    s = sad.astype(np.int64).reshape(sad.shape[0], -1, 2)
    out = np.zeros((f.shape[0], 5), np.int64)
    out[:, 0] = (f != 0).any(axis=2).sum(axis=1)
    out[:, 1] = (f * f).sum(axis=(1, 2))
    out[:, 2] = s[..., 0].sum(axis=1)
    out[:, 3] = s[..., 1].sum(axis=1)
    if flow_ref is not None:
        d = f - flow_ref.astype(np.int64).reshape(f.shape)
        out[:, 4] = (d * d).sum(axis=(1, 2))
    return out


# (n, H, W), every side a multiple of 32, whose n * H * W * 21 wraps 64 bits (to 0; to a negative number) or whose (H / 4) * (W / 4) wraps 32:
# the entry points must refuse them from the sides alone, before any product is formed
WRAPPING_SHAPES = [(16, 2 ** 30, 2 ** 30), (8, 2 ** 30 + 32, 2 ** 30), (1, 2 ** 31 - 32, 32), (2, 32, 2 ** 31 - 32), (65535, 2 ** 17, 2 ** 17)]


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def texture(H, W, seed=0, sigma=1.5):
    """Smooth texture: seeded Gaussian noise low-passed with a separable Gaussian (sigma px), scaled to 0 .. 255, (H, W, 3) uint8 with three
    different channels. White noise has no low-frequency content: the pyramid cannot find its shifts."""
    rng = np.random.default_rng(seed)
    radius = int(np.ceil(4 * sigma))
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2 * sigma * sigma))
    g /= g.sum()
    out = np.zeros((H, W, 3), np.uint8)
    for c in range(3):
        a = rng.standard_normal((H + 2 * radius, W + 2 * radius))
        a = np.apply_along_axis(lambda r: np.convolve(r, g, mode="valid"), 1, a)
        a = np.apply_along_axis(lambda r: np.convolve(r, g, mode="valid"), 0, a)
        a = (a - a.min()) / (a.max() - a.min())
        out[..., c] = np.round(a * 255.0).astype(np.uint8)
    out.setflags(write=False)
    return out


MARGIN = 40   # the translation cases cut their windows this far inside a larger texture: every vector of TRANSLATIONS stays inside it
TRANSLATIONS = [(0, 0), (1, 0), (0, -1), (3, 5), (-7, 2), (13, -11), (-21, 17), (30, -30)]
TRANSLATION_SHAPE = (128, 160)


def translated_pair(vector, shape=TRANSLATION_SHAPE, seed=1):
    """Two frames: a window of a larger texture, and the window whose content has moved by `vector`: frame1[y + vy, x + vx] = frame0[y, x]."""
    H, W = shape
    vy, vx = vector
    big = texture(H + 2 * MARGIN, W + 2 * MARGIN, seed)
    f0 = big[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    f1 = big[MARGIN - vy:MARGIN - vy + H, MARGIN - vx:MARGIN - vx + W]
    return np.ascontiguousarray(np.stack([f0, f1]))


def interior_blocks(shape, vector):
    """(H/8, W/8) bool: the level-0 blocks whose 32 x 32 level-2 ancestor, displaced by the vector and widened by 4 px, lies inside the frame."""
    H, W = shape
    vy, vx = vector
    ok = np.zeros((H // BLOCK, W // BLOCK), bool)
    for by in range(H // BLOCK):
        for bx in range(W // BLOCK):
            y0, x0 = 32 * (by >> 2) + vy - 4, 32 * (bx >> 2) + vx - 4
            ok[by, bx] = y0 >= 0 and x0 >= 0 and y0 + 40 <= H and x0 + 40 <= W
    return ok


def split_pair(shape=(64, 128), left=(0, 4), right=(2, -6), seed=2):
    """A frame whose left half moves by `left` and whose right half moves by `right`."""
    H, W = shape
    a, b = translated_pair(left, shape, seed), translated_pair(right, shape, seed)
    nxt = np.concatenate([a[1][:, :W // 2], b[1][:, W // 2:]], axis=1)
    return np.ascontiguousarray(np.stack([a[0], nxt]))


def noise_frames(n, H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def coarse_noise_frames(n, H, W, seed=4, levels=4):
    """Noise of few grey levels in cells of 2 x 2: many equal SADs, so the lexicographic choice decides."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, levels, (n, H // 2, W // 2, 1), dtype=np.uint8) * (255 // (levels - 1))
    return np.ascontiguousarray(a.repeat(2, axis=1).repeat(2, axis=2).repeat(3, axis=3))


def entering_object(H=64, W=96):
    """A bright square that is half outside the left border in frame 0 and has moved in by 6 px in frame 1, on a dim ramp."""
    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for x0 in (-8, -2):
        f = (20 + (xx + 2 * yy) % 40).astype(np.uint8)
        f[20:36, max(x0, 0):x0 + 16] = 240
        frames.append(np.stack([f, f, f], -1))
    return np.ascontiguousarray(np.stack(frames))
