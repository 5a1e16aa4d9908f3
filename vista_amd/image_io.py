"""Host side of the image I/O kernels (csrc/image_io.hip): the geometry and the coefficient tables, in plain Python / numpy.

`load_img` of the reference (sample.py:174-201) is centre crop -> `PIL.Image.resize(LANCZOS)` -> ToTensor -> x * 2 - 1. Pillow's 8-bit resize is
integer arithmetic after one float64 table per axis (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc), so it can be restated
exactly: `lanczos_tables` builds the same tables, `resize_u8_reference` evaluates them in numpy the way the two kernels do (tests hold it to
Pillow byte for byte), and `ops.load_img_batch` uploads them and launches vk_lanczos_resize_u8.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2      # Pillow's fixed-point scale of an 8-bit channel's weights
LANCZOS_SUPPORT = 3.0


def crop_box(ori_w, ori_h, target_height, target_width):
    """-> (left, top, crop_w, crop_h): the centre crop `load_img` takes before it resizes (sample.py:184-193), with its float comparisons and
    int() truncations. A source wider than the target ratio loses columns, a taller one rows, an exact one nothing."""
    want = target_width / target_height
    have = ori_w / ori_h
    if have > want:
        keep = int(target_width / target_height * ori_h)
        left, right = (ori_w - keep) // 2, (ori_w + keep) // 2
        return left, 0, right - left, ori_h
    if have < want:
        keep = int(target_height / target_width * ori_w)
        top, bottom = (ori_h - keep) // 2, (ori_h + keep) // 2
        return 0, top, ori_w, bottom - top
    return 0, 0, ori_w, ori_h


def _lanczos3(x):
    if not -LANCZOS_SUPPORT <= x < LANCZOS_SUPPORT:
        return 0.0

    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / LANCZOS_SUPPORT)


@functools.lru_cache(maxsize=32)
def lanczos_tables(in_size, out_size):
    """One axis of Pillow's LANCZOS resize from `in_size` to `out_size` samples -> (bounds (out, 2) int32 = [first tap, tap count],
    coef (out, ksize) int32, ksize). float64 throughout, the weights of a tap window summed in tap order, like the C code; each normalised weight
    becomes int(+-0.5 + w * 2**22), rounding away from zero. Rows are zero-padded to ksize."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"lanczos_tables: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = LANCZOS_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [_lanczos3((x + xmin - center + 0.5) * inv) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef, ksize


def _pass(img, bounds, coef, axis):
    """One integer pass along `axis` of an (H, W, 3) uint8 image: clip8((2**21 + sum pixel * weight) >> 22)."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for i, (first, count) in enumerate(bounds):
        acc = np.tensordot(coef[i, :count].astype(np.int64), src[first:first + count], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8_reference(img, box, out_h, out_w):
    """numpy evaluation of the tables, pass for pass what the kernels compute: (H, W, 3) uint8 -> (out_h, out_w, 3) uint8 of the crop `box`
    (left, top, crop_w, crop_h). The check of the tables themselves against Pillow and against tests/golden/image_io.npz."""
    left, top, cw, ch = box
    crop = np.asarray(img)[top:top + ch, left:left + cw]
    bx, cx, _ = lanczos_tables(cw, out_w)
    by, cy, _ = lanczos_tables(ch, out_h)
    return _pass(_pass(crop, bx, cx, 1), by, cy, 0)


def unit_range_table():
    """The 256 values ToTensor and `x * 2.0 - 1.0` give the bytes 0..255, in IEEE float32 (numpy: one correctly rounded operation each)."""
    k = np.arange(256, dtype=np.float32)
    return (k / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)


def grid_geometry(n, height, width, nrow=None, padding=2):
    """Layout of `torchvision.utils.make_grid(samples, nrow=int(n ** 0.5))` with its defaults -> (xmaps, ymaps, rows, cols, padding). One image
    comes back as it is (make_grid returns a single image without a border): padding 0, a 1 x 1 layout."""
    nrow = int(n ** 0.5) if nrow is None else nrow
    if n == 1:
        return 1, 1, height, width, 0
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    return xmaps, ymaps, ymaps * (height + padding) + padding, xmaps * (width + padding) + padding, padding
