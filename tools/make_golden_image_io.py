"""Writes tests/golden/image_io.npz: small uint8 pictures, what Pillow itself makes of them through the reference's `load_img` recipe
(centre crop to the target ratio, `resize(LANCZOS)`) and the [-1, 1] float32 tensors ToTensor + `x * 2 - 1` give -- so that the GPU test of
vk_lanczos_resize_u8 needs no Pillow where it runs. PIL and numpy only.

    python tools/make_golden_image_io.py

Cases (source h x w -> 128 x 256): `wide` 225 x 400, `tall` 100 x 100 (rows cropped, then an upscale), `exact` 200 x 400 (no crop, down by 1.5625),
`cols` 120 x 400 (columns cropped: the only case with a left offset). Per case: <name>_src, <name>_box (left, top, crop_w, crop_h), <name>_u8
(Pillow's bytes, HWC), <name>_f32 (CHW)."""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vista_amd.image_io import crop_box  # noqa: E402

CASES = {"wide": (225, 400), "tall": (100, 100), "exact": (200, 400), "cols": (120, 400)}
TARGET = (128, 256)
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "image_io.npz")


def picture(h, w, seed):
    """Flat coloured rectangles (edges, and black / white for the clipping of the Lanczos overshoot), a patch of chirp and a patch of noise --
    mostly flat so that the archive stays small."""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 3), dtype=np.float64)
    img[:] = rng.integers(0, 256, 3)
    for _ in range(24):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        hh, ww = rng.integers(3, max(4, h // 2)), rng.integers(3, max(4, w // 2))
        img[y0:y0 + hh, x0:x0 + ww] = rng.choice([0, 255, -1], p=[0.2, 0.2, 0.6]) if rng.random() < 0.4 else rng.integers(0, 256, 3)
    img[img < 0] = 128
    ph, pw = h // 4, w // 5
    y, x = np.mgrid[0:ph, 0:pw].astype(np.float64)
    img[h // 8: h // 8 + ph, w // 10: w // 10 + pw] = np.stack([127.5 + 127.5 * np.sin(x * x / (2.0 * pw) + c) * np.cos(y / (3.0 + c)) for c in range(3)], -1)
    img[h - ph - 2: h - 2, w - pw - 3: w - 3] = rng.integers(0, 256, (ph, pw, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    th, tw = TARGET
    out = {"target": np.array(TARGET, dtype=np.int32)}
    for i, (name, (h, w)) in enumerate(CASES.items()):
        src = picture(h, w, i)
        left, top, cw, ch = crop_box(w, h, th, tw)
        u8 = np.asarray(Image.fromarray(src).crop((left, top, left + cw, top + ch)).resize((tw, th), resample=Image.LANCZOS))
        f32 = (u8.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1) * np.float32(2.0) - np.float32(1.0)
        out.update({f"{name}_src": src, f"{name}_box": np.array([left, top, cw, ch], dtype=np.int32), f"{name}_u8": u8, f"{name}_f32": f32})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
