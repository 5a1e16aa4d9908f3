"""The size of the PNG coder's streams (tests/_png_ref.py, which the kernels of csrc/png.hip equal byte for byte) beside zlib run the same way --
raw deflate per 16-row segment, Z_RLE, level 6, memLevel 9, Z_SYNC_FLUSH -- on the same filtered rows, and the file beside Pillow's default file.
No GPU. The largest relative excess over zlib is what tests/test_png_cpu.py bounds (plus 25 %, at least 0.1 %); the Pillow figure is not asserted.
    python tools/png_parity.py [--out profiles/png_parity.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _png_ref as R  # noqa: E402
from tests.test_png_cpu import PARITY_SIZES, PICTURES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_parity.txt"))
    opt = ap.parse_args()
    lines = ["PNG coder, size parity (tools/png_parity.py; no GPU: the reference of tests/_png_ref.py, which the kernels equal byte for byte)",
             "deflate data of the filtered rows in 16-row segments; zlib: raw deflate per segment, Z_RLE, level 6, memLevel 9, Z_SYNC_FLUSH", ""]
    worst = None
    for sizes in (PARITY_SIZES, {k: (40, 56) for k in PARITY_SIZES}):
        for name in sorted(PICTURES):
            h, w = sizes[name]
            ours, theirs, file, pillow = R.size_parity(PICTURES[name](h, w))
            excess = (ours - theirs) / theirs
            if sizes is PARITY_SIZES and (worst is None or excess > worst[0]):
                worst = (excess, name)
            lines.append(f"{name:<13} {h:>4} x {w:<5} ours {ours:>8}   zlib Z_RLE {theirs:>8}   {100 * excess:+7.3f} %     file {file:>8}   Pillow's default "
                         f"{pillow:>8}   {100 * (file - pillow) / pillow:+8.2f} %")
        lines.append("")
    lines += [f"largest excess over zlib, first group (the asserted set): {100 * worst[0]:+.3f} % ({worst[1]}); bound = that + 25 %, at least 0.1 %",
              "noise: zlib stores incompressible segments (5 bytes of overhead each) where this coder writes a Huffman block; stored blocks are not built.",
              "second group (40 x 56, segments of 2.7 KB, not asserted): the tree description weighs more the smaller the segment.",
              "Pillow's default file (zlib level 6 with LZ77 over the whole picture) is smaller on flat pictures, larger on photographic ones."]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(opt.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
