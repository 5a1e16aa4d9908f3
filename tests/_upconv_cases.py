"""Shapes, inputs and float64 references of the folded upsample convolution (ops.pack_upconv2x2 / ops.upconv2x2), shared by
tests/test_upconv_fold_cpu.py and tests/test_upconv_fold_gpu.py. Nothing here touches a GPU or imports vista_amd at import time.

The folded form: conv3x3(pad 1) after a nearest x2 upsample is, per output parity class (a, b), a 2x2 convolution of the SOURCE image whose window
starts at (i + a - 1, j + b - 1); the class weights are sums of the nine taps (ops.fold_upconv2x2). The reference of a folded launch is built from the
values the kernel is handed -- the storage-type inputs and the pack's own folded, rounded class weights (the convention tests/_kernel_cases.py states
for folded packs) -- in float64."""
import torch
import torch.nn.functional as F

from tests._kernel_cases import G, I, conv3x3_ref, nchw2tok, tok2nchw

F64 = torch.float64
# (n, H, W, Cin, Cout, rowvec): the smallest shapes at which each part of the kernel can still go wrong
GPU_SHAPES = (
    (2, 9, 16, 64, 320, False),     # 288 rows per class: a tile that straddles the two images, and a ragged second tile
    (3, 5, 7, 192, 640, False),     # odd sizes, less than one tile per class, two column tiles, three K slabs
    (2, 1, 3, 64, 320, False),      # H = 1: both row neighbours out of range
    (2, 18, 32, 128, 320, False),   # 4.5 row tiles per class, 20 tiles in all: the tile -> (class, row tile) order, through the XCD remap
    (4, 9, 16, 128, 640, True),     # the per-image row vector reaches the right image in every class
)
BASELINE_SHAPES = ((50, 9, 16, 1280, 1280), (50, 18, 32, 1280, 1280), (50, 36, 64, 640, 640))   # the three UNet upsamples of the benchmark step


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def inputs(st, n, H, W, cin, cout, rowvec=False):
    """Seeded CPU inputs: x in the storage type, the fp32 master weight [Cout][Cin][3][3] and bias, optionally a per-image fp32 row vector."""
    g = G(1000 * n + 100 * H + 10 * W + cin + cout)
    i = I(x=torch.randn(n, H * W, cin, generator=g).to(st), w=torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5,
          b=torch.randn(cout, generator=g))
    if rowvec:
        i["rv"] = torch.randn(n, cout, generator=g)
    return i


def scatter_2x2(x, wc, b):
    """The four class convolutions written out: x [n][Cin][H][W], wc [4][Cout][Cin][2][2] (class 2a + b), b [Cout] -> [n][Cout][2H][2W]. Class (a, b)
    reads source rows i + a - 1, i + a: zero padding (1 - a) above and a below, likewise in x."""
    n, _, H, W = x.shape
    out = x.new_zeros(n, wc.shape[1], 2 * H, 2 * W)
    for a in (0, 1):
        for bb in (0, 1):
            out[:, :, a::2, bb::2] = F.conv2d(F.pad(x, (1 - bb, bb, 1 - a, a)), wc[2 * a + bb], b)
    return out


def folded_ref(x, wc, b, n, H, W, rv=None):
    """float64 reference of a folded launch on token-major x (n, H*W, Cin) with class weights wc -> (n, 4*H*W, Cout)."""
    y = nchw2tok(scatter_2x2(tok2nchw(x.double(), n, H, W), wc.double(), b.double()))
    return y if rv is None else y + rv.double()[:, None, :]


def nine_tap_ref(x, w, b, n, H, W, rv=None):
    """float64 conv2d(interpolate(x, 2, "nearest"), w, b, padding=1) on token-major x."""
    y = conv3x3_ref(x, w, b, n, H, W, ups=2)
    return y if rv is None else y + rv.double()[:, None, :]
