// The arithmetic of OpenCLIP image preprocessing (FrozenOpenCLIPImageEmbedder.preprocess), shared by its two kernels: clip_preprocess_kernel
// (elementwise.hip, fp32 NCHW frames in global memory) and clip_preprocess_u8_kernel (perceptual.hip, HWC bytes staged into LDS as fp32).
// kornia 0.6.9 `resize(x, (S, S), "bicubic", align_corners=True, antialias=True)` = separable Gaussian blur (reflect border; sigma =
// (factor - 1) / 2 per axis, kernel size int(max(4 sigma, 3)) made odd -- only when downscaling) followed by F.interpolate(mode="bicubic",
// align_corners=True) (A = -0.75, clamped taps); then (x + 1) / 2 and the CLIP mean / std.
// Both kernels hand clip_resample() a functor from a source row index to a `const float*` indexed by the source column; everything that is
// rounded is in this file, so the two outputs agree bit for bit wherever the fp32 pixel values do.
#pragma once
#include "common.h"

constexpr int CLIP_MAX_KS = 63;  // largest odd Gaussian kernel of the antialias blur (a side of ~7000 px resized to 224)

__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
__device__ __forceinline__ int reflect_idx(int i, int n) { i = i < 0 ? -i : i; return i >= n ? 2 * (n - 1) - i : i; }

// Gaussian taps (the same for every output value): once per workgroup, in LDS, in the order and arithmetic of the per-thread form they
// replace (a runtime-indexed register array lives in scratch: 2 x 63 floats per lane); ks == 1 = no blur along that axis.
// Every thread of the workgroup calls this (it holds the barrier) and gets the two tap sums.
__device__ __forceinline__ void clip_gauss_taps(float* gy, float* gx, int ks_y, int ks_x, float sig_y, float sig_x, float& ny, float& nx) {
    if ((int)threadIdx.x < ks_y) { const float d = (float)((int)threadIdx.x - ks_y / 2); gy[threadIdx.x] = ks_y > 1 ? expf(-d * d / (2.f * sig_y * sig_y)) : 1.f; }
    if ((int)threadIdx.x < ks_x) { const float d = (float)((int)threadIdx.x - ks_x / 2); gx[threadIdx.x] = ks_x > 1 ? expf(-d * d / (2.f * sig_x * sig_x)) : 1.f; }
    __syncthreads();
    ny = 0.f, nx = 0.f;
    for (int k = 0; k < ks_y; ++k) ny += gy[k];
    for (int k = 0; k < ks_x; ++k) nx += gx[k];
}

// source position of output index o along an axis of `size` source and `out_hw` output pixels (align_corners=True)
__device__ __forceinline__ float clip_src_pos(int o, int size, int out_hw) {
    return out_hw > 1 ? (float)o * ((float)(size - 1) / (float)(out_hw - 1)) : 0.f;
}

// The resized value at output (oy, ox) of one channel of one image, in [-1, 1]. rows(y) -> the fp32 pixels of source row y, 0 <= y < H.
template <class Rows>
__device__ __forceinline__ float clip_resample(const Rows& rows, int oy, int ox, int H, int W, int out_hw, const float* gy, const float* gx,
                                               int ks_y, int ks_x, float ny, float nx) {
    const float ry = clip_src_pos(oy, H, out_hw);
    const float rx = clip_src_pos(ox, W, out_hw);
    const int iy = (int)floorf(ry), ix = (int)floorf(rx);
    const float ty = ry - (float)iy, tx = rx - (float)ix;
    const float A = -0.75f;
    const float wy[4] = {cubic2(ty + 1.f, A), cubic1(ty, A), cubic1(1.f - ty, A), cubic2(2.f - ty, A)};
    const float wx[4] = {cubic2(tx + 1.f, A), cubic1(tx, A), cubic1(1.f - tx, A), cubic2(2.f - tx, A)};
    float acc = 0.f;
    for (int a = 0; a < 4; ++a) {
        int yy = iy - 1 + a;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);  // bicubic taps are clamped to the (blurred) image
        float rowacc = 0.f;
        for (int b = 0; b < 4; ++b) {
            int xx = ix - 1 + b;
            xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
            float v = 0.f;  // blurred(yy, xx): reflect-padded separable Gaussian
            for (int ky = 0; ky < ks_y; ++ky) {
                const float* row = rows(reflect_idx(yy + ky - ks_y / 2, H));
                float r = 0.f;
                for (int kx = 0; kx < ks_x; ++kx) r = fmaf(gx[kx], row[reflect_idx(xx + kx - ks_x / 2, W)], r);
                v = fmaf(gy[ky], r, v);
            }
            rowacc = fmaf(wx[b], v / (ny * nx), rowacc);
        }
        acc = fmaf(wy[a], rowacc, acc);
    }
    return acc;
}

// [-1, 1] -> [0, 1] -> CLIP mean / std
__device__ __forceinline__ float clip_normalise(float acc, float mean, float sd) { return ((acc + 1.f) * 0.5f - mean) / sd; }
