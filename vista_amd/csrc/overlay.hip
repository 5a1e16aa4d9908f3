// Drive front door (gfx950): the head-up display of a steered rollout, drawn over the 8-bit frames that are about to be written.
//   vk_stroke_overlay_u8 : (n, H, W, 3) uint8 frames -> the same frames with anti-aliased strokes (round-capped segments, discs) blended in;
//                          a device table picks one of the plan's stroke sets per frame, so one launch draws a video whose rounds differ.
// An element kernel without reuse: a workgroup owns a VK_OVERLAY_TILE_H x VK_OVERLAY_TILE_W tile of one frame, a lane four neighbouring pixels
// of one row (12 bytes: three dwords where W % 4 == 0, bytes otherwise). The plan travels by value in the kernel argument; set, stroke and
// segment indices are wave-uniform, so the plan is read through the scalar path and a tile tests the bounding boxes without vector work. A
// tile outside every box copies (or, in place, returns); a lane outside a stroke's box skips that stroke's per-segment arithmetic, which
// would have left its pixels unchanged anyway (coverage 0 adds 0 * (K - f) = 0). No LDS, no atomics, no barriers.
// No storage-type dependence: the same object code goes into both libraries.
#include <cmath>
#include <cstring>

#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int OV_THREADS = 256;
constexpr int TH = VK_OVERLAY_TILE_H, TW = VK_OVERLAY_TILE_W;
constexpr int PX = 4;                       // pixels per lane
constexpr int GROUPS = TW / PX;             // lanes per tile row
static_assert(GROUPS * TH == OV_THREADS, "one lane per group of four pixels of the tile");
constexpr float COORD_MAX = 1048576.0f;     // 2^20: beyond it the two-pixel margin of the boxes no longer covers fp32 rounding

// The kernel's own layout of the plan: what the host can precompute once is precomputed (d = b - a, r + 0.5, the boxes), in the same fp32
// operations the definition names. Boxes are pixel index ranges [x0, x1) x [y0, y1), clipped to the frame; an empty stroke has an empty box.
struct DevSeg { float ax, ay, dx, dy, inv_len2; };
struct DevStroke { float k[3], alpha, rh; int32_t seg_begin, seg_end, x0, y0, x1, y1; };
struct DevSet { int32_t stroke_begin, stroke_end, x0, y0, x1, y1; };
struct DevPlan {
    DevSet set[VK_OVERLAY_MAX_SETS];
    DevStroke stroke[VK_OVERLAY_MAX_STROKES];
    DevSeg seg[VK_OVERLAY_MAX_SEGMENTS];
    int32_t n_sets, pad;
};
static_assert(sizeof(DevPlan) <= 3072, "the plan shares a 4 KiB kernel argument with the pointers and the launch's hidden arguments");

// Coverage of the pixel centre (px, py) by one segment. One rounding per operation: contraction is switched off for the whole function, so
// that no product is fused into the add or subtract that follows it (the numpy float32 reference cannot fuse either).
__device__ __forceinline__ float seg_cov(float px, float py, float ax, float ay, float dx, float dy, float inv_len2, float rh) {
#pragma clang fp contract(off)
    const float ux = px - ax, uy = py - ay;
    const float m0 = ux * dx, m1 = uy * dy;
    const float dot = m0 + m1;
    const float t = fminf(fmaxf(dot * inv_len2, 0.0f), 1.0f);
    const float tx = t * dx, ty = t * dy;
    const float qx = ax + tx, qy = ay + ty;
    const float ex = px - qx, ey = py - qy;
    const float e0 = ex * ex, e1 = ey * ey;
    const float dist = __builtin_sqrtf(e0 + e1);   // (correctly rounded: the toolchain's default for fp32 sqrt)
    return fminf(fmaxf(rh - dist, 0.0f), 1.0f);
}

__device__ __forceinline__ float blend(float f, float a, float k) {
#pragma clang fp contract(off)
    const float diff = k - f;
    const float ad = a * diff;
    return f + ad;
}

__device__ __forceinline__ bool boxes_meet(int ax0, int ay0, int ax1, int ay1, int bx0, int by0, int bx1, int by1) {
    return ax0 < bx1 && bx0 < ax1 && ay0 < by1 && by0 < ay1;
}

// grid (tiles_y * tiles_x, n). in and out may be the same buffer (no __restrict__ on them): a lane reads its 12 bytes before it writes them and
// touches no other lane's.
template <bool WIDE>
__global__ __launch_bounds__(OV_THREADS) void stroke_overlay_kernel(const uint8_t* in, uint8_t* out, const int32_t* __restrict__ set_of_frame,
                                                                    const DevPlan p, int H, int W, int tiles_x) {
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int ty0 = tyi * TH, tx0 = txi * TW;
    const int ty1 = min(ty0 + TH, H), tx1 = min(tx0 + TW, W);
    // ---- the tile's decision, on wave-uniform values ----
    const int s = __builtin_amdgcn_readfirstlane(set_of_frame[blockIdx.y]);
    bool draw = s >= 0 && s < p.n_sets;
    int k_begin = 0, k_end = 0;
    if (draw) {
        k_begin = p.set[s].stroke_begin;
        k_end = p.set[s].stroke_end;
        draw = boxes_meet(p.set[s].x0, p.set[s].y0, p.set[s].x1, p.set[s].y1, tx0, ty0, tx1, ty1);
    }
    if (!draw && in == out) return;

    const int y = ty0 + tid / GROUPS, x0 = tx0 + (tid % GROUPS) * PX;
    if (y >= H || x0 >= W) return;
    const int nx = WIDE ? PX : min(PX, W - x0);   // (W % 4 == 0: every group is whole)
    const size_t at = ((size_t)blockIdx.y * H + y) * ((size_t)W * 3) + (size_t)x0 * 3;
    uint32_t b[3 * PX];
    if (WIDE) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(in + at);   // (3 W and 3 x0 are multiples of 12)
        const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
        if (!draw) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(out + at);
            dst[0] = w0; dst[1] = w1; dst[2] = w2;
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b[j] = (w0 >> (8 * j)) & 0xffu;
            b[4 + j] = (w1 >> (8 * j)) & 0xffu;
            b[8 + j] = (w2 >> (8 * j)) & 0xffu;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3 * PX; ++j) b[j] = j < 3 * nx ? in[at + j] : 0u;
        if (!draw) {
#pragma unroll
            for (int j = 0; j < 3 * PX; ++j)
                if (j < 3 * nx) out[at + j] = (uint8_t)b[j];
            return;
        }
    }

    float f[3 * PX];
#pragma unroll
    for (int j = 0; j < 3 * PX; ++j) f[j] = (float)b[j];
    const float py = (float)y + 0.5f;
    for (int k = k_begin; k < k_end; ++k) {            // (uniform: every lane of the tile walks the same strokes)
        const DevStroke& sk = p.stroke[k];
        if (!boxes_meet(sk.x0, sk.y0, sk.x1, sk.y1, tx0, ty0, tx1, ty1)) continue;   // scalar
        if (!boxes_meet(sk.x0, sk.y0, sk.x1, sk.y1, x0, y, x0 + PX, y + 1)) continue;  // this lane's four pixels
        float cov[PX] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int g = sk.seg_begin; g < sk.seg_end; ++g) {
            const DevSeg& sg = p.seg[g];
#pragma unroll
            for (int e = 0; e < PX; ++e)
                cov[e] = fmaxf(cov[e], seg_cov((float)(x0 + e) + 0.5f, py, sg.ax, sg.ay, sg.dx, sg.dy, sg.inv_len2, sk.rh));
        }
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            const float a = sk.alpha * cov[e];
#pragma unroll
            for (int c = 0; c < 3; ++c) f[3 * e + c] = blend(f[3 * e + c], a, sk.k[c]);
        }
    }
#pragma unroll
    for (int j = 0; j < 3 * PX; ++j) b[j] = (uint32_t)((int)f[j]) & 0xffu;   // truncating cast
    if (WIDE) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + at);
        dst[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        dst[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        dst[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 3 * PX; ++j)
            if (j < 3 * nx) out[at + j] = (uint8_t)b[j];
    }
}

__host__ inline bool ov_finite_in(float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; }

__host__ inline int32_t ov_clip(double v, int32_t hi) { return v <= 0.0 ? 0 : (v >= (double)hi ? hi : (int32_t)v); }

}  // namespace

extern "C" int vk_stroke_overlay_u8(const void* in, void* out, const int32_t* set_of_frame, const VkStrokePlan* plan, int32_t n, int32_t H,
                                    int32_t W, void* stream) {
    if (!in || !out || !set_of_frame || !plan || n <= 0 || H <= 0 || W <= 0) return VK_EINVAL;
    if (n > 65535) return VK_EINVAL;   // (grid.y)
    if ((((size_t)set_of_frame) & 3) != 0) return VK_EINVAL;
    // dword accesses only where every row of every frame starts on a 4-byte boundary; a shape's path is a function of W alone
    const bool wide = (W % 4) == 0;
    if (wide && (((size_t)in | (size_t)out) & 3) != 0) return VK_EINVAL;
    if (plan->n_sets < 0 || plan->n_sets > VK_OVERLAY_MAX_SETS || plan->n_strokes < 0 || plan->n_strokes > VK_OVERLAY_MAX_STROKES ||
        plan->n_segments < 0 || plan->n_segments > VK_OVERLAY_MAX_SEGMENTS)
        return VK_EINVAL;
    DevPlan p;
    memset(&p, 0, sizeof(p));
    p.n_sets = plan->n_sets;
    for (int g = 0; g < plan->n_segments; ++g) {
        const VkStrokeSegment& sg = plan->seg[g];
        if (!ov_finite_in(sg.ax, -COORD_MAX, COORD_MAX) || !ov_finite_in(sg.ay, -COORD_MAX, COORD_MAX) ||
            !ov_finite_in(sg.bx, -COORD_MAX, COORD_MAX) || !ov_finite_in(sg.by, -COORD_MAX, COORD_MAX))
            return VK_EINVAL;
        if (!std::isfinite(sg.inv_len2) || sg.inv_len2 < 0.0f) return VK_EINVAL;
        p.seg[g] = DevSeg{sg.ax, sg.ay, sg.bx - sg.ax, sg.by - sg.ay, sg.inv_len2};
    }
    for (int k = 0; k < plan->n_strokes; ++k) {
        const VkStroke& sk = plan->stroke[k];
        if (!ov_finite_in(sk.alpha, 0.0f, 1.0f) || !ov_finite_in(sk.r, 0.0f, COORD_MAX)) return VK_EINVAL;
        for (int c = 0; c < 3; ++c)
            if (!ov_finite_in(sk.color[c], 0.0f, 255.0f)) return VK_EINVAL;
        if (sk.seg_begin < 0 || sk.seg_count < 0 || sk.seg_begin > plan->n_segments || sk.seg_count > plan->n_segments - sk.seg_begin) return VK_EINVAL;
        DevStroke& d = p.stroke[k];
        d.k[0] = sk.color[0]; d.k[1] = sk.color[1]; d.k[2] = sk.color[2];
        d.alpha = sk.alpha;
        d.rh = sk.r + 0.5f;
        d.seg_begin = sk.seg_begin;
        d.seg_end = sk.seg_begin + sk.seg_count;
        if (sk.seg_count > 0) {
            double lox = 1e30, loy = 1e30, hix = -1e30, hiy = -1e30;
            for (int g = d.seg_begin; g < d.seg_end; ++g) {
                const VkStrokeSegment& sg = plan->seg[g];
                lox = fmin(lox, fmin((double)sg.ax, (double)sg.bx)); hix = fmax(hix, fmax((double)sg.ax, (double)sg.bx));
                loy = fmin(loy, fmin((double)sg.ay, (double)sg.by)); hiy = fmax(hiy, fmax((double)sg.ay, (double)sg.by));
            }
            // a pixel the stroke can touch has its centre within r + 0.5 of a segment; two more pixels for the rounding of q and dist
            const double grow = (double)sk.r + 2.5;
            d.x0 = ov_clip(floor(lox - grow), W); d.x1 = ov_clip(ceil(hix + grow), W);
            d.y0 = ov_clip(floor(loy - grow), H); d.y1 = ov_clip(ceil(hiy + grow), H);
        }
    }
    for (int s = 0; s < plan->n_sets; ++s) {
        const VkStrokeSet& st = plan->set[s];
        if (st.stroke_begin < 0 || st.stroke_count < 0 || st.stroke_begin > plan->n_strokes || st.stroke_count > plan->n_strokes - st.stroke_begin)
            return VK_EINVAL;
        DevSet& d = p.set[s];
        d.stroke_begin = st.stroke_begin;
        d.stroke_end = st.stroke_begin + st.stroke_count;
        int32_t x0 = W, y0 = H, x1 = 0, y1 = 0;
        for (int k = d.stroke_begin; k < d.stroke_end; ++k) {
            const DevStroke& sk = p.stroke[k];
            if (sk.x0 >= sk.x1 || sk.y0 >= sk.y1) continue;
            x0 = sk.x0 < x0 ? sk.x0 : x0; y0 = sk.y0 < y0 ? sk.y0 : y0;
            x1 = sk.x1 > x1 ? sk.x1 : x1; y1 = sk.y1 > y1 ? sk.y1 : y1;
        }
        if (x0 < x1 && y0 < y1) { d.x0 = x0; d.y0 = y0; d.x1 = x1; d.y1 = y1; }
    }
    const long long tiles_x = ((long long)W + TW - 1) / TW, tiles_y = ((long long)H + TH - 1) / TH;
    if (tiles_x * tiles_y > 0x7fffffffLL) return VK_EINVAL;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n);
    if (wide)
        hipLaunchKernelGGL(stroke_overlay_kernel<true>, grid, dim3(OV_THREADS), 0, (hipStream_t)stream, (const uint8_t*)in, (uint8_t*)out,
                           set_of_frame, p, H, W, (int)tiles_x);
    else
        hipLaunchKernelGGL(stroke_overlay_kernel<false>, grid, dim3(OV_THREADS), 0, (hipStream_t)stream, (const uint8_t*)in, (uint8_t*)out,
                           set_of_frame, p, H, W, (int)tiles_x);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
