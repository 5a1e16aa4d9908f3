// Reward estimation front door (gfx950): what the ensemble knows beyond one scalar, and a picture of it.
//   vk_ensemble_frame_stats : unbiased ensemble variance of E latents -> its sum per frame (fp64, fixed order) and its channel mean per pixel
//   vk_candidate_frame_stats: the same statistics for K candidates' ensembles in one call + every candidate's total and the index of the smallest
//   vk_heat_overlay_u8      : input frames blended towards a heat colour by that per-pixel map -> uint8 HWC frames
// All are HBM-bound element kernels without reuse: lanes walk the contiguous hw (or W) axis, 16 bytes per lane where the shape guarantees the
// alignment (hw % 4 == 0, W % 4 == 0), one element per lane otherwise; the only LDS is the block reduction of the frame sums.
// No storage-type dependence: the same object code goes into both libraries.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int RW_THREADS = 256;

// ---- per-frame statistics -------------------------------------------------------------------------------------------------------------------
// x [E][T][C][hw]. Block (b, t) owns the pixel groups g = b * 256 + tid + k * (VK_FRAME_STATS_BLOCKS * 256) of frame t (a group = V neighbouring
// pixels, V = 4 where hw % 4 == 0, else 1): which thread adds which element is a function of hw alone, so a frame's sum does not depend on T or
// on the frames around it. The per-element value is ens_var_partial_kernel's (csrc/elementwise.hip), operation for operation.
__device__ __forceinline__ float ens_var_at(const float* __restrict__ p, size_t member_stride, int E) {
    float mean = 0.f;
    for (int e = 0; e < E; ++e) mean += p[(size_t)e * member_stride];
    mean /= (float)E;
    float d2 = 0.f;
    for (int e = 0; e < E; ++e) {
        const float d = p[(size_t)e * member_stride] - mean;
        d2 = fmaf(d, d, d2);
    }
    return d2 / (float)(E - 1);
}

// One block's share of one frame: xt = the frame in member 0 (member e lies e * member_stride floats further), m_frame = the frame's row of the map or
// null, out = where this block's partial sum goes. Both kernels below are this body and nothing else, so a frame's numbers do not depend on
// which of them produced it.
template <int V>
__device__ __forceinline__ void frame_stats_block(const float* __restrict__ xt, size_t member_stride, float* __restrict__ m_frame,
                                                  double* __restrict__ out, int E, int C, int hw) {
    __shared__ double red[RW_THREADS];
    const int groups = hw / V;   // (V = 4 only where hw % 4 == 0)
    double acc = 0.0;
    for (int g = blockIdx.x * RW_THREADS + threadIdx.x; g < groups; g += VK_FRAME_STATS_BLOCKS * RW_THREADS) {
        float msum[V];
#pragma unroll
        for (int j = 0; j < V; ++j) msum[j] = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* p = xt + (size_t)c * hw + (size_t)g * V;
            float v[V];
            if (V == 4) {
                float mean[4] = {0.f, 0.f, 0.f, 0.f}, d2[4] = {0.f, 0.f, 0.f, 0.f};
                for (int e = 0; e < E; ++e) {
                    const float4 q = *reinterpret_cast<const float4*>(p + (size_t)e * member_stride);
                    mean[0] += q.x; mean[1] += q.y; mean[2] += q.z; mean[3] += q.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) mean[j] /= (float)E;
                for (int e = 0; e < E; ++e) {
                    const float4 q = *reinterpret_cast<const float4*>(p + (size_t)e * member_stride);
                    const float d0 = q.x - mean[0], d1 = q.y - mean[1], d2_ = q.z - mean[2], d3 = q.w - mean[3];
                    d2[0] = fmaf(d0, d0, d2[0]); d2[1] = fmaf(d1, d1, d2[1]); d2[2] = fmaf(d2_, d2_, d2[2]); d2[3] = fmaf(d3, d3, d2[3]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = d2[j] / (float)(E - 1);
            } else {
                v[0] = ens_var_at(p, member_stride, E);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc += (double)v[j];
                msum[j] += v[j];
            }
        }
        if (m_frame) {
            float* m = m_frame + (size_t)g * V;
            if (V == 4) {
                float4 o;
                o.x = msum[0] / (float)C; o.y = msum[1] / (float)C; o.z = msum[2] / (float)C; o.w = msum[3] / (float)C;
                *reinterpret_cast<float4*>(m) = o;
            } else {
                m[0] = msum[0] / (float)C;
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = RW_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

template <int V>
__global__ __launch_bounds__(RW_THREADS) void frame_stats_kernel(const float* __restrict__ x, float* __restrict__ map, double* __restrict__ partial,
                                                                 int E, int T, int C, int hw) {
    const int t = blockIdx.y;
    const size_t frame = (size_t)C * hw;
    frame_stats_block<V>(x + (size_t)t * frame, (size_t)T * frame, map ? map + (size_t)t * hw : nullptr,
                         partial + (size_t)t * VK_FRAME_STATS_BLOCKS + blockIdx.x, E, C, hw);
}

// ---- the same statistics for K candidates' ensembles at once (the planner's round) ------------------------------------------------------------
// x [K][E][T][C][hw]; block (b, tt, k) is block (b, t0 + tt) of frame_stats_kernel on candidate k's ensemble: frames before t0 are never read.
template <int V>
__global__ __launch_bounds__(RW_THREADS) void candidate_stats_kernel(const float* __restrict__ x, float* __restrict__ map,
                                                                     double* __restrict__ partial, int E, int T, int t0, int C, int hw) {
    const int tt = blockIdx.y, k = blockIdx.z, Ts = T - t0;
    const size_t frame = (size_t)C * hw;
    const size_t row = (size_t)k * Ts + tt;   // (k, tt) in frame_sum / map / partial
    frame_stats_block<V>(x + ((size_t)k * E * T + (size_t)(t0 + tt)) * frame, (size_t)T * frame, map ? map + row * hw : nullptr,
                         partial + row * VK_FRAME_STATS_BLOCKS + blockIdx.x, E, C, hw);
}

// One block: (1) a thread per (candidate, frame) adds the frame's partials in block order, as frame_stats_fold_kernel does; (2) a thread per
// candidate adds its frame sums in frame order; (3) thread 0 picks the smallest total -- ties to the lowest index, a NaN never, -1 if all are NaN.
__global__ __launch_bounds__(RW_THREADS) void candidate_fold_select_kernel(const double* __restrict__ partial, double* __restrict__ frame_sum,
                                                                           double* __restrict__ total, int32_t* __restrict__ best, int K, int Ts) {
    const long long rows = (long long)K * Ts;
    for (long long r = threadIdx.x; r < rows; r += RW_THREADS) {
        double a = 0.0;
        for (int b = 0; b < VK_FRAME_STATS_BLOCKS; ++b) a += partial[(size_t)r * VK_FRAME_STATS_BLOCKS + b];
        frame_sum[r] = a;
    }
    __syncthreads();   // (orders the block's global writes before its reads below)
    for (int k = threadIdx.x; k < K; k += RW_THREADS) {
        double a = 0.0;
        for (int t = 0; t < Ts; ++t) a += frame_sum[(size_t)k * Ts + t];
        total[k] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int arg = -1;
        double least = 0.0;
        for (int k = 0; k < K; ++k) {
            const double v = total[k];
            if (v != v) continue;
            if (arg < 0 || v < least) {
                arg = k;
                least = v;
            }
        }
        *best = arg;
    }
}

// one thread per frame adds the frame's VK_FRAME_STATS_BLOCKS partials in block order
__global__ void frame_stats_fold_kernel(const double* __restrict__ partial, double* __restrict__ frame_sum, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double a = 0.0;
    for (int b = 0; b < VK_FRAME_STATS_BLOCKS; ++b) a += partial[(size_t)t * VK_FRAME_STATS_BLOCKS + b];
    frame_sum[t] = a;
}

// ---- heat overlay ---------------------------------------------------------------------------------------------------------------------------
__host__ inline int rw_grid(long long n) {
    long long g = (n + RW_THREADS - 1) / RW_THREADS;
    const long long cap = 256LL * 32;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// one rounding per operation (the numpy float32 expression, as csrc/image_io.hip's to_u8), truncating cast. The blend is a multiply followed
// by an add: contraction is switched off for this function, so that neither becomes part of an FMA (the __f*_rn intrinsics are plain
// operators in this toolchain's headers and would not prevent it).
__device__ __forceinline__ void heat_px(float r, float g, float b, float m, float inv_vmax, float alpha, uint32_t* px) {
#pragma clang fp contract(off)
    const float a = alpha * fminf(1.0f, m * inv_vmax);
    const float f[3] = {r, g, b};
    const float K[3] = {255.0f, 32.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = f[c] + 1.0f;
        const float fc = (255.0f * s) * 0.5f;   // vk_frames_to_u8(real = 1) before its cast (* 0.5f is exact: the reference divides by 2.0)
        const float d = K[c] - fc;
        const float ad = a * d;
        const float v = fc + ad;
        px[c] = (uint32_t)((int)v) & 0xffu;
    }
}

__global__ void heat_overlay_kernel(const float* __restrict__ x, const float* __restrict__ map, uint8_t* __restrict__ out, int n_img, int H, int W,
                                    int cell, float inv_vmax, float alpha) {
    const int groups = (W + 3) >> 2;
    const long long total = (long long)n_img * H * groups;
    const bool wide = (W & 3) == 0;   // whole groups: 16-byte aligned fp32 rows, 12 bytes out on a 4-byte boundary
    const size_t plane = (size_t)H * W;
    const int mw = W / cell, mh = H / cell;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(i % groups);
        const long long r = i / groups;
        const int img = (int)(r / H), y = (int)(r - (long long)img * H);
        const float* p = x + (size_t)img * 3 * plane + (size_t)y * W + g * 4;
        const float* mrow = map + ((size_t)img * mh + y / cell) * mw;
        uint8_t* dst = out + ((size_t)r * W + g * 4) * 3;
        uint32_t px[12];
        if (wide) {
            const float4 vr = *reinterpret_cast<const float4*>(p);
            const float4 vg = *reinterpret_cast<const float4*>(p + plane);
            const float4 vb = *reinterpret_cast<const float4*>(p + 2 * plane);
            const int x0 = g * 4;
            heat_px(vr.x, vg.x, vb.x, mrow[x0 / cell], inv_vmax, alpha, px);
            heat_px(vr.y, vg.y, vb.y, mrow[(x0 + 1) / cell], inv_vmax, alpha, px + 3);
            heat_px(vr.z, vg.z, vb.z, mrow[(x0 + 2) / cell], inv_vmax, alpha, px + 6);
            heat_px(vr.w, vg.w, vb.w, mrow[(x0 + 3) / cell], inv_vmax, alpha, px + 9);
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int q = 0; q < 3; ++q) d32[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | (px[4 * q + 3] << 24);
        } else {
            const int nx = min(4, W - g * 4);
            for (int e = 0; e < nx; ++e) {
                heat_px(p[e], p[plane + e], p[2 * plane + e], mrow[(g * 4 + e) / cell], inv_vmax, alpha, px);
                dst[3 * e] = (uint8_t)px[0];
                dst[3 * e + 1] = (uint8_t)px[1];
                dst[3 * e + 2] = (uint8_t)px[2];
            }
        }
    }
}

}  // namespace

extern "C" int vk_ensemble_frame_stats(const float* x, double* frame_sum, float* map, double* partial_ws, int32_t E, int32_t T, int32_t C,
                                       int32_t hw, void* stream) {
    if (!x || !frame_sum || !partial_ws || E < 2 || E > 64 || T <= 0 || C <= 0 || hw <= 0) return VK_EINVAL;
    if (T > 65535) return VK_EINVAL;   // (grid.y)
    const dim3 grid(VK_FRAME_STATS_BLOCKS, T);
    // 16-byte accesses only where every row of every member starts on a 16-byte boundary
    const bool vec = (hw % 4) == 0 && (((size_t)x) & 15) == 0 && (!map || (((size_t)map) & 15) == 0);
    if ((hw % 4) == 0 && !vec) return VK_EINVAL;   // a shape's path (and so its summation order) is a function of hw alone
    if (vec)
        hipLaunchKernelGGL(frame_stats_kernel<4>, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, x, map, partial_ws, E, T, C, hw);
    else
        hipLaunchKernelGGL(frame_stats_kernel<1>, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, x, map, partial_ws, E, T, C, hw);
    VK_CHECK_LAUNCH();
    hipLaunchKernelGGL(frame_stats_fold_kernel, dim3((T + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)partial_ws, frame_sum, T);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_candidate_frame_stats(const float* x, double* frame_sum, double* total, int32_t* best, float* map, double* partial_ws,
                                        int32_t K, int32_t E, int32_t T, int32_t t0, int32_t C, int32_t hw, void* stream) {
    if (!x || !frame_sum || !total || !best || !partial_ws || K < 1 || E < 2 || E > 64 || t0 < 0 || t0 >= T || C <= 0 || hw <= 0) return VK_EINVAL;
    const int Ts = T - t0;
    if (Ts > 65535 || K > 65535) return VK_EINVAL;   // (grid.y, grid.z)
    const dim3 grid(VK_FRAME_STATS_BLOCKS, Ts, K);
    // the rule of vk_ensemble_frame_stats: the path is a function of hw alone, and the 16-byte path needs its alignment
    const bool vec = (hw % 4) == 0 && (((size_t)x) & 15) == 0 && (!map || (((size_t)map) & 15) == 0);
    if ((hw % 4) == 0 && !vec) return VK_EINVAL;
    if (vec)
        hipLaunchKernelGGL(candidate_stats_kernel<4>, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, x, map, partial_ws, E, T, t0, C, hw);
    else
        hipLaunchKernelGGL(candidate_stats_kernel<1>, grid, dim3(RW_THREADS), 0, (hipStream_t)stream, x, map, partial_ws, E, T, t0, C, hw);
    VK_CHECK_LAUNCH();
    hipLaunchKernelGGL(candidate_fold_select_kernel, dim3(1), dim3(RW_THREADS), 0, (hipStream_t)stream, (const double*)partial_ws, frame_sum, total,
                       best, K, Ts);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_heat_overlay_u8(const float* frames, const float* map, void* out, int32_t n_img, int32_t H, int32_t W, int32_t cell,
                                  float inv_vmax, float alpha, void* stream) {
    if (!frames || !map || !out || n_img <= 0 || H <= 0 || W <= 0 || cell <= 0 || (H % cell) || (W % cell)) return VK_EINVAL;
    if (!(alpha >= 0.0f && alpha <= 1.0f) || !(inv_vmax >= 0.0f) || inv_vmax > 3.402823466e38f) return VK_EINVAL;   // (NaN fails both comparisons)
    if ((((size_t)frames) & 15) != 0 || (((size_t)out) & 3) != 0) return VK_EINVAL;
    if ((long long)n_img * H > 0x7fffffffLL) return VK_EINVAL;
    hipLaunchKernelGGL(heat_overlay_kernel, dim3(rw_grid((long long)n_img * H * ((W + 3) / 4))), dim3(RW_THREADS), 0, (hipStream_t)stream, frames,
                       map, (uint8_t*)out, n_img, H, W, cell, inv_vmax, alpha);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
