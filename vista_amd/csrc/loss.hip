// Denoising-loss front door (gfx950): the reference's StandardDiffusionLoss, forward only.
//   vk_loss_noise_input : x + (noise + level * offset) * ((1 - mask) * sigma), bit for bit torch's fp32 expression
//   vk_fourier_highpass : the reference's fourier_filter of every H x W plane -- 2-D DFT, byte mask (kept 1 / masked `scale`), inverse, real part
//   vk_loss_stats       : per frame the three sums the loss is assembled from (fp64, fixed order), the dynamics weight's norm per (clip, channel)
// fp32 latents in and out: no storage-type dependence, the same object code goes into both libraries (as csrc/reward.hip).
// The element kernels are HBM-bound without reuse: lanes walk the contiguous hw axis, 16 bytes per lane where hw % 4 == 0 and the pointers
// allow. The transform keeps a plane resident in LDS: one workgroup per plane, two complex fp32 buffers and two fp64 twiddle tables.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int HP_THREADS = 512;

// ---- noising ----------------------------------------------------------------------------------------------------------------------------------
// Operation by operation what the reference evaluates (loss.py: noise + level * offset; (1 - mask) * sigma; input + noise * sigmas_bc), each
// rounded once in fp32: contraction is switched off for this function so that no multiply and add become an FMA (as heat_px, csrc/reward.hip).
__device__ __forceinline__ float noise_el(float x, float nz, float lo, bool has_off, float s) {
#pragma clang fp contract(off)
    float n = nz;
    if (has_off) n = nz + lo;
    const float ns = n * s;
    return x + ns;
}

// x, noise, out [n][C][hw]; sigma, mask [n]; offset [n][C]. One (n, c) row per blockIdx.y, lanes over the row's groups of V elements.
template <int V>
__global__ __launch_bounds__(LS_THREADS) void noise_input_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                                 const float* __restrict__ sigma, const float* __restrict__ mask,
                                                                 const float* __restrict__ offset, float level, float* __restrict__ out,
                                                                 int rows, int C, int hw) {
#pragma clang fp contract(off)
    const int groups = hw / V;
    for (int row = blockIdx.y; row < rows; row += gridDim.y) {
        const int n = row / C;
        float s = sigma[n];
        if (mask) {
            const float keep = 1.0f - mask[n];
            s = keep * s;
        }
        float lo = 0.f;
        if (offset) lo = level * offset[row];
        const size_t base = (size_t)row * hw;
        for (int g = blockIdx.x * LS_THREADS + threadIdx.x; g < groups; g += gridDim.x * LS_THREADS) {
            const size_t i = base + (size_t)g * V;
            if (V == 4) {
                const float4 a = *reinterpret_cast<const float4*>(x + i);
                const float4 b = *reinterpret_cast<const float4*>(noise + i);
                float4 o;
                o.x = noise_el(a.x, b.x, lo, offset != nullptr, s);
                o.y = noise_el(a.y, b.y, lo, offset != nullptr, s);
                o.z = noise_el(a.z, b.z, lo, offset != nullptr, s);
                o.w = noise_el(a.w, b.w, lo, offset != nullptr, s);
                *reinterpret_cast<float4*>(out + i) = o;
            } else {
                out[i] = noise_el(x[i], noise[i], lo, offset != nullptr, s);
            }
        }
    }
}

// ---- Fourier high-pass ------------------------------------------------------------------------------------------------------------------------
// One workgroup per plane. LDS: twiddles of the row and the column transform as fp64 (cos, sin)(2 pi j / W), j < W, and (2 pi j / H), j < H, then
// two complex fp32 buffers bufA, bufB of H * W each. Four dense passes, every output a sum accumulated in fp64 and rounded to fp32 once:
//   1  A[h][kw] = sum_w d[h][w] e^{-2 pi i kw w / W}            (d is real: it lies in bufB's first half)
//   2  B[kh][kw] = keep[kh][kw] * sum_h A[h][kw] e^{-2 pi i kh h / H}      keep = 1 where the byte is set, `scale` elsewhere
//   3  A[h][kw] = sum_kh B[kh][kw] e^{+2 pi i kh h / H}
//   4  y[h][w] = Re sum_kw A[h][kw] e^{+2 pi i kw w / W} / (H W)  -> global
// Lanes walk the fastest output index: in passes 2 and 3 a wave reads consecutive complex elements of a row (8-byte stride: no bank conflict) and
// one twiddle (a broadcast). Passes 1 and 4 are NOT conflict-free: the plane element is a broadcast, but every lane reads its own 16-byte twiddle at
// index k * j mod N, a stride that changes with j and lands several lanes of a group on one bank. Left so: 100 planes of 72 x 128 take 0.38 ms
// against 83 ms for the forward they follow (profiles/diffusion_loss_parity.txt). The twiddle index is advanced by k and wrapped: no division
// in the loops.
// d is formed on load: a alone (b == NULL), a - b, or (a * (1 - m) + b * m) - b with m = cond_mask[plane / planes_per_image] -- fp32, one
// rounding per operation, nothing contracted (the reference's replace_cond_frames blend).
__device__ __forceinline__ float hp_load(const float* __restrict__ a, const float* __restrict__ b, bool has_m, float m, size_t i) {
#pragma clang fp contract(off)
    float p = a[i];
    if (!b) return p;
    const float t = b[i];
    if (has_m) {
        const float keep = 1.0f - m;
        const float pk = p * keep;
        const float tm = t * m;
        p = pk + tm;
    }
    return p - t;
}

__global__ __launch_bounds__(HP_THREADS) void fourier_highpass_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                      const float* __restrict__ cond_mask, const uint8_t* __restrict__ keep,
                                                                      float scale, float* __restrict__ y, int planes_per_image, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) char hp_lds[];
    double2* twW = reinterpret_cast<double2*>(hp_lds);
    double2* twH = twW + W;
    float2* bufA = reinterpret_cast<float2*>(twH + H);
    float2* bufB = bufA + (size_t)H * W;
    float* d = reinterpret_cast<float*>(bufB);
    const int tid = threadIdx.x, hwn = H * W;
    const size_t plane = (size_t)blockIdx.x * hwn;
    const bool has_m = cond_mask != nullptr && b != nullptr;
    const float m = has_m ? cond_mask[blockIdx.x / planes_per_image] : 0.f;

    for (int j = tid; j < W; j += HP_THREADS) {
        double s, c;
        sincospi(2.0 * (double)j / (double)W, &s, &c);
        twW[j] = make_double2(c, s);
    }
    for (int j = tid; j < H; j += HP_THREADS) {
        double s, c;
        sincospi(2.0 * (double)j / (double)H, &s, &c);
        twH[j] = make_double2(c, s);
    }
    for (int i = tid; i < hwn; i += HP_THREADS) d[i] = hp_load(a, b, has_m, m, plane + i);
    __syncthreads();

    // pass 1: rows, forward (e^{-i t} = cos t - i sin t)
    for (int o = tid; o < hwn; o += HP_THREADS) {
        const int h = o / W, kw = o - h * W;
        const float* row = d + h * W;
        double re = 0.0, im = 0.0;
        int j = 0;
        for (int w = 0; w < W; ++w) {
            const double v = (double)row[w];
            const double2 t = twW[j];
            re += v * t.x;
            im -= v * t.y;
            j += kw;
            if (j >= W) j -= W;
        }
        bufA[o] = make_float2((float)re, (float)im);
    }
    __syncthreads();
    // pass 2: columns, forward, then the mask
    for (int o = tid; o < hwn; o += HP_THREADS) {
        const int kh = o / W, kw = o - kh * W;
        double re = 0.0, im = 0.0;
        int j = 0;
        for (int h = 0; h < H; ++h) {
            const float2 v = bufA[h * W + kw];
            const double2 t = twH[j];
            re += (double)v.x * t.x + (double)v.y * t.y;
            im += (double)v.y * t.x - (double)v.x * t.y;
            j += kh;
            if (j >= H) j -= H;
        }
        float fr = (float)re, fi = (float)im;
        if (!keep[o]) {
            fr *= scale;
            fi *= scale;
        }
        bufB[o] = make_float2(fr, fi);
    }
    __syncthreads();
    // pass 3: columns, inverse (e^{+i t})
    for (int o = tid; o < hwn; o += HP_THREADS) {
        const int h = o / W, kw = o - h * W;
        double re = 0.0, im = 0.0;
        int j = 0;
        for (int kh = 0; kh < H; ++kh) {
            const float2 v = bufB[kh * W + kw];
            const double2 t = twH[j];
            re += (double)v.x * t.x - (double)v.y * t.y;
            im += (double)v.y * t.x + (double)v.x * t.y;
            j += h;
            if (j >= H) j -= H;
        }
        bufA[o] = make_float2((float)re, (float)im);
    }
    __syncthreads();
    // pass 4: rows, inverse, real part, 1 / (H W)
    const double inv = 1.0 / ((double)H * (double)W);
    for (int o = tid; o < hwn; o += HP_THREADS) {
        const int h = o / W, w = o - h * W;
        const float2* row = bufA + h * W;
        double re = 0.0;
        int j = 0;
        for (int kw = 0; kw < W; ++kw) {
            const float2 v = row[kw];
            const double2 t = twW[j];
            re += (double)v.x * t.x - (double)v.y * t.y;
            j += w;
            if (j >= W) j -= W;
        }
        y[plane + o] = (float)(re * inv);
    }
}

// ---- loss statistics --------------------------------------------------------------------------------------------------------------------------
// One element of predict = out * (1 - m) + target * m (fp32, one rounding per operation, as the reference's blend), or out where there is no mask.
__device__ __forceinline__ float blend_el(float o, float t, bool has_m, float m) {
#pragma clang fp contract(off)
    if (!has_m) return o;
    const float keep = 1.0f - m;
    const float ok = o * keep;
    const float tm = t * m;
    return ok + tm;
}

// dd = (target_t - target_{t-1}) - (predict_t - predict_{t-1});  a = dd^2 (l2) or |dd| (l1)
__device__ __forceinline__ float dyn_el(float pt, float pp, float tt, float tp, bool l1) {
#pragma clang fp contract(off)
    const float dt = tt - tp;
    const float dp = pt - pp;
    const float dd = dt - dp;
    return l1 ? fabsf(dd) : dd * dd;
}

template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, bool wide, float* v) {
    if (V == 4 && wide) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = p[j];
    }
}

__device__ __forceinline__ double block_sum(double acc, double* red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = LS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Pass 1. out, target [B * T][C][hw]. Block (j, c, b) adds, for t = 1 .. T - 1 in order, the groups g = j * 256 + tid + k * (VK_LOSS_STATS_BLOCKS * 256)
// of channel c of frame t of clip b (a group = V neighbouring elements, V = 4 where hw % 4 == 0): which thread adds which element is a function
// of T and hw alone, so a clip's norm does not depend on B or on the launch. l2: sum of a^2; l1: sum of a (the norms F.normalize divides by).
template <int V>
__global__ __launch_bounds__(LS_THREADS) void dyn_norm_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                              const float* __restrict__ cond_mask, double* __restrict__ partial, int T, int C,
                                                              int hw, int l1, int wide) {
    __shared__ double red[LS_THREADS];
    const int c = blockIdx.y, bclip = blockIdx.z, groups = hw / V;
    double acc = 0.0;
    for (int t = 1; t < T; ++t) {
        const size_t f1 = (size_t)bclip * T + t, f0 = f1 - 1;
        const bool has_m = cond_mask != nullptr;
        const float m1 = has_m ? cond_mask[f1] : 0.f, m0 = has_m ? cond_mask[f0] : 0.f;
        const size_t r1 = (f1 * C + c) * (size_t)hw, r0 = (f0 * C + c) * (size_t)hw;
        for (int g = blockIdx.x * LS_THREADS + threadIdx.x; g < groups; g += VK_LOSS_STATS_BLOCKS * LS_THREADS) {
            float o1[V], o0[V], t1[V], t0[V];
            load_v<V>(out + r1 + (size_t)g * V, wide, o1);
            load_v<V>(out + r0 + (size_t)g * V, wide, o0);
            load_v<V>(target + r1 + (size_t)g * V, wide, t1);
            load_v<V>(target + r0 + (size_t)g * V, wide, t0);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float av = dyn_el(blend_el(o1[j], t1[j], has_m, m1), blend_el(o0[j], t0[j], has_m, m0), t1[j], t0[j], l1 != 0);
                acc += l1 ? (double)av : (double)av * (double)av;
            }
        }
    }
    const double r = block_sum(acc, red);
    if (threadIdx.x == 0) partial[((size_t)bclip * C + c) * VK_LOSS_STATS_BLOCKS + blockIdx.x] = r;
}

// Pass 2. One block per frame f = b * T + t: thread tid adds the groups tid, tid + 256, ... of the frame's C * hw elements (channel-major, as they
// lie), then the block's tree. The clip's norms are folded first, by thread c < C, from pass 1's partials in block order and rounded to fp32 once.
//   sums[f] = (S0, S1, S2) = (sum e, sum e * aux_w, sum |hf|^p)
template <int V>
__global__ __launch_bounds__(LS_THREADS) void frame_sums_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                                const float* __restrict__ cond_mask, const float* __restrict__ hf,
                                                                const double* __restrict__ partial, double* __restrict__ sums, int T, int C,
                                                                int hw, int l1, int wide) {
#pragma clang fp contract(off)
    __shared__ double red[LS_THREADS];
    __shared__ float den[VK_LOSS_MAX_CHANNELS];
    const size_t f = blockIdx.x;
    const int bclip = (int)(f / T), t = (int)(f - (size_t)bclip * T);
    const bool first = t == 0, has_m = cond_mask != nullptr, has_hf = hf != nullptr;
    if (T > 1 && (int)threadIdx.x < C) {   // (T == 1: no differences, pass 1 did not run and den is never read)
        double n = 0.0;
        for (int j = 0; j < VK_LOSS_STATS_BLOCKS; ++j) n += partial[((size_t)bclip * C + threadIdx.x) * VK_LOSS_STATS_BLOCKS + j];
        const float nf = l1 ? (float)n : (float)sqrt(n);
        den[threadIdx.x] = fmaxf(nf, 1e-12f);   // F.normalize: v / max(||v||, eps), eps = 1e-12
    }
    __syncthreads();
    const float m1 = has_m ? cond_mask[f] : 0.f, m0 = (has_m && !first) ? cond_mask[f - 1] : 0.f;
    const int groups = hw / V, total = C * groups;
    const size_t r1 = f * C * (size_t)hw;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < total; i += LS_THREADS) {
        const int c = i / groups, g = i - c * groups;
        const size_t at = r1 + (size_t)c * hw + (size_t)g * V;
        float o1[V], t1[V], o0[V], t0[V], hv[V];
        load_v<V>(out + at, wide, o1);
        load_v<V>(target + at, wide, t1);
        if (!first) {
            load_v<V>(out + at - (size_t)C * hw, wide, o0);
            load_v<V>(target + at - (size_t)C * hw, wide, t0);
        }
        if (has_hf) load_v<V>(hf + at, wide, hv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float p = blend_el(o1[j], t1[j], has_m, m1);
            const float df = p - t1[j];
            const float e = l1 ? fabsf(df) : df * df;
            float ew = e;
            if (!first) {
                const float av = dyn_el(p, blend_el(o0[j], t0[j], has_m, m0), t1[j], t0[j], l1 != 0);
                const float q = av / den[c];
                const float aw = 1.0f + q;
                ew = e * aw;
            }
            s0 += (double)e;
            s1 += (double)ew;
            if (has_hf) {
                const float h = l1 ? fabsf(hv[j]) : hv[j] * hv[j];
                s2 += (double)h;
            }
        }
    }
    const double a0 = block_sum(s0, red), a1 = block_sum(s1, red), a2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        sums[f * 3] = a0;
        sums[f * 3 + 1] = a1;
        sums[f * 3 + 2] = a2;
    }
}

}  // namespace

extern "C" int vk_loss_noise_input(const float* x, const float* noise, const float* sigma, const float* mask, const float* offset, float level,
                                   float* out, int32_t n, int32_t C, int32_t hw, void* stream) {
    if (!x || !noise || !sigma || !out || n <= 0 || C <= 0 || hw <= 0) return VK_EINVAL;
    if ((long long)n * C > 0x7fffffffLL) return VK_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(noise, 4) || !aligned_to(out, 4) || !aligned_to(sigma, 4) || !aligned_to(mask, 4) || !aligned_to(offset, 4))
        return VK_EINVAL;
    const int rows = n * C;
    const bool vec = (hw % 4) == 0 && aligned_to(x, 16) && aligned_to(noise, 16) && aligned_to(out, 16);
    const int groups = vec ? hw / 4 : hw;
    int gx = (groups + LS_THREADS - 1) / LS_THREADS;
    if (gx > 1024) gx = 1024;
    const dim3 grid(gx, rows < 65535 ? rows : 65535);
    if (vec)
        hipLaunchKernelGGL(noise_input_kernel<4>, grid, dim3(LS_THREADS), 0, (hipStream_t)stream, x, noise, sigma, mask, offset, level, out, rows, C, hw);
    else
        hipLaunchKernelGGL(noise_input_kernel<1>, grid, dim3(LS_THREADS), 0, (hipStream_t)stream, x, noise, sigma, mask, offset, level, out, rows, C, hw);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_fourier_highpass_lds_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return VK_EINVAL;
    const long long bytes = 16LL * H * W + 16LL * ((long long)H + W);
    if (bytes > VK_HIGHPASS_LDS_BYTES) return VK_EINVAL;
    return (int)bytes;
}

extern "C" int vk_fourier_highpass(const float* a, const float* b, const float* cond_mask, const void* keep, float scale, float* y,
                                   int32_t planes, int32_t planes_per_image, int32_t H, int32_t W, void* stream) {
    if (!a || !keep || !y || planes <= 0 || planes_per_image <= 0 || H <= 0 || W <= 0) return VK_EINVAL;
    if (cond_mask && !b) return VK_EINVAL;
    if (y == a || y == b) return VK_EINVAL;
    if (!aligned_to(a, 4) || !aligned_to(b, 4) || !aligned_to(cond_mask, 4) || !aligned_to(y, 4)) return VK_EINVAL;
    const int lds = vk_fourier_highpass_lds_bytes(H, W);
    if (lds < 0) return VK_EINVAL;   // a plane the workgroup cannot hold: refused before any HIP call
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)fourier_highpass_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return VK_ELAUNCH;
    hipLaunchKernelGGL(fourier_highpass_kernel, dim3((unsigned)planes), dim3(HP_THREADS), (size_t)lds, (hipStream_t)stream, a, b, cond_mask,
                       (const uint8_t*)keep, scale, y, planes_per_image, H, W);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_loss_stats(const float* out, const float* target, const float* cond_mask, const float* hf, double* sums, double* partial_ws,
                             int32_t B, int32_t T, int32_t C, int32_t hw, int32_t l1, void* stream) {
    if (!out || !target || !sums || B <= 0 || T <= 0 || C <= 0 || hw <= 0) return VK_EINVAL;
    const bool dynamics = T > 1;   // T == 1 has no frame differences: launch 1 and its workspace are not needed
    if (dynamics && (!partial_ws || B > 65535)) return VK_EINVAL;   // (B is launch 1's grid.z)
    if (C > VK_LOSS_MAX_CHANNELS || (long long)B * T > 0x7fffffffLL || (long long)C * hw > 0x7fffffffLL) return VK_EINVAL;
    if (l1 != 0 && l1 != 1) return VK_EINVAL;
    if (!aligned_to(out, 4) || !aligned_to(target, 4) || !aligned_to(cond_mask, 4) || !aligned_to(hf, 4) || !aligned_to(sums, 8) ||
        !aligned_to(partial_ws, 8))
        return VK_EINVAL;
    // the grouping (and with it the order of every sum) is a function of hw alone; 16-byte loads are taken where the pointers allow them
    const int wide = (hw % 4) == 0 && aligned_to(out, 16) && aligned_to(target, 16) && aligned_to(hf, 16);
    const dim3 g1(VK_LOSS_STATS_BLOCKS, C, B), g2((unsigned)(B * T));
    if ((hw % 4) == 0) {
        if (dynamics) {
            hipLaunchKernelGGL(dyn_norm_kernel<4>, g1, dim3(LS_THREADS), 0, (hipStream_t)stream, out, target, cond_mask, partial_ws, T, C, hw, l1, wide);
            VK_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(frame_sums_kernel<4>, g2, dim3(LS_THREADS), 0, (hipStream_t)stream, out, target, cond_mask, hf,
                           (const double*)partial_ws, sums, T, C, hw, l1, wide);
    } else {
        if (dynamics) {
            hipLaunchKernelGGL(dyn_norm_kernel<1>, g1, dim3(LS_THREADS), 0, (hipStream_t)stream, out, target, cond_mask, partial_ws, T, C, hw, l1, 0);
            VK_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(frame_sums_kernel<1>, g2, dim3(LS_THREADS), 0, (hipStream_t)stream, out, target, cond_mask, hf,
                           (const double*)partial_ws, sums, T, C, hw, l1, 0);
    }
    VK_CHECK_LAUNCH();
    return VK_OK;
}
