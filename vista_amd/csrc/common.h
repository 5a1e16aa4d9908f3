// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of the Vista denoising hot path.
// Everything here is written for MI355X only: 64-lane wavefronts, MFMA 32x32x16 bf16, 160 KiB LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // one MFMA A/B operand (8 bf16, 4 VGPRs)
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // 32x32 MFMA accumulator
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

#define VK_WAVE 64

// ---- the 16-bit STORAGE type of the build ----------------------------------------------------------------------------------------------------
// Default build (libvista_hip.so): every activation and weight is bf16 (BASELINE config 2 names bf16). -DVK_F16=1 (libvista_hip_f16.so, round 6):
// the same kernels with IEEE fp16 storage and v_mfma_f32_32x32x16_f16 -- the reference's own autocast width (sample_utils.py:301-303), 3 more
// mantissa bits at the same MFMA rate and the same instruction counts (v_cvt_pk_f16_f32 / v_cvt_f32_f16 / v_dot2c_f32_f16 exist on gfx950).
// The helpers below keep their historical "bf16" names: they pack / unpack THE STORAGE TYPE. What stays bf16 in both builds has its own names
// (*_bf16x): the softmax numerators P and the V operand of the attention P.V product -- the zero-base softmax needs bf16's exponent range
// (attention.hip), so the q|k|v projections of an fp16 build write their V column block as bf16 (VkGemmDesc.alt_cols_from).
#ifndef VK_F16
#define VK_F16 0
#endif
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;

__device__ __forceinline__ float bf16x_lo(uint32_t u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16x_hi(uint32_t u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
// two fp32 -> packed bf16x2 (round-to-nearest-even; lowers to v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ uint32_t pack_bf16x(float a, float b) {
    f32x2_t v = {a, b};
    bf16x2_t r = __builtin_convertvector(v, bf16x2_t);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ f32x16_t vk_mfma_bf16x(bf16x8_t a, bf16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

#if VK_F16
__device__ __forceinline__ float bf16_lo(uint32_t u) { return (float)__builtin_bit_cast(f16x2_t, u)[0]; }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return (float)__builtin_bit_cast(f16x2_t, u)[1]; }
__device__ __forceinline__ float bf16_to_f32(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
// two fp32 -> packed fp16x2 (round-to-nearest-even: v_cvt_pk_f16_f32; values beyond 65504 become inf -- the reference's autocast does the same)
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    f32x2_t v = {a, b};
    f16x2_t r = __builtin_convertvector(v, f16x2_t);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ f32x16_t vk_mfma(bf16x8_t a, bf16x8_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
// sum += x.lo * y.lo + x.hi * y.hi on packed pairs of the storage type (v_dot2c_f32_f16)
__device__ __forceinline__ float vk_dot2(uint32_t x, uint32_t y, float acc) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, x), __builtin_bit_cast(f16x2_t, y), acc, false);
}
#define VK_ONE_PAIR 0x3c003c00u   // (1, 1) in the storage type
#else
__device__ __forceinline__ float bf16_lo(uint32_t u) { return bf16x_lo(u); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return bf16x_hi(u); }
__device__ __forceinline__ float bf16_to_f32(uint16_t u) { return __builtin_bit_cast(float, ((uint32_t)u) << 16); }
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) { return pack_bf16x(a, b); }
__device__ __forceinline__ f32x16_t vk_mfma(bf16x8_t a, bf16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float vk_dot2(uint32_t x, uint32_t y, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, x), __builtin_bit_cast(bf16x2_t, y), acc, false);
}
#define VK_ONE_PAIR 0x3f803f80u
#endif
__device__ __forceinline__ uint16_t f32_to_bf16(float a) { return (uint16_t)(pack_bf16(a, 0.f) & 0xffffu); }

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    f[0] = bf16_lo(v.x); f[1] = bf16_hi(v.x);
    f[2] = bf16_lo(v.y); f[3] = bf16_hi(v.y);
    f[4] = bf16_lo(v.z); f[5] = bf16_hi(v.z);
    f[6] = bf16_lo(v.w); f[7] = bf16_hi(v.w);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 v;
    v.x = pack_bf16(f[0], f[1]); v.y = pack_bf16(f[2], f[3]);
    v.z = pack_bf16(f[4], f[5]); v.w = pack_bf16(f[6], f[7]);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- lane-pair helpers of the 32x32 MFMA accumulator layout (GEMM epilogues, attention output stores) ----
// Accumulator element r = 4*g + e: lane l31 of the lower half-wave (lh = 0) holds columns c..c+3 of accumulator quad g and lane l31 of the
// upper half the next four, for the SAME output row. Swapping the upper half of quad g with the lower half of quad g+1 (v_permlane32_swap)
// leaves the lower lane with 8 contiguous bf16 of quad g and the upper lane with 8 contiguous bf16 of quad g+1: one 16-byte store instead
// of two 8-byte ones. The epilogue of the GEMMs is store-ISSUE bound (16-40 stores per lane), so halving the count matters most
// where tiles are short (K = 320: 5 K-steps per tile).
__device__ __forceinline__ uint4 widen_pair(uint2 qa, uint2 qb) {
    const auto rx = __builtin_amdgcn_permlane32_swap(qa.x, qb.x, false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(qa.y, qb.y, false, false);
    return make_uint4(rx[0], ry[0], rx[1], ry[1]);
}

// The inverse, for loads: the lower lane read the 8 contiguous bf16 of quad g (its own 4 and its partner's 4), the upper lane those of
// quad g+1; two swaps hand every lane its own 4 values of both quads.
__device__ __forceinline__ void unwiden_pair(const uint4& w, uint2& qa, uint2& qb) {
    const auto rx = __builtin_amdgcn_permlane32_swap(w.x, w.z, false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(w.y, w.w, false, false);
    qa = make_uint2(rx[0], ry[0]);
    qb = make_uint2(rx[1], ry[1]);
}

__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (uint32_t)v;
}

// MX-fp8 quantisation of ONE 32-column block of an output row held as the four accumulator quads of a 32x32 fragment: lane half lh holds
// columns 8g + 4lh + e (g = quad, e = 0..3), i.e. 16 of the 32 values; its partner lane (l ^ 32) the others. Returns the lane's 16 bytes
// of the block's 32 e4m3 bytes (to be stored at byte offset 16*lh of the block) and the block's E8M0 exponent byte (both lanes get it):
// 2^(ex) >= max|v| / 448, the smallest such power of two (frexp), so every value lands in e4m3's range with at most one binade unused.
__device__ __forceinline__ uint4 mx_quant_block(const float (&v)[4][4], int& e8m0) {
    float amax = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[g][e]));
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    int ex = -127;
    if (amax > 0.f) frexpf(amax * (1.f / 448.f), &ex);  // amax/448 = f * 2^ex, f in [0.5, 1)
    ex = ex < -127 ? -127 : (ex > 127 ? 127 : ex);
    const float inv = ldexpf(1.f, -ex);
    uint32_t q[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) q[g] = pack_fp8x4(v[g][0] * inv, v[g][1] * inv, v[g][2] * inv, v[g][3] * inv);
    // lower lane: [own q0 | partner q0 | own q1 | partner q1] = columns 0-15; upper lane: [partner q2 | own q2 | partner q3 | own q3] = 16-31
    const auto r02 = __builtin_amdgcn_permlane32_swap(q[0], q[2], false, false);
    const auto r13 = __builtin_amdgcn_permlane32_swap(q[1], q[3], false, false);
    e8m0 = ex + 127;
    return make_uint4(r02[0], r02[1], r13[0], r13[1]);
}

__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
// erf-form GELU (F.gelu default, reference vwm/modules/attention.py:92): x * Phi(x) with the normal CDF as a logistic of an odd quintic,
// Phi(x) ~= 1 / (1 + exp(-x (a + b x^2 + c x^4))), a = 1.59501577, b = 7.40112920e-2, c = -7.03033577e-4 (minimax fit of x * Phi(x) over
// |x| <= 12; x^2 clamped at 50 where the quintic would turn around and Phi is 0 / 1 in fp32 anyway). |x Phi(x) - gelu(x)| <= 2.6e-5
// everywhere in fp32 (tests/test_host_cpu.py evaluates this very formula) -- a hundred times below the bf16 resolution of the values the
// GEGLU epilogue stores. 7 plain VALU ops + 2 transcendentals per gate, against 15 + 2 for the erfc form (Abramowitz-Stegun 7.1.26) it
// replaces: the GEGLU epilogue is VALU-bound with every wave of the CU in it at once, and the gelu was half of its instructions.
__device__ __forceinline__ float gelu_erf_f(float x) {
    const float u = fminf(x * x, 50.f);
    const float t = fmaf(u, fmaf(u, 0.0010142630f, -0.10677572f), -2.3011212f);  // -(a + b u + c u^2) * log2(e)
    return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * t));
}

// XCD-aware, bijective block remap (8 XCDs, block b is observed on XCD b%8): gives each XCD a
// contiguous range of logical tile ids so neighbouring tiles share that XCD's private L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int nx = 8;
    int xcd = bid % nx, slot = bid / nx;
    int q = nblk / nx, r = nblk % nx;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

// Counted wait on the wave's vector-memory queue: at most N operations outstanding, i.e. everything but the N youngest has landed (loads retire in
// order among themselves). The pipelined kernels keep their youngest LDS-DMA pieces in flight across a barrier with it.
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// s_memtime stamp of the timing builds (-DPIPE_TIMING / -DGS_TIMING / -DFF_TIMING: tools/build_variant.sh); the product build has no caller
__device__ __forceinline__ unsigned long long vk_stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}

// error codes returned by the C-ABI launchers
#define VK_OK 0
#define VK_EINVAL (-22)
#define VK_ELAUNCH (-5)

#define VK_CHECK_LAUNCH() do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return VK_ELAUNCH; } while (0)

// operand contract (include/vista_hip.h): is `p` a multiple of `a` bytes (a power of two)? NULL is: an absent optional operand is not checked
static inline bool aligned_to(const void* p, size_t a) { return (((size_t)p) & (a - 1)) == 0; }
