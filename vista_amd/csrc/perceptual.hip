// CLIP-space scores of predicted frames (gfx950): the three kernels under vista_amd/perceptual.py.
//   vk_clip_preprocess_patches_u8 : vk_clip_preprocess_patches reading the (n, H, W, 3) uint8 stacks vk_frames_to_u8 writes. A byte b stands for
//                                   (float)b / 127.5f - 1.0f; from there the arithmetic is clip_resample.h's, shared with the fp32 kernel, so the
//                                   output equals that kernel's on the converted frames bit for bit.
//   vk_embed_row_stats            : per row of two (n, d) fp32 matrices a.b, a.a, b.b in fp64, one fixed order for all three
//   vk_embed_mmd_sums             : the three pair sums of a Gaussian-kernel MMD over row-normalised embeddings, fp64, fixed order
// No float atomics anywhere: partials go to the caller's workspace and a fold adds them in a fixed order; two calls give the same bits.
// Only the 16-bit store of the first kernel sees the storage type (it writes what vk_clip_preprocess_patches of the same library writes).
#include "common.h"
#include "clip_resample.h"
#include "vista_hip.h"

namespace {

constexpr int PC_THREADS = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {   // fixed order: lane l takes l + 32, then + 16, ...
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// lanes by shuffle, then the four waves in wave order; the sum is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_sum_f64(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < PC_THREADS / 64; ++w) s += red[w];
    __syncthreads();   // (red may be used again)
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- (a) preprocessing from bytes
// One fp32 division, one fp32 subtraction, nothing contracted: what `u8.float() / 127.5 - 1.0` computes.
__device__ __forceinline__ float byte_to_unit(uint32_t b) {
#pragma clang fp contract(off)
    const float q = (float)b / 127.5f;
    return q - 1.0f;
}

// The first and last source index the outputs o0 .. o1 of one axis read: bicubic taps iy - 1 .. iy + 2 clamped to the image, each widened by
// the blur's radius and reflected at the border. Reflection maps into the same range: an index -j (j <= radius) becomes j, and the range
// starts at 0 and reaches at least min(size - 1, radius) then; likewise at the far border.
__host__ __device__ inline void src_range(int o0, int o1, int size, int out_hw, int ks, int* lo, int* hi) {
    const float scale = out_hw > 1 ? (float)(size - 1) / (float)(out_hw - 1) : 0.f;
    int a = (int)floorf(out_hw > 1 ? (float)o0 * scale : 0.f) - 1, b = (int)floorf(out_hw > 1 ? (float)o1 * scale : 0.f) + 2;
    a = a < 0 ? 0 : (a > size - 1 ? size - 1 : a);
    b = b < 0 ? 0 : (b > size - 1 ? size - 1 : b);
    a -= ks / 2;
    b += ks / 2;
    *lo = a < 0 ? 0 : a;
    *hi = b > size - 1 ? size - 1 : b;
}

// grid (tiles * tiles, n): one workgroup owns a tile x tile block of output pixels of one frame, all three channels. It stages the source
// rectangle those outputs read into LDS as fp32, planar per channel ([3][rows_max][cols_max], dynamic), converting every byte once, and then
// every thread below tile * tile runs clip_resample over the LDS planes for its pixel.
// WIDE (W % 4 == 0, a 4-byte aligned stack): every row of every frame starts on a 4-byte boundary and is a whole number of dwords long, so
// the rectangle is loaded a dword per lane from the dword that holds its first byte, and no dword reaches past its row. Any other W or base: a
// byte per lane.
// A rectangle larger than the (rows_max, cols_max) the host sized the LDS for is never staged: the workgroup returns, its outputs stay zero.
template <bool WIDE>
__global__ __launch_bounds__(PC_THREADS) void clip_preprocess_u8_kernel(const uint8_t* __restrict__ img, uint16_t* __restrict__ out, int H, int W,
                                                                        int out_hw, int ps, int ldo, float sig_y, float sig_x, int ks_y, int ks_x,
                                                                        float m0, float m1, float m2, float s0, float s1, float s2, int tile,
                                                                        int rows_max, int cols_max) {
    extern __shared__ __attribute__((aligned(16))) float px[];
    __shared__ float gy[CLIP_MAX_KS], gx[CLIP_MAX_KS];
    const int tid = threadIdx.x;
    float ny, nx;
    clip_gauss_taps(gy, gx, ks_y, ks_x, sig_y, sig_x, ny, nx);
    const int tiles = (out_hw + tile - 1) / tile;
    const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
    const int oy0 = ty * tile, ox0 = tx * tile;
    const int oy1 = min(oy0 + tile, out_hw) - 1, ox1 = min(ox0 + tile, out_hw) - 1;
    int row_lo, row_hi, col_lo, col_hi;
    src_range(oy0, oy1, H, out_hw, ks_y, &row_lo, &row_hi);
    src_range(ox0, ox1, W, out_hw, ks_x, &col_lo, &col_hi);
    const int rows = row_hi - row_lo + 1, cols = col_hi - col_lo + 1;
    if (rows > rows_max || cols > cols_max) return;   // (uniform over the workgroup)
    const size_t row_bytes = (size_t)W * 3;
    const uint8_t* frame = img + (size_t)blockIdx.y * H * row_bytes;
    const int b_lo = col_lo * 3, b_hi = (col_hi + 1) * 3;   // the rectangle's bytes of a row: [b_lo, b_hi)
    const int plane = rows_max * cols_max;
    if (WIDE) {
        const int d_lo = b_lo >> 2, nd = ((b_hi + 3) >> 2) - d_lo;   // (row_bytes % 4 == 0 and b_hi <= row_bytes: the last dword ends inside the row)
        for (int i = tid; i < rows * nd; i += PC_THREADS) {
            const int r = i / nd, d = d_lo + (i - r * nd);
            const uint32_t v = *reinterpret_cast<const uint32_t*>(frame + (size_t)(row_lo + r) * row_bytes + (size_t)d * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = d * 4 + k;
                if (j >= b_lo && j < b_hi) {
                    const int col = j / 3, ch = j - col * 3;
                    px[ch * plane + r * cols_max + (col - col_lo)] = byte_to_unit((v >> (8 * k)) & 0xffu);
                }
            }
        }
    } else {
        const int nb = b_hi - b_lo;
        for (int i = tid; i < rows * nb; i += PC_THREADS) {
            const int r = i / nb, j = b_lo + (i - r * nb);
            const int col = j / 3, ch = j - col * 3;
            px[ch * plane + r * cols_max + (col - col_lo)] = byte_to_unit(frame[(size_t)(row_lo + r) * row_bytes + j]);
        }
    }
    __syncthreads();
    if (tid >= tile * tile) return;
    const int ly = tid / tile, lx = tid - ly * tile;
    const int oy = oy0 + ly, ox = ox0 + lx;
    if (oy > oy1 || ox > ox1) return;
    const int gp = out_hw / ps;
    const int py = oy / ps, ky = oy - py * ps, pxi = ox / ps, kx = ox - pxi * ps;
    uint16_t* dst = out + ((size_t)blockIdx.y * (1 + gp * gp) + 1 + py * gp + pxi) * ldo + ky * ps + kx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* pl = px + c * plane;
        const float acc = clip_resample([=](int y) { return pl + (y - row_lo) * cols_max - col_lo; }, oy, ox, H, W, out_hw, gy, gx, ks_y, ks_x,
                                        ny, nx);
        const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
        dst[c * ps * ps] = f32_to_bf16(clip_normalise(acc, mean, sd));
    }
}

constexpr int CLIP_U8_LDS_FLOATS = 15 * 1024;   // 60 KiB of dynamic LDS beside the two tap tables: three workgroups per CU where a tile needs 45 KiB

// the largest source rectangle any tile of `tile` x `tile` outputs reads
__host__ inline void tile_extent(int size, int out_hw, int ks, int tile, int* extent) {
    int worst = 0;
    for (int o0 = 0; o0 < out_hw; o0 += tile) {
        int lo, hi;
        const int o1 = (o0 + tile < out_hw ? o0 + tile : out_hw) - 1;
        src_range(o0, o1, size, out_hw, ks, &lo, &hi);
        worst = hi - lo + 1 > worst ? hi - lo + 1 : worst;
    }
    *extent = worst;
}

// ---------------------------------------------------------------------------------------------------------------- (b) row statistics
// grid (n): thread t adds the products of columns t, t + 256, ... in that order, the threads are added by block_sum_f64. The three sums are the
// same function of d, and a product of two fp32 values is exact in fp64: with a == b the three results are the same bits.
__global__ __launch_bounds__(PC_THREADS) void embed_row_stats_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                     double* __restrict__ out, int d) {
    __shared__ double red[PC_THREADS / 64];
    const float* ra = a + (size_t)blockIdx.x * d;
    const float* rb = b + (size_t)blockIdx.x * d;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int k = threadIdx.x; k < d; k += PC_THREADS) {
        const double x = (double)ra[k], y = (double)rb[k];
        ab += x * y;
        aa += x * x;
        bb += y * y;
    }
    ab = block_sum_f64(ab, red);
    aa = block_sum_f64(aa, red);
    bb = block_sum_f64(bb, red);
    if (threadIdx.x == 0) {
        out[(size_t)blockIdx.x * 3 + 0] = ab;
        out[(size_t)blockIdx.x * 3 + 1] = aa;
        out[(size_t)blockIdx.x * 3 + 2] = bb;
    }
}

// ---------------------------------------------------------------------------------------------------------------- (c) MMD pair sums
constexpr int MT = VK_EMBED_MMD_TILE;   // 64 x 64 pairs per workgroup, 4 x 4 per thread
constexpr int KT = 32;                  // columns staged per step
constexpr int KROW = KT + 4;            // LDS row stride in floats: 16 rows read 16 bytes each at one column hit 16 different groups of 4 banks
static_assert(MT == 64 && PC_THREADS == 256 && KT % 4 == 0, "the thread maps below are written for 64 x 64 tiles and 256 threads");

// grid (m + n): the fp32 inverse norm of every row of x, then of y, from the fp64 sum of squares (the order of embed_row_stats_kernel).
// A zero row gives inf, a row with a non-finite value NaN: every pair sum that row is in is then NaN.
__global__ __launch_bounds__(PC_THREADS) void embed_inv_norm_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ inv,
                                                                    int m, int d) {
    __shared__ double red[PC_THREADS / 64];
    const int r = blockIdx.x;
    const float* row = r < m ? x + (size_t)r * d : y + (size_t)(r - m) * d;
    double ss = 0.0;
    for (int k = threadIdx.x; k < d; k += PC_THREADS) {
        const double v = (double)row[k];
        ss += v * v;
    }
    ss = block_sum_f64(ss, red);
    if (threadIdx.x == 0) inv[r] = (float)(1.0 / sqrt(ss));
}

// grid (T, T, 3), T = ceil(max(m, n) / 64). z = 0: pairs of x with x, i < j; z = 1: y with y, i < j; z = 2: every x with every y. Workgroup
// (bj, bi) owns the pairs of rows 64 bi .. + 63 of the first set with rows 64 bj .. + 63 of the second; it stages both sets' rows, each times
// its inverse norm, 32 columns at a time, and thread (ty, tx) runs the sixteen pairs (ty + 16 p, tx + 16 q): per pair one fp32 sum over the
// columns in ascending order of the squared fp32 difference (an FMA of the difference with itself into the sum), then 1 - k as -expm1f of
// -gamma times that sum, added in fp64 in the order (p, q). Two equal rows give differences of 0, a sum of 0 and a term of exactly 0.
// Every workgroup writes its partial, also the ones that own no pair (0): the fold reads all T * T of a sum.
__global__ __launch_bounds__(PC_THREADS) void embed_mmd_tile_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ inv, double* __restrict__ part, int m, int n, int d,
                                                                    float gamma) {
    __shared__ __attribute__((aligned(16))) float sa[MT * KROW];
    __shared__ __attribute__((aligned(16))) float sb[MT * KROW];
    __shared__ double red[PC_THREADS / 64];
    const int z = blockIdx.z, bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x;
    const float* A = z == 1 ? y : x;
    const float* B = z == 0 ? x : y;
    const float* invA = z == 1 ? inv + m : inv;
    const float* invB = z == 0 ? inv : inv + m;
    const int na = z == 1 ? n : m, nb = z == 0 ? m : n;
    const bool tri = z != 2;
    const int i0 = bi * MT, j0 = bj * MT;
    double acc = 0.0;
    if (i0 < na && j0 < nb && !(tri && bj < bi)) {   // (uniform over the workgroup)
        // staging map: element e = tid + 256 s of a 64 x 32 tile is (row e / 32, column e % 32): a wave reads two rows' 128 contiguous bytes
        const int sr = tid >> 5, sk = tid & 31;
        float ia[8], ib[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int ra = i0 + sr + 8 * s, rb = j0 + sr + 8 * s;
            ia[s] = ra < na ? invA[ra] : 0.f;
            ib[s] = rb < nb ? invB[rb] : 0.f;
        }
        const int ty = tid >> 4, tx = tid & 15;
        float d2[4][4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) d2[p][q] = 0.f;
        for (int k0 = 0; k0 < d; k0 += KT) {
            const bool kin = k0 + sk < d;
#pragma unroll
            for (int s = 0; s < 8; ++s) {   // rows past the set and columns past d are staged as 0: their differences add +0 to a sum
                const int ra = i0 + sr + 8 * s, rb = j0 + sr + 8 * s;
                sa[(sr + 8 * s) * KROW + sk] = (kin && ra < na) ? A[(size_t)ra * d + k0 + sk] * ia[s] : 0.f;
                sb[(sr + 8 * s) * KROW + sk] = (kin && rb < nb) ? B[(size_t)rb * d + k0 + sk] * ib[s] : 0.f;
            }
            __syncthreads();
#pragma unroll 2
            for (int kk = 0; kk < KT; kk += 4) {
                f32x4_t u[4], v[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) u[p] = *reinterpret_cast<const f32x4_t*>(sa + (ty + 16 * p) * KROW + kk);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const f32x4_t*>(sb + (tx + 16 * q) * KROW + kk);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float df = u[p][e] - v[q][e];
                            d2[p][q] = fmaf(df, df, d2[p][q]);
                        }
            }
            __syncthreads();
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
                if (i < na && j < nb && (!tri || i < j)) acc += (double)(-expm1f(-(gamma * d2[p][q])));
            }
    }
    const double s = block_sum_f64(acc, red);
    if (tid == 0) part[((size_t)z * gridDim.y + bi) * gridDim.x + bj] = s;
}

// grid (3), one workgroup per sum: thread t adds the partials t, t + 256, ... in that order, then block_sum_f64
__global__ __launch_bounds__(PC_THREADS) void embed_mmd_fold_kernel(const double* __restrict__ part, double* __restrict__ out, int count) {
    __shared__ double red[PC_THREADS / 64];
    double s = 0.0;
    for (int t = threadIdx.x; t < count; t += PC_THREADS) s += part[(size_t)blockIdx.x * count + t];
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__host__ inline long long mmd_tiles(int m, int n) { return ((long long)(m > n ? m : n) + MT - 1) / MT; }
__host__ inline bool mmd_shape_ok(int m, int n, int d) {
    return m >= 1 && n >= 1 && d >= 1 && m <= VK_EMBED_MAX_ROWS && n <= VK_EMBED_MAX_ROWS && d <= VK_EMBED_MAX_DIM;
}

}  // namespace

extern "C" int vk_clip_preprocess_patches_u8(const void* img, void* out, int32_t n_img, int32_t H, int32_t W, int32_t out_hw, int32_t patch,
                                             int32_t ldo, float sigma_y, float sigma_x, int32_t ks_y, int32_t ks_x, const float* mean3,
                                             const float* std3, void* stream) {
    if (!img || !out || !mean3 || !std3 || n_img <= 0 || H < 2 || W < 2 || out_hw <= 0 || patch <= 0 || (out_hw % patch) != 0 ||
        ldo < 3 * patch * patch || ks_y < 1 || ks_x < 1 || ks_y > CLIP_MAX_KS || ks_x > CLIP_MAX_KS || !(ks_y & 1) || !(ks_x & 1) || !(sigma_y > 0.f) || !(sigma_x > 0.f))
        return VK_EINVAL;
    if (n_img > 65535 || out_hw > 4096 || H > VK_CLIP_U8_MAX_SIDE || W > VK_CLIP_U8_MAX_SIDE) return VK_EINVAL;   // (grid.y; tiles^2 in grid.x; 3 W as an int)
    if (ks_y / 2 >= H || ks_x / 2 >= W) return VK_EINVAL;   // (a reflected tap must land inside the frame)
    if (!aligned_to(out, 2)) return VK_EINVAL;
    const bool wide = (W % 4) == 0 && aligned_to(img, 4);
    // the largest tile whose source rectangle fits the LDS; a single output's (4 + 62)^2 pixels of three channels always do
    int tile = 16, rows_max = 0, cols_max = 0;
    for (;; tile >>= 1) {
        tile_extent(H, out_hw, ks_y, tile, &rows_max);
        tile_extent(W, out_hw, ks_x, tile, &cols_max);
        if (3LL * rows_max * cols_max <= CLIP_U8_LDS_FLOATS) break;
        if (tile == 1) return VK_EINVAL;
    }
    const int tiles = (out_hw + tile - 1) / tile;
    const dim3 grid((unsigned)(tiles * tiles), (unsigned)n_img);
    const size_t lds = (size_t)3 * rows_max * cols_max * sizeof(float);
    // the caller zero-fills `out` once (class-token rows and the K padding); this launch writes the 3*patch*patch image columns
    if (wide)
        hipLaunchKernelGGL(clip_preprocess_u8_kernel<true>, grid, dim3(PC_THREADS), lds, (hipStream_t)stream, (const uint8_t*)img, (uint16_t*)out, H, W,
                           out_hw, patch, ldo, sigma_y, sigma_x, ks_y, ks_x, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], tile, rows_max,
                           cols_max);
    else
        hipLaunchKernelGGL(clip_preprocess_u8_kernel<false>, grid, dim3(PC_THREADS), lds, (hipStream_t)stream, (const uint8_t*)img, (uint16_t*)out, H, W,
                           out_hw, patch, ldo, sigma_y, sigma_x, ks_y, ks_x, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], tile, rows_max,
                           cols_max);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_embed_row_stats(const float* a, const float* b, double* out, int32_t n, int32_t d, void* stream) {
    if (!a || !b || !out || n <= 0 || d <= 0 || n > VK_EMBED_MAX_ROWS || d > VK_EMBED_MAX_DIM) return VK_EINVAL;
    if (!aligned_to(a, 4) || !aligned_to(b, 4) || !aligned_to(out, 8)) return VK_EINVAL;
    hipLaunchKernelGGL(embed_row_stats_kernel, dim3((unsigned)n), dim3(PC_THREADS), 0, (hipStream_t)stream, a, b, out, d);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_embed_mmd_ws_bytes(int32_t m, int32_t n, int32_t d) {
    if (!mmd_shape_ok(m, n, d)) return VK_EINVAL;
    const long long t = mmd_tiles(m, n);
    const long long bytes = 3 * t * t * 8 + (((long long)m + n) * 4 + 7) / 8 * 8;   // [3][T][T] fp64 partials, then m + n fp32 inverse norms
    return bytes > 0x7fffffffLL ? VK_EINVAL : (int)bytes;
}

extern "C" int vk_embed_mmd_sums(const float* x, const float* y, double* out3, void* ws, int32_t m, int32_t n, int32_t d, float sigma,
                                 void* stream) {
    if (!x || !y || !out3 || !ws || vk_embed_mmd_ws_bytes(m, n, d) < 0 || !(sigma > 0.f) || !(sigma < INFINITY)) return VK_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(out3, 8) || !aligned_to(ws, 8)) return VK_EINVAL;
    const long long t = mmd_tiles(m, n);
    double* part = (double*)ws;
    float* inv = (float*)(part + 3 * t * t);
    const float gamma = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
    hipLaunchKernelGGL(embed_inv_norm_kernel, dim3((unsigned)(m + n)), dim3(PC_THREADS), 0, (hipStream_t)stream, x, y, inv, m, d);
    VK_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_mmd_tile_kernel, dim3((unsigned)t, (unsigned)t, 3), dim3(PC_THREADS), 0, (hipStream_t)stream, x, y, (const float*)inv,
                       part, m, n, d, gamma);
    VK_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_mmd_fold_kernel, dim3(3), dim3(PC_THREADS), 0, (hipStream_t)stream, (const double*)part, out3, (int)(t * t));
    VK_CHECK_LAUNCH();
    return VK_OK;
}
