// Evaluation front door (gfx950): how close predicted 8-bit frames are to the real ones.
//   vk_frame_fidelity_u8 : two (n, H, W, 3) uint8 stacks -> per frame and channel the exact sum of squared differences (uint64) and the sum of
//                          the SSIM index map (Wang et al. 2004: 11-tap Gaussian window, valid positions only) in fp64, fixed order
// One workgroup owns a VK_FIDELITY_TILE_H x VK_FIDELITY_TILE_W tile of window positions of one frame. It stages the (TILE_H + 10) x (TILE_W + 10)
// halo of both frames into LDS once, as fp32 about the pivot 128 and planar per channel, then per channel runs the horizontal pass of the five
// window quantities (x, y, x^2, y^2, xy) into LDS and the vertical pass from LDS into registers, forms the index and block-reduces in fp64.
// Its partial goes to the caller's workspace; a fold kernel adds a frame's partials in a fixed order. No float atomics, no integer atomics.
// LDS per workgroup: 2 * 3 * 26 * 44 * 4 (halo) + 5 * 26 * 32 * 4 (horizontal pass) + 144 (reduction) = 44,240 bytes.
// No storage-type dependence: the same object code goes into both libraries.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int FD_THREADS = 256;
constexpr int TAPS = VK_FIDELITY_TAPS;                 // 11
constexpr int TH = VK_FIDELITY_TILE_H, TW = VK_FIDELITY_TILE_W;
constexpr int HH = TH + TAPS - 1, HW_ = TW + TAPS - 1;  // halo: 26 rows x 42 pixels
constexpr int HROW = 44;                                // halo row stride in floats: a multiple of 4 (16-byte reads), >= 4 * (TW / 4 - 1) + 16
constexpr int ROW_BYTES = HW_ * 3;                      // 126 bytes of an HWC row belong to a tile's halo
constexpr int ROW_DWORDS = (ROW_BYTES + 3) / 4;         // 32
static_assert(TH == 16 && TW == 32 && FD_THREADS == 256, "the thread maps below are written for 16 x 32 tiles and 256 threads");
static_assert(HROW % 4 == 0 && HROW >= TW + 12, "halo rows are read 16 bytes at a time");

struct Window { float w[TAPS]; };   // reaches the kernel by value in its argument

// The SSIM index of one window from its five weighted moments about the pivot (mx, my: means of x - 128, y - 128; xx, yy, xy: weighted means of
// the pivoted squares and product). Variances and the covariance do not see the pivot; it is added back for the luminance term only.
// Contraction is off for the whole function: mx * mx + my * my must stay two products and an add (as an FMA of one product into the other it
// would no longer equal 2 * (mx * my) when x == y), and xx - mx * mx, yy - my * my, xy - mx * my must round the same way as one another.
// With x == y numerator and denominator are then the same products of the same sums, and the quotient is exactly 1.
__device__ __forceinline__ float ssim_index(float mx, float my, float xx, float yy, float xy) {
#pragma clang fp contract(off)
    const float C1 = 6.5025f, C2 = 58.5225f;   // (0.01 * 255)^2, (0.03 * 255)^2
    const float ux = mx + 128.0f, uy = my + 128.0f;
    const float sxx = xx - mx * mx, syy = yy - my * my, sxy = xy - mx * my;
    const float uxy = ux * uy, uxx = ux * ux, uyy = uy * uy;
    const float num = (2.0f * uxy + C1) * (2.0f * sxy + C2);
    const float den = ((uxx + uyy) + C1) * ((sxx + syy) + C2);
    return num / den;
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // fixed order: lane l takes l + 32, then + 16, ...
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// one byte pair of the halo: pivot, store planar, and add the squared difference where this tile owns the pixel
__device__ __forceinline__ void stage_byte(float* sa, float* sb, int r, int j, uint32_t av, uint32_t bv, bool own, uint32_t* sse) {
    const int col = j / 3, ch = j - col * 3;
    sa[(ch * HH + r) * HROW + col] = (float)((int)av - 128);
    sb[(ch * HH + r) * HROW + col] = (float)((int)bv - 128);
    const int d = (int)av - (int)bv;
    const uint32_t dd = own ? (uint32_t)(d * d) : 0u;
    sse[0] += ch == 0 ? dd : 0u;
    sse[1] += ch == 1 ? dd : 0u;
    sse[2] += ch == 2 ? dd : 0u;
}

// grid (tiles_y * tiles_x, n). Which tile owns which window positions, and which pixels' squared differences, is a function of (H, W) alone.
// WIDE (W % 4 == 0, both stacks 4-byte aligned): every row of every frame starts on a 4-byte boundary and is a whole number of dwords long, a
// tile's first byte (3 * 32 * tx into the row) too, so the halo is loaded a dword per lane and no dword reaches past its row. Any other W: a
// byte per lane.
template <bool WIDE>
__global__ __launch_bounds__(FD_THREADS) void fidelity_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                   double* __restrict__ ssim_part, unsigned long long* __restrict__ sse_part,
                                                                   Window win, int H, int W, int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float sa[3 * HH * HROW];
    __shared__ __attribute__((aligned(16))) float sb[3 * HH * HROW];
    __shared__ __attribute__((aligned(16))) float hq[5 * HH * TW];
    __shared__ double red_f[3][FD_THREADS / 64];
    __shared__ uint32_t red_u[3][FD_THREADS / 64];
    const int tid = threadIdx.x;
    const int nt = tiles_x * tiles_y;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;   // the last tile of an axis owns the pixels up to the frame's edge
    const size_t row_bytes = (size_t)W * 3;
    const size_t frame_off = (size_t)blockIdx.y * H * row_bytes;
    const uint8_t* fa = a + frame_off;
    const uint8_t* fb = b + frame_off;

    // ---- stage the halo of both frames, add this tile's share of the squared differences ----
    uint32_t sse[3] = {0u, 0u, 0u};   // (at most 26 * 42 pixels of 255^2 per tile and channel: 32 bits hold it)
    if (WIDE) {
        for (int i = tid; i < HH * ROW_DWORDS; i += FD_THREADS) {
            const int r = i / ROW_DWORDS, d = i - r * ROW_DWORDS;
            const int gy = y0 + r;
            const size_t off = (size_t)x0 * 3 + (size_t)d * 4;   // (multiples of 4; off < row_bytes implies off + 4 <= row_bytes)
            const bool in = gy < H && off < row_bytes;
            uint32_t va = 0x80808080u, vb = 0x80808080u;          // (outside the frame: the pivot, never part of a valid window)
            if (in) {
                va = *reinterpret_cast<const uint32_t*>(fa + (size_t)gy * row_bytes + off);
                vb = *reinterpret_cast<const uint32_t*>(fb + (size_t)gy * row_bytes + off);
            }
            const bool own_row = in && (r < TH || last_y);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = d * 4 + k;
                if (j < ROW_BYTES) stage_byte(sa, sb, r, j, (va >> (8 * k)) & 0xffu, (vb >> (8 * k)) & 0xffu, own_row && (j < TW * 3 || last_x), sse);
            }
        }
    } else {
        for (int i = tid; i < HH * ROW_BYTES; i += FD_THREADS) {
            const int r = i / ROW_BYTES, j = i - r * ROW_BYTES;
            const int gy = y0 + r;
            const size_t off = (size_t)x0 * 3 + j;
            const bool in = gy < H && off < row_bytes;
            uint32_t va = 128u, vb = 128u;
            if (in) {
                va = fa[(size_t)gy * row_bytes + off];
                vb = fb[(size_t)gy * row_bytes + off];
            }
            stage_byte(sa, sb, r, j, va, vb, in && (r < TH || last_y) && (j < TW * 3 || last_x), sse);
        }
    }
    __syncthreads();

    const int px = tid & (TW - 1), pg = tid >> 5;     // vertical pass: column px, window rows 2 * pg and 2 * pg + 1
    const bool col_ok = x0 + px < W - (TAPS - 1);
    const bool ok0 = col_ok && y0 + 2 * pg < H - (TAPS - 1), ok1 = col_ok && y0 + 2 * pg + 1 < H - (TAPS - 1);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c) {
        // ---- horizontal pass: thread (r, g) forms the five quantities at columns 4g .. 4g + 3 of halo row r from 14 pixels of each frame ----
        if (tid < HH * (TW / 4)) {
            const int r = tid >> 3, g = tid & 7;
            float xa[16], xb[16];
            const f32x4_t* pa = reinterpret_cast<const f32x4_t*>(sa + (c * HH + r) * HROW + 4 * g);
            const f32x4_t* pb = reinterpret_cast<const f32x4_t*>(sb + (c * HH + r) * HROW + 4 * g);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4_t qa = pa[m], qb = pb[m];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xa[4 * m + e] = qa[e];
                    xb[4 * m + e] = qb[e];
                }
            }
            f32x4_t o[5];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) {
                    const float x = xa[e + k], y = xb[e + k], w = win.w[k];
                    s0 = fmaf(w, x, s0);
                    s1 = fmaf(w, y, s1);
                    s2 = fmaf(w, x * x, s2);   // (|x|, |y| <= 128: the squares and the product are exact in fp32)
                    s3 = fmaf(w, y * y, s3);
                    s4 = fmaf(w, x * y, s4);
                }
                o[0][e] = s0; o[1][e] = s1; o[2][e] = s2; o[3][e] = s3; o[4][e] = s4;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) *reinterpret_cast<f32x4_t*>(hq + (q * HH + r) * TW + 4 * g) = o[q];
        }
        __syncthreads();
        // ---- vertical pass: two window positions per thread from 12 rows of each quantity ----
        float m0[5], m1[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float v[TAPS + 1];
#pragma unroll
            for (int k = 0; k <= TAPS; ++k) v[k] = hq[(q * HH + 2 * pg + k) * TW + px];
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                s0 = fmaf(win.w[k], v[k], s0);
                s1 = fmaf(win.w[k], v[k + 1], s1);
            }
            m0[q] = s0;
            m1[q] = s1;
        }
        if (ok0) acc[c] += (double)ssim_index(m0[0], m0[1], m0[2], m0[3], m0[4]);
        if (ok1) acc[c] += (double)ssim_index(m1[0], m1[1], m1[2], m1[3], m1[4]);
        __syncthreads();   // (hq is overwritten by the next channel)
    }

    // ---- block reduction in a fixed order: lanes by shuffle, then the four waves in wave order ----
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double f = wave_sum_f64(acc[c]);
        const uint32_t u = wave_sum_u32(sse[c]);
        if (lane == 0) {
            red_f[c][wave] = f;
            red_u[c][wave] = u;
        }
    }
    __syncthreads();
    if (tid < 3) {
        double f = 0.0;
        unsigned long long u = 0ull;
        for (int w = 0; w < FD_THREADS / 64; ++w) {
            f += red_f[tid][w];
            u += red_u[tid][w];
        }
        const size_t at = ((size_t)blockIdx.y * nt + tile) * 3 + tid;
        ssim_part[at] = f;
        sse_part[at] = u;
    }
}

// grid (3, n), one wave per (frame, channel): lane l adds the tiles l, l + 64, ... in that order, the lanes are added by the fixed shuffle tree
__global__ __launch_bounds__(64) void fidelity_fold_kernel(const double* __restrict__ ssim_part, const unsigned long long* __restrict__ sse_part,
                                                           double* __restrict__ ssim_sum, unsigned long long* __restrict__ sse, int nt) {
    const int c = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    double s = 0.0;
    unsigned long long u = 0ull;
    for (int t = lane; t < nt; t += 64) {
        const size_t at = ((size_t)f * nt + t) * 3 + c;
        s += ssim_part[at];
        u += sse_part[at];
    }
    s = wave_sum_f64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u += __shfl_down(u, o, 64);
    if (lane == 0) {
        ssim_sum[(size_t)f * 3 + c] = s;
        sse[(size_t)f * 3 + c] = u;
    }
}

__host__ inline long long fd_tiles(int H, int W, int* tiles_x, int* tiles_y) {
    *tiles_x = (W - (TAPS - 1) + TW - 1) / TW;
    *tiles_y = (H - (TAPS - 1) + TH - 1) / TH;
    return (long long)*tiles_x * *tiles_y;
}

}  // namespace

extern "C" int vk_frame_fidelity_ws_bytes(int32_t H, int32_t W) {
    if (H < TAPS || W < TAPS) return VK_EINVAL;
    int tiles_x, tiles_y;
    const long long bytes = fd_tiles(H, W, &tiles_x, &tiles_y) * 3 * 16;
    return bytes > 0x7fffffffLL ? VK_EINVAL : (int)bytes;
}

extern "C" int vk_frame_fidelity_u8(const void* a, const void* b, uint64_t* sse, double* ssim_sum, void* ws, const float* window11, int32_t n,
                                    int32_t H, int32_t W, void* stream) {
    if (!a || !b || !sse || !ssim_sum || !ws || !window11 || n <= 0 || H < TAPS || W < TAPS) return VK_EINVAL;
    if (n > 65535) return VK_EINVAL;   // (grid.y)
    if ((((size_t)ws) & 7) != 0 || (((size_t)sse) & 7) != 0 || (((size_t)ssim_sum) & 7) != 0) return VK_EINVAL;
    int tiles_x, tiles_y;
    const long long nt = fd_tiles(H, W, &tiles_x, &tiles_y);
    if (nt * 48 > 0x7fffffffLL) return VK_EINVAL;   // (what vk_frame_fidelity_ws_bytes can state; also bounds grid.x)
    // dword loads only where every row of both stacks starts on a 4-byte boundary; a shape's path is a function of (H, W) alone
    const bool wide = (W % 4) == 0;
    if (wide && (((size_t)a | (size_t)b) & 3) != 0) return VK_EINVAL;
    Window win;
    for (int k = 0; k < TAPS; ++k) win.w[k] = window11[k];
    double* ssim_part = (double*)ws;                                                     // [n][nt][3] fp64
    unsigned long long* sse_part = (unsigned long long*)ws + (size_t)n * nt * 3;         // [n][nt][3] uint64
    const dim3 grid((unsigned)nt, (unsigned)n);
    if (wide)
        hipLaunchKernelGGL(fidelity_tile_kernel<true>, grid, dim3(FD_THREADS), 0, (hipStream_t)stream, (const uint8_t*)a, (const uint8_t*)b,
                           ssim_part, sse_part, win, H, W, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL(fidelity_tile_kernel<false>, grid, dim3(FD_THREADS), 0, (hipStream_t)stream, (const uint8_t*)a, (const uint8_t*)b,
                           ssim_part, sse_part, win, H, W, tiles_x, tiles_y);
    VK_CHECK_LAUNCH();
    hipLaunchKernelGGL(fidelity_fold_kernel, dim3(3, n), dim3(64), 0, (hipStream_t)stream, (const double*)ssim_part,
                       (const unsigned long long*)sse_part, ssim_sum, (unsigned long long*)sse, (int)nt);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
