// Motion scores of the evaluation front door (gfx950): hierarchical block matching on 8-bit luma. Integer arithmetic from end to end, so the
// result is held to a plain numpy restatement bit for bit (tests/_motion_ref.py). The definition is in include/vista_hip.h.
//   vk_flow_luma_pyramid_u8 : (n, H, W, 3) uint8 -> three luma levels per frame (level l + 1 the rounded 2 x 2 mean of level l)
//   vk_block_flow_u8        : the pyramids -> per pair of consecutive frames and 8 x 8 block of level 0 its vector, its SAD and its SAD at zero
//   vk_flow_pair_sums       : the int64 sums over a pair's blocks behind every score
// vk_block_flow_u8 runs one workgroup per (pair, 8 x 8 block of level 2) for the whole descent: that block, its 4 children at level 1 and its
// 16 grandchildren at level 0. A child's vector is twice its parent's plus an increment of at most 2, so every level-0 descendant's vector lies
// within 6 of four times the coarse vector, and ONE window of frame i + 1 per level serves all 1 + 4 + 16 blocks: 22 x 22 bytes at level 2 (the
// block widened by the search range 7), 20 x 20 at level 1 (16 + 2 * 2, displaced by twice the coarse vector), 44 x 44 at level 0 (32 + 2 * 6,
// displaced by four times it). Coordinates are clamped to the image where a window is staged, never in the search loops. A candidate is one
// lane: per row of its block it reads the three dwords that cover its eight window bytes, byte-aligns them in registers (v_alignbyte_b32) and
// adds the row's absolute differences four bytes per instruction (v_sad_u8). The smallest (SAD, |dy| + |dx|, dy, dx) is the minimum of one
// packed 32-bit key, so the order of evaluation cannot matter.
// LDS per workgroup: 1024 + 256 + 64 (the blocks of frame i) + 22 * 24 + 20 * 24 + 44 * 48 (the windows, rows padded to whole dwords past the
// last unaligned read) + 96 (the keys of the reductions, the SADs at zero) = 4,560 bytes: the LDS never limits occupancy, the 256 threads do.
// No storage-type dependence: the same object code goes into both libraries.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int FL_THREADS = 256;
constexpr int BLK = VK_FLOW_BLOCK;              // 8
constexpr int R2 = VK_FLOW_COARSE_RANGE;        // 7
constexpr int R1 = VK_FLOW_REFINE_RANGE;        // 2
constexpr int REACH = 2 * R1 + R1;              // 6: how far a level-0 vector can lie from four times the coarse vector
constexpr int W2 = BLK + 2 * R2, S2 = 24;       // window side and row stride in bytes, level 2
constexpr int W1 = 2 * BLK + 2 * R1, S1 = 24;   // level 1
constexpr int W0 = 4 * BLK + 2 * REACH, S0 = 48;   // level 0
static_assert(VK_FLOW_LEVELS == 3 && BLK == 8 && R2 == 7 && R1 == 2, "the thread maps and the key below are written for these");
static_assert(S2 % 4 == 0 && S2 >= ((2 * R2) & ~3) + 12 && S1 % 4 == 0 && S1 >= ((BLK + 2 * R1) & ~3) + 12 && S0 % 4 == 0 &&
              S0 >= ((3 * BLK + 2 * REACH) & ~3) + 12, "a candidate reads three dwords from the aligned start of its eight bytes");
static_assert((2 * R2 + 1) * (2 * R2 + 1) <= FL_THREADS && (2 * R1 + 1) * (2 * R1 + 1) <= 32, "one candidate per lane");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int absi(int v) { return v < 0 ? -v : v; }

// (SAD, |dy| + |dx|, dy, dx) in one word whose order is the lexicographic one: SAD <= 16320 < 2^14, the rest four bits each (r <= 7)
__device__ __forceinline__ uint32_t make_key(uint32_t sad, int dy, int dx, int r) {
    return (sad << 12) | ((uint32_t)(absi(dy) + absi(dx)) << 8) | ((uint32_t)(dy + r) << 4) | (uint32_t)(dx + r);
}
__device__ __forceinline__ int key_dy(uint32_t k, int r) { return (int)((k >> 4) & 15u) - r; }
__device__ __forceinline__ int key_dx(uint32_t k, int r) { return (int)(k & 15u) - r; }

// The SAD of the 8 x 8 block at `cur` (rows cs bytes apart, 4-byte aligned) against the window bytes at (row, col) of `win` (rows ws apart)
__device__ __forceinline__ uint32_t block_sad(const uint8_t* cur, int cs, const uint8_t* win, int ws, int row, int col) {
    const uint32_t sh = (uint32_t)col & 3u;
    const uint8_t* w = win + row * ws + (col & ~3);
    uint32_t sad = 0;
#pragma unroll
    for (int r = 0; r < BLK; ++r) {
        const uint32_t* wd = reinterpret_cast<const uint32_t*>(w + r * ws);
        const uint32_t* cd = reinterpret_cast<const uint32_t*>(cur + r * cs);
        const uint32_t a = wd[0], b = wd[1], c = wd[2];
        sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(b, a, sh), cd[0], sad);
        sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(c, b, sh), cd[1], sad);
    }
    return sad;
}

// side x side bytes of one level of a frame, from (y0, x0), coordinates clamped to the level (edge replicate), into dst (rows stride apart)
__device__ __forceinline__ void stage_window(uint8_t* dst, int stride, int side, const uint8_t* __restrict__ src, int y0, int x0, int Hl, int Wl,
                                             int tid) {
    for (int i = tid; i < side * side; i += FL_THREADS) {
        const int r = i / side, c = i - r * side;
        dst[r * stride + c] = src[(size_t)clampi(y0 + r, Hl - 1) * Wl + clampi(x0 + c, Wl - 1)];
    }
}

// 4 x 4 pixels of level 0 per thread: 16 luma bytes, the 2 x 2 of level 1 and the one byte of level 2 they decide. grid (patches / 256, n).
__global__ __launch_bounds__(FL_THREADS) void flow_pyramid_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ l0,
                                                                  uint8_t* __restrict__ l1, uint8_t* __restrict__ l2, int H, int W) {
    const int pw = W >> 2, ph = H >> 2;
    const int idx = blockIdx.x * FL_THREADS + threadIdx.x;
    if (idx >= pw * ph) return;
    const int py = idx / pw, px = idx - py * pw;
    const size_t f = blockIdx.y;
    const uint8_t* src = frames + f * (size_t)H * W * 3;
    uint32_t y[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(src + ((size_t)(4 * py + r) * W + 4 * px) * 3);   // (12 bytes, 4-byte aligned)
        const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t ch[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int j = 3 * k + c;
                ch[c] = (d[j >> 2] >> (8 * (j & 3))) & 0xffu;
            }
            y[r][k] = (77u * ch[0] + 150u * ch[1] + 29u * ch[2] + 128u) >> 8;
        }
        *reinterpret_cast<uint32_t*>(l0 + (f * H + 4 * py + r) * (size_t)W + 4 * px) = y[r][0] | (y[r][1] << 8) | (y[r][2] << 16) | (y[r][3] << 24);
    }
    uint32_t m[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) m[r][k] = (y[2 * r][2 * k] + y[2 * r][2 * k + 1] + y[2 * r + 1][2 * k] + y[2 * r + 1][2 * k + 1] + 2u) >> 2;
    const int W1l = W >> 1, H1l = H >> 1;
#pragma unroll
    for (int r = 0; r < 2; ++r)
        *reinterpret_cast<uint16_t*>(l1 + (f * H1l + 2 * py + r) * (size_t)W1l + 2 * px) = (uint16_t)(m[r][0] | (m[r][1] << 8));
    l2[(f * ph + py) * (size_t)pw + px] = (uint8_t)((m[0][0] + m[0][1] + m[1][0] + m[1][1] + 2u) >> 2);
}

// grid ((H / 32) * (W / 32), n - 1): the descent of one level-2 block of the pair (blockIdx.y, blockIdx.y + 1)
__global__ __launch_bounds__(FL_THREADS) void block_flow_kernel(const uint8_t* __restrict__ l0, const uint8_t* __restrict__ l1,
                                                                const uint8_t* __restrict__ l2, int16_t* __restrict__ flow,
                                                                uint16_t* __restrict__ sad_out, int H, int W) {
    __shared__ __attribute__((aligned(16))) uint8_t cur0[4 * BLK * 4 * BLK];
    __shared__ __attribute__((aligned(16))) uint8_t cur1[2 * BLK * 2 * BLK];
    __shared__ __attribute__((aligned(16))) uint8_t cur2[BLK * BLK];
    __shared__ __attribute__((aligned(16))) uint8_t win2[W2 * S2];
    __shared__ __attribute__((aligned(16))) uint8_t win1[W1 * S1];
    __shared__ __attribute__((aligned(16))) uint8_t win0[W0 * S0];
    __shared__ uint32_t red[FL_THREADS / 64];
    __shared__ uint32_t key1[4];
    __shared__ uint32_t zero_sad[16];
    const int tid = threadIdx.x;
    const int gx = W >> 5, Bx = blockIdx.x % gx, By = blockIdx.x / gx;
    const size_t pair = blockIdx.y;
    const int H1l = H >> 1, W1l = W >> 1, H2l = H >> 2, W2l = W >> 2;
    const uint8_t* c0 = l0 + pair * (size_t)H * W;
    const uint8_t* c1 = l1 + pair * (size_t)H1l * W1l;
    const uint8_t* c2 = l2 + pair * (size_t)H2l * W2l;
    const uint8_t* n0 = c0 + (size_t)H * W;
    const uint8_t* n1 = c1 + (size_t)H1l * W1l;
    const uint8_t* n2 = c2 + (size_t)H2l * W2l;

    // ---- frame i: the 32 x 32, 16 x 16 and 8 x 8 bytes of the three levels (inside the image: no clamp), a dword per lane ----
    {
        const int r = tid >> 3, d = tid & 7;   // 32 rows x 8 dwords
        reinterpret_cast<uint32_t*>(cur0)[tid] = *reinterpret_cast<const uint32_t*>(c0 + (size_t)(32 * By + r) * W + 32 * Bx + 4 * d);
        if (tid < 64) {                        // 16 rows x 4 dwords
            const int r1 = tid >> 2, d1 = tid & 3;
            reinterpret_cast<uint32_t*>(cur1)[tid] = *reinterpret_cast<const uint32_t*>(c1 + (size_t)(16 * By + r1) * W1l + 16 * Bx + 4 * d1);
        } else if (tid < 80) {                 // 8 rows x 2 dwords
            const int t = tid - 64, r2 = t >> 1, d2 = t & 1;
            reinterpret_cast<uint32_t*>(cur2)[t] = *reinterpret_cast<const uint32_t*>(c2 + (size_t)(8 * By + r2) * W2l + 8 * Bx + 4 * d2);
        }
    }
    stage_window(win2, S2, W2, n2, 8 * By - R2, 8 * Bx - R2, H2l, W2l, tid);
    __syncthreads();

    // ---- the SAD at zero displacement of the 16 level-0 blocks: 16 lanes a block, a dword of frame i + 1 each ----
    {
        const int b = tid >> 4, j = tid & 15, by = b >> 2, bx = b & 3, r = j >> 1, d = j & 1;
        const uint32_t mine = *reinterpret_cast<const uint32_t*>(cur0 + (8 * by + r) * 32 + 8 * bx + 4 * d);
        const uint32_t next = *reinterpret_cast<const uint32_t*>(n0 + (size_t)(32 * By + 8 * by + r) * W + 32 * Bx + 8 * bx + 4 * d);
        uint32_t s = __builtin_amdgcn_sad_u8(mine, next, 0u);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (j == 0) zero_sad[b] = s;
    }

    // ---- level 2: the 225 vectors of [-7, 7]^2, one per lane ----
    uint32_t key = 0xffffffffu;
    if (tid < (2 * R2 + 1) * (2 * R2 + 1)) {
        const int iy = tid / (2 * R2 + 1), ix = tid - iy * (2 * R2 + 1);
        key = make_key(block_sad(cur2, BLK, win2, S2, iy, ix), iy - R2, ix - R2, R2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor(key, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    key = min(min(red[0], red[1]), min(red[2], red[3]));
    const int v2y = key_dy(key, R2), v2x = key_dx(key, R2);

    // ---- level 1: four blocks, 25 increments each around twice the coarse vector; a block is half a wave ----
    stage_window(win1, S1, W1, n1, 16 * By + 2 * v2y - R1, 16 * Bx + 2 * v2x - R1, H1l, W1l, tid);
    stage_window(win0, S0, W0, n0, 32 * By + 4 * v2y - REACH, 32 * Bx + 4 * v2x - REACH, H, W, tid);
    __syncthreads();
    const int cand = tid & 31, iy = cand / (2 * R1 + 1), ix = cand - iy * (2 * R1 + 1);   // (cand < 25: iy, ix in 0 .. 4)
    const bool live = cand < (2 * R1 + 1) * (2 * R1 + 1);
    key = 0xffffffffu;
    if (tid < 128 && live) {
        const int b = tid >> 5, by = b >> 1, bx = b & 1;
        key = make_key(block_sad(cur1 + (8 * by) * 16 + 8 * bx, 16, win1, S1, 8 * by + iy, 8 * bx + ix), iy - R1, ix - R1, R1);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor(key, o, 64));
    if (tid < 128 && cand == 0) key1[tid >> 5] = key;
    __syncthreads();

    // ---- level 0: sixteen blocks around twice their parent's vector, eight at a time ----
    const int bw = W >> 3;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int b = (tid >> 5) + 8 * it, by = b >> 2, bx = b & 3;
        const uint32_t pk = key1[(by >> 1) * 2 + (bx >> 1)];
        const int oy = 2 * key_dy(pk, R1), ox = 2 * key_dx(pk, R1);   // twice the parent's increment: within 4 of four times the coarse vector
        key = 0xffffffffu;
        if (live) key = make_key(block_sad(cur0 + (8 * by) * 32 + 8 * bx, 32, win0, S0, 8 * by + REACH + oy + iy - R1, 8 * bx + REACH + ox + ix - R1),
                                 iy - R1, ix - R1, R1);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor(key, o, 64));
        if (cand == 0) {
            const int vy = 4 * v2y + oy + key_dy(key, R1), vx = 4 * v2x + ox + key_dx(key, R1);
            const size_t at = (pair * (size_t)(H >> 3) + 4 * By + by) * bw + 4 * Bx + bx;
            reinterpret_cast<uint32_t*>(flow)[at] = ((uint32_t)vy & 0xffffu) | ((uint32_t)vx << 16);
            reinterpret_cast<uint32_t*>(sad_out)[at] = (key >> 12) | (zero_sad[b] << 16);
        }
    }
}

// grid (pairs): out[p] = {blocks with a non-zero vector, sum |v|^2, sum SAD, sum SAD at zero, sum |v - v_ref|^2 (0 without ref)}. Exact
// integers, so any order gives them; the order here is fixed all the same (lane strides, the shuffle tree, the waves in wave order).
__global__ __launch_bounds__(FL_THREADS) void flow_sums_kernel(const int16_t* __restrict__ flow, const uint16_t* __restrict__ sad,
                                                               const int16_t* __restrict__ ref, long long* __restrict__ out, int blocks) {
    __shared__ long long part[FL_THREADS / 64][5];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * blocks;
    long long s[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < blocks; i += FL_THREADS) {
        const uint32_t v = reinterpret_cast<const uint32_t*>(flow)[base + i], e = reinterpret_cast<const uint32_t*>(sad)[base + i];
        const int vy = (int16_t)(v & 0xffffu), vx = (int16_t)(v >> 16);
        s[0] += (vy != 0 || vx != 0) ? 1 : 0;
        s[1] += vy * vy + vx * vx;
        s[2] += e & 0xffffu;
        s[3] += e >> 16;
        if (ref) {
            const uint32_t q = reinterpret_cast<const uint32_t*>(ref)[base + i];
            const int dy = vy - (int16_t)(q & 0xffffu), dx = vx - (int16_t)(q >> 16);
            s[4] += dy * dy + dx * dx;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, 64);
        if ((tid & 63) == 0) part[tid >> 6][k] = s[k];
    }
    __syncthreads();
    if (tid < 5) {
        long long t = 0;
        for (int w = 0; w < FL_THREADS / 64; ++w) t += part[w][tid];
        out[(size_t)blockIdx.x * 5 + tid] = t;
    }
}

// Each factor is bounded before it is multiplied: H, W <= VK_FLOW_MAX_SIDE and n <= 65535 keep n * H * W * 21 below 2^53.
__host__ inline bool flow_shape_ok(int n, int H, int W) {
    if (n < 1 || n > VK_FLOW_MAX_FRAMES || H < 32 || W < 32 || H > VK_FLOW_MAX_SIDE || W > VK_FLOW_MAX_SIDE || H % 32 != 0 || W % 32 != 0) return false;
    return (long long)n * H * W * 21 / 16 <= 0x7fffffffLL;
}

}  // namespace

extern "C" int vk_flow_pyramid_bytes(int32_t n, int32_t H, int32_t W) {
    return flow_shape_ok(n, H, W) ? (int)((long long)n * H * W * 21 / 16) : VK_EINVAL;
}

extern "C" int vk_flow_luma_pyramid_u8(const void* frames, void* pyr, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!frames || !pyr || !flow_shape_ok(n, H, W) || !aligned_to(frames, 4) || !aligned_to(pyr, 4)) return VK_EINVAL;
    uint8_t* l0 = (uint8_t*)pyr;
    uint8_t* l1 = l0 + (size_t)n * H * W;
    uint8_t* l2 = l1 + (size_t)n * H * W / 4;
    const unsigned patches = (unsigned)(H / 4) * (unsigned)(W / 4);
    hipLaunchKernelGGL(flow_pyramid_kernel, dim3((patches + FL_THREADS - 1) / FL_THREADS, (unsigned)n), dim3(FL_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)frames, l0, l1, l2, H, W);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_block_flow_u8(const void* pyr, int16_t* flow, uint16_t* sad, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!pyr || !flow || !sad || n < 2 || !flow_shape_ok(n, H, W) || !aligned_to(pyr, 4) || !aligned_to(flow, 4) || !aligned_to(sad, 4))
        return VK_EINVAL;
    const uint8_t* l0 = (const uint8_t*)pyr;
    const uint8_t* l1 = l0 + (size_t)n * H * W;
    const uint8_t* l2 = l1 + (size_t)n * H * W / 4;
    hipLaunchKernelGGL(block_flow_kernel, dim3((unsigned)(H / 32) * (unsigned)(W / 32), (unsigned)(n - 1)), dim3(FL_THREADS), 0,
                       (hipStream_t)stream, l0, l1, l2, flow, sad, H, W);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_flow_pair_sums(const int16_t* flow, const uint16_t* sad, const int16_t* flow_ref, int64_t* out, int32_t pairs, int32_t blocks,
                                 void* stream) {
    if (!flow || !sad || !out || pairs < 1 || blocks < 1 || (long long)pairs * blocks > 0x7fffffffLL) return VK_EINVAL;
    if (!aligned_to(flow, 4) || !aligned_to(sad, 4) || !aligned_to(flow_ref, 4) || !aligned_to(out, 8)) return VK_EINVAL;
    hipLaunchKernelGGL(flow_sums_kernel, dim3((unsigned)pairs), dim3(FL_THREADS), 0, (hipStream_t)stream, flow, sad, flow_ref, (long long*)out,
                       blocks);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
