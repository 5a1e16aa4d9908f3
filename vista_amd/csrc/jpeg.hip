// Motion-JPEG video output (gfx950): a baseline sequential JPEG encoder (ITU-T T.81) for the 8-bit frames the front doors already hold on the GPU.
//   vk_jpeg_dct_quant_u8   : (n, H, W, 3) uint8 -> quantised DCT coefficients, int16, zigzag order, blocks in scan order (4:2:0, 16 x 16 MCUs)
//   vk_jpeg_interval_sizes : the coded bytes of every restart interval (one MCU row), stuffing, padding and RSTm marker included
//   vk_jpeg_entropy_write  : every interval's Huffman-coded bytes at the caller's offset (Annex K "typical" tables)
// uint8 in, int16 and bytes out: no storage-type dependence, the same object code goes into both libraries (as csrc/loss.hip).
//
// Stage A. A workgroup owns JA_TM neighbouring MCUs of one MCU row: 16 pixel rows of up to 128 pixels, 384 bytes per row. An MCU's 48 bytes per
// pixel row are no power of two, so the tile is not cut by MCU on the way in: the 16 row segments are copied to LDS as bytes, 16 per lane where
// 3 W % 16 == 0 and the frames are 16-byte aligned (4 where 3 W % 4 == 0, else 1) -- consecutive lanes on consecutive chunks of a row -- and
// MCUs are cut out of LDS. Edge replication is an index clamp on the LDS read, so the copy never leaves the frame. The 48 blocks of the tile
// then lie block-major in LDS, rows padded to 9 floats: the row pass (a lane per block row) strides 9 dwords, the column pass (a lane per block
// column) 1 dword within a block and 72 between blocks -- both free of bank conflicts. The coefficients leave through LDS as well: a tile's
// blocks are one contiguous run of the output, stored 16 bytes per lane.
//
// Stage B. A workgroup owns one restart interval and walks its blocks 256 at a time, a lane per block. A block's DC predictor is the DC of the
// previous block of its component in scan order (0 at the interval's start): read from the coefficient array, no dependency between lanes.
// Per chunk: bit length per block -> workgroup scan -> every lane ORs its block's bits into a zeroed LDS bit buffer (big-endian words; the
// first and last word of a block may be shared and take an integer atomicOr, the words between are the block's own and take plain stores) ->
// the buffer's whole bytes are counted (0xFF is followed by 0x00), scanned 256 words at a time and stored, every output byte by exactly one
// lane. At most 7 bits are carried from chunk to chunk. A chunk of 256 blocks is at most 256 x 1665 bits = 53280 bytes: it fits LDS whatever the
// content, and the interval (any number of chunks) never has to. Integer ORs only: the bytes do not depend on the order of execution.
#include "common.h"
#include "vista_hip.h"

namespace {

// ---- stage A ----------------------------------------------------------------------------------------------------------------------------------
constexpr int JA_THREADS = 256;
constexpr int JA_TM = 8;                          // MCUs per workgroup
constexpr int JA_PX = JA_TM * 16;                 // pixels per tile row
constexpr int JA_RAW_PITCH = JA_PX * 3 + 16;      // bytes; a multiple of 16
constexpr int JA_BLOCKS = JA_TM * 6;
constexpr int JA_BLK = 72;                        // floats per block: 8 rows of 8 + 1

struct DevQuant { float q[2][64]; };              // [luma, chroma][zigzag index], the divisors as floats

__device__ __constant__ uint8_t JA_ZIGZAG[64] = {   // natural (row-major) index of zigzag position k
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// m[u][x] = C(u) / 2 * cos((2 x + 1) u pi / 16), C(0) = 1 / sqrt(2), else 1: the float64 values rounded to fp32
__device__ __constant__ float JA_DCT[64] = {
    0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f,
    0.49039264020161522f, 0.41573480615127262f, 0.27778511650980114f, 0.09754516100806417f, -0.09754516100806410f, -0.27778511650980098f, -0.41573480615127267f, -0.49039264020161522f,
    0.46193976625564337f, 0.19134171618254492f, -0.19134171618254486f, -0.46193976625564337f, -0.46193976625564342f, -0.19134171618254517f, 0.19134171618254500f, 0.46193976625564326f,
    0.41573480615127262f, -0.09754516100806410f, -0.49039264020161522f, -0.27778511650980109f, 0.27778511650980092f, 0.49039264020161522f, 0.09754516100806439f, -0.41573480615127256f,
    0.35355339059327379f, -0.35355339059327373f, -0.35355339059327384f, 0.35355339059327368f, 0.35355339059327384f, -0.35355339059327334f, -0.35355339059327356f, 0.35355339059327329f,
    0.27778511650980114f, -0.49039264020161522f, 0.09754516100806415f, 0.41573480615127273f, -0.41573480615127256f, -0.09754516100806401f, 0.49039264020161533f, -0.27778511650980076f,
    0.19134171618254492f, -0.46193976625564342f, 0.46193976625564326f, -0.19134171618254495f, -0.19134171618254528f, 0.46193976625564337f, -0.46193976625564320f, 0.19134171618254478f,
    0.09754516100806417f, -0.27778511650980109f, 0.41573480615127273f, -0.49039264020161533f, 0.49039264020161522f, -0.41573480615127251f, 0.27778511650980076f, -0.09754516100806429f};

// one 8-point DCT-II row of T.81 A.3.3's separable form: out[u] = sum_x m[u][x] * in[x], m[u][x] = C(u) / 2 * cos((2 x + 1) u pi / 16)
__device__ __forceinline__ void dct8(const float* __restrict__ m, const float* in, float* out) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float acc = 0.f;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc = fmaf(m[u * 8 + x], in[x], acc);
        out[u] = acc;
    }
}

template <int V>
__global__ __launch_bounds__(JA_THREADS) void jpeg_dct_quant_kernel(const uint8_t* __restrict__ frames, int16_t* __restrict__ coef,
                                                                    const DevQuant dq, int H, int W, int mcu_h, int mcu_w, int tiles_x) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[16 * JA_RAW_PITCH];
    __shared__ float blk[JA_BLOCKS * JA_BLK];
    __shared__ __attribute__((aligned(16))) int16_t q16[JA_BLOCKS * 64];
    __shared__ float mat[64];
    __shared__ float qf[2][64];
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int my = t % mcu_h, f = t / mcu_h;
    const int mx0 = tx * JA_TM, tm = min(JA_TM, mcu_w - mx0);
    const int x0 = mx0 * 16, y0 = my * 16;
    const int cols = min(JA_PX, W - x0), rows = min(16, H - y0);   // the part of the tile that lies inside the frame: both >= 1

    if (tid < 64) {
        mat[tid] = JA_DCT[tid];
        qf[0][tid] = dq.q[0][tid];
        qf[1][tid] = dq.q[1][tid];
    }
    // ---- the tile's bytes, row segment by row segment ----
    {
        const int row_bytes = cols * 3, chunks = row_bytes / V;     // (V > 1 only where 3 W % V == 0: then row_bytes % V == 0 as x0 * 3 % 16 == 0)
        const size_t base = ((size_t)f * H + y0) * ((size_t)W * 3) + (size_t)x0 * 3;
        for (int i = tid; i < rows * chunks; i += JA_THREADS) {
            const int r = i / chunks, c = i - r * chunks;
            const uint8_t* src = frames + base + (size_t)r * ((size_t)W * 3) + (size_t)c * V;
            uint8_t* dst = raw + r * JA_RAW_PITCH + c * V;
            if (V == 16) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
            else if (V == 4) *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
            else *dst = *src;
        }
    }
    __syncthreads();
    // ---- colour conversion, 2 x 2 chroma means, level shift: a lane per 2 x 2 quad ----
    for (int i = tid; i < 8 * 8 * tm; i += JA_THREADS) {
        const int qy = i / (8 * tm), qx = i - qy * (8 * tm);
        float cb = 0.f, cr = 0.f, s_cb[4], s_cr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ly = qy * 2 + (k >> 1), lx = qx * 2 + (k & 1);
            const uint8_t* p = raw + min(ly, rows - 1) * JA_RAW_PITCH + min(lx, cols - 1) * 3;
            const float R = (float)p[0], G = (float)p[1], B = (float)p[2];
            const float Y = 0.299f * R + 0.587f * G + 0.114f * B;
            s_cb[k] = -0.168736f * R - 0.331264f * G + 0.5f * B + 128.f;
            s_cr[k] = 0.5f * R - 0.418688f * G - 0.081312f * B + 128.f;
            const int m = lx >> 4, b = m * 6 + ((ly >> 3) << 1) + ((lx >> 3) & 1);
            blk[b * JA_BLK + (ly & 7) * 9 + (lx & 7)] = Y - 128.f;
        }
        cb = ((s_cb[0] + s_cb[1]) + (s_cb[2] + s_cb[3])) * 0.25f;
        cr = ((s_cr[0] + s_cr[1]) + (s_cr[2] + s_cr[3])) * 0.25f;
        const int m = qx >> 3;
        blk[(m * 6 + 4) * JA_BLK + qy * 9 + (qx & 7)] = cb - 128.f;
        blk[(m * 6 + 5) * JA_BLK + qy * 9 + (qx & 7)] = cr - 128.f;
    }
    __syncthreads();
    // ---- rows, in place: a lane per block row ----
    for (int i = tid; i < 6 * tm * 8; i += JA_THREADS) {
        float* row = blk + (i >> 3) * JA_BLK + (i & 7) * 9;
        float in[8], out[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = row[x];
        dct8(mat, in, out);
#pragma unroll
        for (int x = 0; x < 8; ++x) row[x] = out[x];
    }
    __syncthreads();
    // ---- columns, in place: a lane per block column ----
    for (int i = tid; i < 6 * tm * 8; i += JA_THREADS) {
        const int b = i >> 3, c = i & 7;
        const float* col = blk + b * JA_BLK + c;
        float in[8], out[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = col[y * 9];
        dct8(mat, in, out);
#pragma unroll
        for (int v = 0; v < 8; ++v) blk[b * JA_BLK + v * 9 + c] = out[v];
    }
    __syncthreads();
    // ---- quantiser, rounding half away from zero, clamp, zigzag: a lane per coefficient ----
    for (int i = tid; i < 6 * tm * 64; i += JA_THREADS) {
        const int b = i >> 6, k = i & 63, nat = JA_ZIGZAG[k];
        const float v = blk[b * JA_BLK + (nat >> 3) * 9 + (nat & 7)] / qf[(b % 6) >= 4 ? 1 : 0][k];
        q16[i] = (int16_t)(int)fminf(fmaxf(roundf(v), k == 0 ? -1024.f : -1023.f), 1023.f);
    }
    __syncthreads();
    // ---- out: the tile's blocks are one contiguous run of coef ----
    {
        const size_t first = (((size_t)f * mcu_h + my) * mcu_w + mx0) * 6 * 64;
        uint4* dst = reinterpret_cast<uint4*>(coef + first);
        const uint4* src = reinterpret_cast<const uint4*>(q16);
        for (int i = tid; i < 6 * tm * 8; i += JA_THREADS) dst[i] = src[i];
    }
}

// ---- stage B ----------------------------------------------------------------------------------------------------------------------------------
constexpr int JB_THREADS = 256;
constexpr int JB_MAX_BLOCK_BITS = 27 + 63 * 26;                              // DC: 16-bit code at most + 11; AC: 16 + 10 each
constexpr int JB_WORDS = (JB_THREADS * JB_MAX_BLOCK_BITS + 7 + 31) / 32 + 2;  // a chunk's bits, 7 carried bits, the 1-bit padding

// Annex K tables K.3 - K.6 as BITS (codes per length 1 .. 16) and HUFFVAL.
struct HuffSpec { uint8_t bits[16]; uint8_t n; uint8_t val[162]; };
constexpr HuffSpec SPEC_DC0 = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec SPEC_DC1 = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec SPEC_AC0 = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec SPEC_AC1 = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> (code << 5) | length, generated as T.81 Annex C does (codes of one length count up, a shift between lengths). 0: no such symbol.
struct HuffCodes { uint32_t e[2][2][256]; };       // [luma, chroma][DC, AC][symbol]
constexpr void fill_codes(const HuffSpec& s, uint32_t* e) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) e[s.val[k++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}
constexpr HuffCodes make_codes() {
    HuffCodes h{};
    fill_codes(SPEC_DC0, h.e[0][0]);
    fill_codes(SPEC_AC0, h.e[0][1]);
    fill_codes(SPEC_DC1, h.e[1][0]);
    fill_codes(SPEC_AC1, h.e[1][1]);
    return h;
}
__device__ __constant__ HuffCodes JB_CODES = make_codes();

// The symbols of one block, in order, handed to `emit(bits, nbits)`: Huffman code and appended bits of a coefficient together (at most 26).
template <class Emit>
__device__ __forceinline__ void code_block(const int16_t* __restrict__ blk, int pred, const uint32_t* __restrict__ dc, const uint32_t* __restrict__ ac,
                                           Emit&& emit) {
    const uint4* src = reinterpret_cast<const uint4*>(blk);
    int run = 0;
    for (int j = 0; j < 8; ++j) {
        const uint4 w = src[j];
        const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int v = (int)(int16_t)((d[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
            if (j == 0 && e == 0) {
                const int diff = min(max(v, -1024), 1023) - pred;   // (stage A's ranges: a foreign array is coded as its clamped self, and no
                                                                    // block can outgrow JB_MAX_BLOCK_BITS; pred arrives clamped)
                const int cat = diff == 0 ? 0 : 32 - __builtin_clz((unsigned)(diff < 0 ? -diff : diff));
                const uint32_t en = dc[cat];
                const uint32_t vb = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u);
                emit(((en >> 5) << cat) | vb, (int)(en & 31u) + cat);
            } else if (v == 0) {
                ++run;
            } else {
                while (run >= 16) {
                    const uint32_t z = ac[0xf0];
                    emit(z >> 5, (int)(z & 31u));
                    run -= 16;
                }
                v = min(max(v, -1023), 1023);
                const int cat = 32 - __builtin_clz((unsigned)(v < 0 ? -v : v));
                const uint32_t en = ac[(run << 4) | cat];
                const uint32_t vb = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
                emit(((en >> 5) << cat) | vb, (int)(en & 31u) + cat);
                run = 0;
            }
        }
    }
    if (run > 0) {
        const uint32_t z = ac[0x00];
        emit(z >> 5, (int)(z & 31u));
    }
}

// exclusive scan of v over the workgroup (256 lanes, 4 waves); *total = the sum. Two barriers; `part` is 4 words of LDS.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                   // (part may still be read from the previous scan)
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < JB_THREADS / 64; ++w) {
        const uint32_t p = part[w];
        if (w < wave) before += p;
        sum += p;
    }
    *total = sum;
    return before + inc - v;
}

__device__ __forceinline__ int count_ff(uint32_t w) {
    return (int)((w >> 24) == 0xffu) + (int)(((w >> 16) & 0xffu) == 0xffu) + (int)(((w >> 8) & 0xffu) == 0xffu) + (int)((w & 0xffu) == 0xffu);
}

// One workgroup per restart interval: blockIdx.x = frame * mcu_h + MCU row. WRITE = false: sizes[interval] = its bytes. WRITE = true: the bytes
// go to out + offsets[interval]; a byte at or beyond out_bytes is not stored (offsets that do not come from the sizes cannot leave the buffer).
template <bool WRITE>
__global__ __launch_bounds__(JB_THREADS) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int32_t* __restrict__ sizes,
                                                                  const int64_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                                  long long out_bytes, int mcu_h, int mcu_w) {
    __shared__ uint32_t bits[JB_WORDS];
    __shared__ uint32_t codes[2][2][256];
    __shared__ uint32_t part[JB_THREADS / 64];
    const int tid = threadIdx.x;
    const int interval = blockIdx.x, row = interval % mcu_h;
    const int nb = 6 * mcu_w;
    const int16_t* base = coef + (size_t)interval * nb * 64;
    for (int i = tid; i < 1024; i += JB_THREADS) (&codes[0][0][0])[i] = (&JB_CODES.e[0][0][0])[i];

    long long at = 0;                                  // stuffed bytes of this interval so far
    if (WRITE) at = offsets[interval];
    const long long begin = at;
    uint32_t lead = 0, carry = 0;                      // bits (< 8) carried from the previous chunk, and their byte (high bits)
    for (int c0 = 0; c0 < nb; c0 += JB_THREADS) {
        const int b = c0 + tid;
        const bool have = b < nb;
        const bool last_chunk = c0 + JB_THREADS >= nb;
        const int k = have ? b % 6 : 0;
        const int chroma = k >= 4 ? 1 : 0;
        int pred = 0;
        if (have) {
            // the previous block of the same component: Y01 <- Y00, Y10 <- Y01, Y11 <- Y10 of this MCU; Y00 <- Y11, Cb <- Cb, Cr <- Cr of the last
            const int pb = (k >= 1 && k <= 3) ? b - 1 : (k == 0 ? b - 3 : b - 6);
            if (pb >= 0) pred = min(max((int)base[(size_t)pb * 64], -1024), 1023);
        }
        __syncthreads();                               // codes are in LDS; the previous chunk's buffer has been read
        uint32_t len = 0;
        if (have) code_block(base + (size_t)b * 64, pred, codes[chroma][0], codes[chroma][1], [&](uint32_t, int n) { len += (uint32_t)n; });
        uint32_t total;
        const uint32_t start = lead + block_scan(len, part, &total);
        const uint32_t all_bits = lead + total;
        const uint32_t used_words = (all_bits + 31) / 32 + 1;
        for (uint32_t i = tid; i < used_words; i += JB_THREADS) bits[i] = i == 0 ? carry << 24 : 0u;
        __syncthreads();
        if (have) {
            uint32_t w = start >> 5;
            int cnt = (int)(start & 31u);
            uint64_t acc = 0;
            bool first = true;
            code_block(base + (size_t)b * 64, pred, codes[chroma][0], codes[chroma][1], [&](uint32_t v, int n) {
                acc = (acc << n) | v;
                cnt += n;
                if (cnt >= 32) {
                    const uint32_t word = (uint32_t)(acc >> (cnt - 32));
                    if (first) atomicOr(&bits[w], word);
                    else bits[w] = word;
                    first = false;
                    ++w;
                    cnt -= 32;
                    acc &= (1ull << cnt) - 1ull;
                }
            });
            if (cnt > 0) atomicOr(&bits[w], (uint32_t)(acc << (32 - cnt)));
        }
        __syncthreads();
        // ---- the chunk's whole bytes (the last chunk: its partial byte too, padded with 1-bits) ----
        uint32_t nbytes = all_bits >> 3;
        const uint32_t rem = all_bits & 7u;
        if (last_chunk && rem) {
            if (tid == 0) atomicOr(&bits[nbytes >> 2], (0xffu >> rem) << (24 - 8 * (nbytes & 3u)));
            ++nbytes;
            __syncthreads();
        }
        for (uint32_t w0 = 0; w0 * 4 < nbytes; w0 += JB_THREADS) {
            const uint32_t wi = w0 + tid;
            const int nby = wi * 4 < nbytes ? (int)min(4u, nbytes - wi * 4) : 0;
            uint32_t word = nby ? bits[wi] : 0u;
            if (nby < 4) word &= ~(0xffffffffu >> (8 * nby));        // bytes past the end are not 0xFF
            uint32_t round_total;
            const uint32_t ff_before = block_scan((uint32_t)count_ff(word), part, &round_total);
            if (WRITE) {
                long long p = at + (long long)wi * 4 - (long long)w0 * 4 + ff_before;
                for (int j = 0; j < nby; ++j) {
                    const uint32_t byte = (word >> (24 - 8 * j)) & 0xffu;
                    if (p >= 0 && p < out_bytes) out[p] = (uint8_t)byte;
                    ++p;
                    if (byte == 0xffu) {
                        if (p >= 0 && p < out_bytes) out[p] = 0;
                        ++p;
                    }
                }
            }
            const uint32_t round_bytes = min((uint32_t)JB_THREADS * 4u, nbytes - w0 * 4);
            at += round_bytes + round_total;
        }
        if (!last_chunk) {
            carry = rem ? (bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3u))) & 0xffu : 0u;
            lead = rem;
        }
    }
    const bool marker = row != mcu_h - 1;              // every interval but a frame's last is followed by RSTm, m = row mod 8
    if (tid == 0) {
        if (WRITE) {
            if (marker) {
                if (at >= 0 && at < out_bytes) out[at] = 0xff;
                if (at + 1 >= 0 && at + 1 < out_bytes) out[at + 1] = (uint8_t)(0xd0 + (row & 7));
            }
        } else {
            sizes[interval] = (int32_t)(at - begin + (marker ? 2 : 0));
        }
    }
}

bool jb_geometry_ok(int32_t n, int32_t mcu_h, int32_t mcu_w, int32_t blocks) {
    if (n <= 0 || mcu_h <= 0 || mcu_w <= 0 || mcu_h > 4096 || mcu_w > 4096) return false;   // (4096 MCUs = 65536 pixels: the last size 65535 pads to)
    const long long nblk = 6LL * n * mcu_h * mcu_w;
    return nblk <= 0x7fffffffLL && nblk == (long long)blocks;
}

}  // namespace

extern "C" int vk_jpeg_dct_quant_u8(const void* frames, void* coef, const VkJpegQuant* quant, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!frames || !coef || !quant || n <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return VK_EINVAL;
    if (quant->quality < 1 || quant->quality > 100) return VK_EINVAL;
    if (!aligned_to(coef, 16)) return VK_EINVAL;
    DevQuant dq;
    for (int k = 0; k < 64; ++k) {
        if (quant->luma[k] < 1 || quant->luma[k] > 255 || quant->chroma[k] < 1 || quant->chroma[k] > 255) return VK_EINVAL;
        dq.q[0][k] = (float)quant->luma[k];
        dq.q[1][k] = (float)quant->chroma[k];
    }
    const long long mcu_h = (H + 15) / 16, mcu_w = (W + 15) / 16, tiles_x = (mcu_w + JA_TM - 1) / JA_TM;
    if (6LL * n * mcu_h * mcu_w > 0x7fffffffLL) return VK_EINVAL;    // (also bounds the grid: tiles <= MCUs)
    if ((long long)n * H * W * 3 > 0x7fffffffLL) return VK_EINVAL;
    const dim3 grid((unsigned)(tiles_x * mcu_h * n));
    const uint8_t* in = (const uint8_t*)frames;
    int16_t* out = (int16_t*)coef;
    // the width of the copy into LDS: a function of W and of the frames' address; the coefficients are the same on every path
    if ((W * 3) % 16 == 0 && aligned_to(frames, 16))
        hipLaunchKernelGGL(jpeg_dct_quant_kernel<16>, grid, dim3(JA_THREADS), 0, (hipStream_t)stream, in, out, dq, H, W, (int)mcu_h, (int)mcu_w, (int)tiles_x);
    else if ((W * 3) % 4 == 0 && aligned_to(frames, 4))
        hipLaunchKernelGGL(jpeg_dct_quant_kernel<4>, grid, dim3(JA_THREADS), 0, (hipStream_t)stream, in, out, dq, H, W, (int)mcu_h, (int)mcu_w, (int)tiles_x);
    else
        hipLaunchKernelGGL(jpeg_dct_quant_kernel<1>, grid, dim3(JA_THREADS), 0, (hipStream_t)stream, in, out, dq, H, W, (int)mcu_h, (int)mcu_w, (int)tiles_x);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_jpeg_interval_sizes(const void* coef, int32_t* sizes, int32_t n, int32_t mcu_h, int32_t mcu_w, int32_t blocks, void* stream) {
    if (!coef || !sizes || !jb_geometry_ok(n, mcu_h, mcu_w, blocks)) return VK_EINVAL;
    if (!aligned_to(coef, 16) || !aligned_to(sizes, 4)) return VK_EINVAL;
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)(n * mcu_h)), dim3(JB_THREADS), 0, (hipStream_t)stream, (const int16_t*)coef, sizes,
                       (const int64_t*)nullptr, (uint8_t*)nullptr, 0LL, mcu_h, mcu_w);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_jpeg_entropy_write(const void* coef, const int64_t* offsets, void* out, int64_t out_bytes, int32_t n, int32_t mcu_h, int32_t mcu_w,
                                     int32_t blocks, void* stream) {
    if (!coef || !offsets || !out || !jb_geometry_ok(n, mcu_h, mcu_w, blocks)) return VK_EINVAL;
    if (out_bytes <= 0 || out_bytes > 0x7fffffffLL) return VK_EINVAL;
    if (!aligned_to(coef, 16) || !aligned_to(offsets, 8)) return VK_EINVAL;
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)(n * mcu_h)), dim3(JB_THREADS), 0, (hipStream_t)stream, (const int16_t*)coef,
                       (int32_t*)nullptr, offsets, (uint8_t*)out, (long long)out_bytes, mcu_h, mcu_w);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
