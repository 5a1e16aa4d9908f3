// PNG output (gfx950): the row filter and a deflate coder for the 8-bit frames the front doors already hold on the GPU.
//   vk_png_filter_u8     : (n, H, W, 3) uint8 -> (n, H, 1 + 3 W) uint8, per row the filter type libpng's heuristic picks and the filtered bytes
//   vk_png_deflate_plan  : per segment of seg_rows rows: tokens, histograms, length-limited Huffman codes, the coded tree description, the
//                          segment's size in bytes and its Adler-32 pair; the code tables go to a plan buffer
//   vk_png_deflate_write : every segment's bytes at the caller's offset, from the plan
// uint8 in, bytes out, integer arithmetic only: no storage-type dependence, the same object code goes into both libraries (as csrc/jpeg.hip).
//
// A segment is ONE dynamic-Huffman block (BTYPE 10; BFINAL on a frame's last segment), followed on every other segment by an empty stored block
// (3 zero bits, padding to the byte, 00 00 FF FF): every segment starts on a byte boundary and workgroups write disjoint bytes.
//
// Tokens (zlib's Z_RLE, restated): at position i >= 1 of the segment, if bytes i, i + 1, i + 2 equal byte i - 1, a match of distance 1 and length
// min(rest of the run inside the segment, 258); otherwise a literal. Equivalently, per maximal run of equal bytes: its first byte is a literal,
// the k bytes behind it are cut into blocks of 258 from the front, a block of 3 or more is one match, a shorter one is literals. A lane owns one
// byte of a 256-byte chunk: j, its distance from the run's start, comes from a max-scan of the start positions (carried from chunk to chunk), so
// r = (j - 1) % 258 is its place in its block: r >= 2 is inside a match; r == 1 is inside one iff the next byte continues the run; r == 0 finds
// the block's length, the distance to the run's end, in the ballots of "my run ends with me" over the chunk and its 258 bytes of lookahead (at
// most five 64-bit words, however long the run: a flat picture costs no more per chunk than a noisy one). A segment never has to fit LDS.
//
// Code construction, a pure function of a histogram (`limit` 15 for the literal/length alphabet, 7 for the code-length alphabet):
//   * fewer than two used symbols: symbols 0, then 1, are counted once until two are (inflate refuses an incomplete code-length or literal set);
//   * the used symbols are sorted by (count, symbol) ascending (a parallel rank); Huffman by two queues -- the leaves in that order, the internal
//     nodes in order of creation --, each time the lighter front, the LEAF on a tie; a symbol's length is its leaf's depth;
//   * if the longest length exceeds `limit`, every used count becomes (count + 1) >> 1 and the construction is repeated (it ends: equal counts
//     give a tree of depth 9 for 286 symbols and 5 for 19).
//   The distance alphabet holds distance 1 alone: one code of length 1 where the segment has a match, a single zero length where it has none --
//   the two incomplete sets inflate accepts. Codes are canonical (RFC 1951 3.2.2), stored bit-reversed: deflate packs bits LSB first.
//   The tree description is the literal/length lengths 0 .. HLIT + 256, then the one distance length, run-length coded: a run of r zeros is
//   18 (11 .. 138) while r >= 11, then 17 (3 .. 10) if r >= 3, else r times 0; a run of r equal lengths v > 0 is v, then 16 (3 .. 6) while at
//   least 3 remain, then v for each left. Runs do not cross from the literal/length lengths into the distance length.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int PN_THREADS = 256;
constexpr int PN_LOOK = 258;                              // bytes of lookahead behind a chunk
constexpr int PN_LIT = 286, PN_CL = 19;
constexpr int PN_ADLER = 65521;
constexpr int PN_HDR_WORDS = 130;                         // 17 + 19 * 3 + 287 * (7 + 7) = 4092 bits at most, and a word to spill into
constexpr int PN_CODES_AT = 4, PN_HDR_AT = PN_CODES_AT + PN_LIT;
static_assert(PN_HDR_AT + PN_HDR_WORDS == VK_PNG_PLAN_WORDS, "the plan layout of include/vista_hip.h");
constexpr int PN_BIT_WORDS = (PN_THREADS * 21 + 7 + 31) / 32 + 2;   // a chunk's tokens (15 + 5 + 1 bits at most each) and 7 carried bits
static_assert(PN_BIT_WORDS >= PN_HDR_WORDS, "the header is flushed through the same buffer");

// match length 3 .. 258 -> (length code 0 .. 28) | extra bits << 8 | extra value << 16
struct LenTable { uint32_t e[259]; };
constexpr LenTable make_len_table() {
    constexpr int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    constexpr int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    LenTable t{};
    for (int m = 3; m <= 258; ++m) {
        int k = 28;
        while (base[k] > m) --k;
        t.e[m] = (uint32_t)k | ((uint32_t)extra[k] << 8) | ((uint32_t)(m - base[k]) << 16);
    }
    return t;
}
__device__ __constant__ LenTable PN_LEN = make_len_table();
__device__ __constant__ uint8_t PN_LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ __constant__ uint8_t PN_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- filter ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t signed_abs(int v) {
    v &= 255;
    return (uint32_t)(v < 128 ? v : 256 - v);
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// One workgroup per row: five sums of |byte as int8| -> the type with the smallest, the lowest on a tie -> the row, coded with it.
__global__ __launch_bounds__(PN_THREADS) void png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ rows, int H, int W3) {
    __shared__ uint32_t part[5][PN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = blockIdx.x;
    const bool top = row % (size_t)H == 0;
    const uint8_t* cur = frames + row * (size_t)W3;
    const uint8_t* up = cur - W3;                     // (read only where !top)
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (int x = tid; x < W3; x += PN_THREADS) {
        const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = top ? 0 : up[x], c = (top || x < 3) ? 0 : up[x - 3];
        s[0] += signed_abs(v);
        s[1] += signed_abs(v - a);
        s[2] += signed_abs(v - b);
        s[3] += signed_abs(v - ((a + b) >> 1));
        s[4] += signed_abs(v - paeth(a, b, c));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t v = s[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) part[k][wave] = v;
    }
    __syncthreads();
    int best = 0;
    uint32_t best_sum = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < PN_THREADS / 64; ++w) v += part[k][w];
        if (k == 0 || v < best_sum) {
            best = k;
            best_sum = v;
        }
    }
    uint8_t* out = rows + row * ((size_t)W3 + 1);
    if (tid == 0) out[0] = (uint8_t)best;
    for (int x = tid; x < W3; x += PN_THREADS) {
        const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = top ? 0 : up[x], c = (top || x < 3) ? 0 : up[x - 3];
        const int pred = best == 0 ? 0 : best == 1 ? a : best == 2 ? b : best == 3 ? ((a + b) >> 1) : paeth(a, b, c);
        out[1 + x] = (uint8_t)(v - pred);
    }
}

// ---- deflate --------------------------------------------------------------------------------------------------------------------------------
// exclusive sum of v over the workgroup; *total = the sum. Two barriers; `part` is 4 words of LDS.
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
    for (int w = 0; w < PN_THREADS / 64; ++w) {
        const uint32_t p = part[w];
        if (w < wave) before += p;
        sum += p;
    }
    *total = sum;
    return before + inc - v;
}

// inclusive maximum of v over the lanes up to this one; *total = the maximum over the workgroup
__device__ __forceinline__ int block_scan_max(int v, int* part, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, up);
    }
    __syncthreads();
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int all = part[0];
#pragma unroll
    for (int w = 0; w < PN_THREADS / 64; ++w) {
        const int p = part[w];
        if (w < wave) inc = max(inc, p);
        all = max(all, p);
    }
    *total = all;
    return inc;
}

struct Builder {                                       // LDS scratch of the code construction
    uint32_t f[PN_LIT + 2], lw[PN_LIT + 2], iw[PN_LIT + 2];
    uint16_t order[PN_LIT + 2], leaf_parent[PN_LIT + 2], node_parent[PN_LIT + 2], depth[PN_LIT + 2];
    int again;
};

// freq[0 .. n) -> len[0 .. n), the rule of the header comment. Called by the whole workgroup; freq and len are LDS.
__device__ void build_lengths(const uint32_t* freq, int n, int limit, uint8_t* len, Builder& B) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int s = tid; s < n; s += PN_THREADS) B.f[s] = freq[s];
    __syncthreads();
    if (tid == 0) {
        int used = 0;
        for (int s = 0; s < n; ++s) used += B.f[s] != 0;
        for (int s = 0; s < 2; ++s)
            if (used < 2 && B.f[s] == 0) {
                B.f[s] = 1;
                ++used;
            }
    }
    __syncthreads();
    for (;;) {
        for (int s = tid; s < n; s += PN_THREADS) {
            len[s] = 0;
            const uint32_t fs = B.f[s];
            if (fs) {
                int rank = 0;
                for (int t = 0; t < n; ++t) {
                    const uint32_t ft = B.f[t];
                    rank += ft != 0 && (ft < fs || (ft == fs && t < s));
                }
                B.order[rank] = (uint16_t)s;
                B.lw[rank] = fs;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int m = 0;
            for (int s = 0; s < n; ++s) m += B.f[s] != 0;
            int li = 0, ni = 0;
            for (int k = 0; k < m - 1; ++k) {         // internal node k: the two lightest fronts
                uint32_t w = 0;
                for (int pick = 0; pick < 2; ++pick) {
                    if (li < m && (ni >= k || B.lw[li] <= B.iw[ni])) {
                        w += B.lw[li];
                        B.leaf_parent[li++] = (uint16_t)k;
                    } else {
                        w += B.iw[ni];
                        B.node_parent[ni++] = (uint16_t)k;
                    }
                }
                B.iw[k] = w;
            }
            if (m >= 2) B.depth[m - 2] = 0;
            for (int k = m - 3; k >= 0; --k) B.depth[k] = B.depth[B.node_parent[k]] + 1;
            int longest = 0;
            for (int i = 0; i < m; ++i) {
                const int d = B.depth[B.leaf_parent[i]] + 1;
                len[B.order[i]] = (uint8_t)min(d, 255);
                longest = max(longest, d);
            }
            B.again = longest > limit;
        }
        __syncthreads();
        if (!B.again) break;
        for (int s = tid; s < n; s += PN_THREADS) B.f[s] = (B.f[s] + 1) >> 1;
        __syncthreads();
    }
}

// canonical codes of len[0 .. n) -> e[s] = bit-reversed code | length << 16 (0 for an unused symbol). One lane.
__device__ void assign_codes(const uint8_t* len, int n, uint32_t* e) {
    uint32_t count[16], next[16];
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int s = 0; s < n; ++s) count[len[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        e[s] = l ? ((__brev(next[l]++) >> (32 - l)) | ((uint32_t)l << 16)) : 0u;
    }
}

struct BitWriter {                                     // one lane, LSB first, into zeroed words
    uint32_t* w;
    uint32_t at;
    __device__ void put(uint32_t v, int n) {
        if (n == 0) return;
        const uint32_t i = at >> 5, sh = at & 31u;
        const uint64_t x = (uint64_t)v << sh;
        w[i] |= (uint32_t)x;
        if (sh + n > 32) w[i + 1] |= (uint32_t)(x >> 32);
        at += (uint32_t)n;
    }
};

// One workgroup per segment: blockIdx.x = frame * segs + segment of the frame.
// WRITE = false: sizes[seg], adler[2 seg], adler[2 seg + 1] and plan[seg] are written. WRITE = true: the segment's bytes go to out + offsets[seg];
// a byte at or beyond out_bytes is not stored (offsets that do not come from the sizes cannot leave the buffer).
template <bool WRITE>
__global__ __launch_bounds__(PN_THREADS) void png_deflate_kernel(const uint8_t* __restrict__ rows, int32_t* __restrict__ sizes,
                                                                 uint32_t* __restrict__ adler, uint32_t* __restrict__ plan,
                                                                 const int64_t* __restrict__ offsets, uint8_t* __restrict__ out, long long out_bytes,
                                                                 int H, int row_bytes, int seg_rows, int segs) {
    __shared__ uint8_t buf[PN_THREADS + PN_LOOK + 2];
    __shared__ unsigned long long ends[8];
    __shared__ uint32_t part[PN_THREADS / 64];
    __shared__ int part_max[PN_THREADS / 64];
    __shared__ uint32_t codes[PN_LIT + 2];             // WRITE: the plan's table. plan pass: the literal/length histogram, then the table
    __shared__ uint32_t bits[PN_BIT_WORDS];            // WRITE: the bit buffer. plan pass: the header's bits
    const int tid = threadIdx.x;
    const int seg = blockIdx.x, k = seg % segs, frame = seg / segs;
    const int row0 = k * seg_rows, nrows = min(seg_rows, H - row0);
    const bool final = k == segs - 1;
    const int len = nrows * row_bytes;                 // (<= VK_PNG_MAX_SEGMENT_BYTES)
    const uint8_t* data = rows + ((size_t)frame * H + row0) * (size_t)row_bytes;
    uint32_t* my_plan = plan + (size_t)seg * VK_PNG_PLAN_WORDS;

    long long at = 0;
    uint32_t lead = 0, carry = 0;                      // bits (< 8) carried from the previous flush, and their value
    uint32_t dist_len = 0;
    unsigned long long a1 = 0, a2 = 0;                 // this lane's share of the Adler sums

    // the whole bytes of bits[0 .. nbits) go out at `at`; the rest is carried
    auto flush = [&](uint32_t nbits) {
        const uint32_t nbytes = nbits >> 3, rem = nbits & 7u;
        for (uint32_t i = tid; i < nbytes; i += PN_THREADS) {
            const long long p = at + i;
            if (p >= 0 && p < out_bytes) out[p] = (uint8_t)(bits[i >> 2] >> (8 * (i & 3u)));
        }
        carry = rem ? (bits[nbytes >> 2] >> (8 * (nbytes & 3u))) & ((1u << rem) - 1u) : 0u;
        lead = rem;
        at += nbytes;
    };

    if (WRITE) {
        at = offsets[seg];
        const uint32_t hbits = min(my_plan[0], (uint32_t)(PN_HDR_WORDS - 2) * 32u);
        dist_len = my_plan[1] & 1u;
        for (int i = tid; i < PN_LIT; i += PN_THREADS) codes[i] = my_plan[PN_CODES_AT + i];
        for (int i = tid; i < PN_HDR_WORDS; i += PN_THREADS) bits[i] = my_plan[PN_HDR_AT + i];
        __syncthreads();
        flush(hbits);
    } else {
        for (int i = tid; i < PN_LIT + 2; i += PN_THREADS) codes[i] = 0;
    }

    int run_start = -1;                                // where the run of the previous chunk's last byte began
    for (int base = 0; base < len; base += PN_THREADS) {
        __syncthreads();                               // the previous chunk's buf and bits have been read
        for (int i = tid; i < PN_THREADS + PN_LOOK; i += PN_THREADS) buf[i] = base + i < len ? data[base + i] : 0;
        const int g = base + tid;
        const bool have = g < len;
        const int before = (tid == 0 && g > 0 && have) ? (int)data[g - 1] : 0;
        __syncthreads();
        const int byte = buf[tid];
        const bool start = have && (g == 0 || byte != (tid == 0 ? before : (int)buf[tid - 1]));
        // ends[p >> 6] bit p & 63: the run of window position p ends with it (the next byte differs or lies behind the segment), p < 512
        const bool end0 = g + 1 >= len || buf[tid + 1] != byte;
        const bool end1 = g + PN_THREADS + 1 >= len || buf[tid + PN_THREADS + 1] != buf[tid + PN_THREADS];
        const unsigned long long mask0 = __ballot(end0), mask1 = __ballot(end1);
        if ((tid & 63) == 0) {
            ends[tid >> 6] = mask0;
            ends[4 + (tid >> 6)] = mask1;
        }
        int last_start;
        int rs = block_scan_max(start ? g : -1, part_max, &last_start);
        rs = max(rs, run_start);
        run_start = max(run_start, last_start);
        // ---- this byte's token: 0 none, 1 literal, m >= 3 a match of m ----
        int token = 0;
        if (have) {
            const int j = g - rs;
            if (j == 0) {
                token = 1;
            } else {
                const int r = (j - 1) % 258;
                if (r == 0) {                          // the block's length: to the run's end, 258 at most (no end among the next 257: 258)
                    int w = tid >> 6;
                    unsigned long long mk = ends[w] & (~0ull << (tid & 63));
                    while (!mk && w < 7 && (w + 1) * 64 <= tid + 257) mk = ends[++w];
                    const int m = mk ? min(258, w * 64 + __ffsll((long long)mk) - tid) : 258;
                    token = m >= 3 ? m : 1;
                } else if (r == 1) {
                    token = end0 ? 1 : 0;
                }
            }
        }
        uint32_t sym = 0, extra_bits = 0, extra = 0;
        if (token == 1) {
            sym = (uint32_t)byte;
        } else if (token >= 3) {
            const uint32_t e = PN_LEN.e[token];
            sym = 257u + (e & 255u);
            extra_bits = (e >> 8) & 255u;
            extra = e >> 16;
        }
        if (!WRITE) {
            if (token) atomicAdd(&codes[sym], 1u);
            if (have) {
                a1 += (unsigned)byte;
                a2 += (unsigned long long)(len - g) * (unsigned)byte;
            }
        } else {
            uint32_t v = 0, nb = 0;
            if (token) {
                const uint32_t e = codes[sym], l = min(e >> 16, 15u);   // (a foreign plan cannot outgrow the bit buffer)
                v = (e & 0xffffu) | (extra << l);      // (the distance code, where there is one, is a 0 bit)
                nb = l + extra_bits + (token >= 3 ? dist_len : 0u);
            }
            uint32_t total;
            const uint32_t begin = lead + block_scan(nb, part, &total);
            const uint32_t all_bits = lead + total;
            for (uint32_t i = tid; i < (all_bits + 31) / 32 + 1; i += PN_THREADS) bits[i] = i == 0 ? carry : 0u;
            __syncthreads();
            if (nb) {
                const uint32_t w = begin >> 5, sh = begin & 31u;
                const uint64_t x = (uint64_t)v << sh;
                atomicOr(&bits[w], (uint32_t)x);
                if (sh + nb > 32) atomicOr(&bits[w + 1], (uint32_t)(x >> 32));
            }
            __syncthreads();
            flush(all_bits);
        }
    }

    if (WRITE) {
        // ---- end of block, and behind every segment but a frame's last the empty stored block ----
        if (tid == 0) {
            const uint32_t e = codes[256], l = min(e >> 16, 15u);
            const uint64_t acc = (uint64_t)carry | ((uint64_t)(e & 0xffffu) << lead);
            const uint32_t n = lead + l + (final ? 0u : 3u);
            const uint32_t nbytes = (n + 7) >> 3;
            for (uint32_t i = 0; i < nbytes + (final ? 0u : 4u); ++i) {
                const long long p = at + i;
                const uint8_t b = i < nbytes ? (uint8_t)(acc >> (8 * i)) : (i - nbytes < 2 ? 0x00 : 0xff);
                if (p >= 0 && p < out_bytes) out[p] = b;
            }
        }
        return;
    }

    // ---- the plan ----
    __shared__ Builder B;
    __shared__ uint8_t lit_len[PN_LIT + 2], cl_len[PN_CL + 1], tree_sym[PN_LIT + 2], tree_extra[PN_LIT + 2];
    __shared__ uint32_t cl_hist[PN_CL + 1], cl_codes[PN_CL + 1];
    __shared__ unsigned long long sums[2];
    __shared__ int n_tree, hlit_s;
    __shared__ uint32_t n_match_s;
    if (tid == 0) {
        sums[0] = 0;
        sums[1] = 0;
    }
    __syncthreads();                                   // every token is counted
    atomicAdd(&sums[0], a1);
    atomicAdd(&sums[1], a2);
    if (tid == 0) codes[256] = 1;                      // the end of block
    build_lengths(codes, PN_LIT, 15, lit_len, B);
    if (tid < PN_CL) cl_hist[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        int hlit = 257;
        uint32_t n_match = 0;
        for (int s = 257; s < PN_LIT; ++s) {
            if (lit_len[s]) hlit = s + 1;
            n_match += codes[s];
        }
        n_match_s = n_match;
        hlit_s = hlit;
        int nt = 0;
        auto emit = [&](int s, int x) {
            tree_sym[nt] = (uint8_t)s;
            tree_extra[nt++] = (uint8_t)x;
            cl_hist[s]++;
        };
        for (int i = 0; i < hlit;) {
            const int v = lit_len[i];
            int r = 1;
            while (i + r < hlit && lit_len[i + r] == v) ++r;
            i += r;
            if (v == 0) {
                while (r >= 11) {
                    const int c = min(r, 138);
                    emit(18, c - 11);
                    r -= c;
                }
                if (r >= 3) {
                    emit(17, r - 3);
                    r = 0;
                }
                for (; r > 0; --r) emit(0, 0);
            } else {
                emit(v, 0);
                --r;
                while (r >= 3) {
                    const int c = min(r, 6);
                    emit(16, c - 3);
                    r -= c;
                }
                for (; r > 0; --r) emit(v, 0);
            }
        }
        emit(n_match ? 1 : 0, 0);                      // the one distance length
        n_tree = nt;
    }
    build_lengths(cl_hist, PN_CL, 7, cl_len, B);
    for (int i = tid; i < PN_HDR_WORDS; i += PN_THREADS) bits[i] = 0;
    __syncthreads();
    if (tid == 0) {
        assign_codes(cl_len, PN_CL, cl_codes);
        int hclen = 4;
        for (int i = 0; i < PN_CL; ++i)
            if (cl_len[PN_CL_ORDER[i]]) hclen = max(hclen, i + 1);
        BitWriter w{bits, 0};
        w.put(final ? 1u : 0u, 1);
        w.put(2, 2);
        w.put((uint32_t)(hlit_s - 257), 5);
        w.put(0, 5);
        w.put((uint32_t)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) w.put(cl_len[PN_CL_ORDER[i]], 3);
        for (int i = 0; i < n_tree; ++i) {
            const int s = tree_sym[i];
            w.put(cl_codes[s] & 0xffffu, (int)(cl_codes[s] >> 16));
            w.put(tree_extra[i], s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
        const uint32_t dl = n_match_s ? 1u : 0u;
        unsigned long long nbits = w.at;
        for (int s = 0; s < PN_LIT; ++s)
            nbits += (unsigned long long)codes[s] * (lit_len[s] + (s >= 257 ? (uint32_t)PN_LEN_EXTRA[s - 257] + dl : 0u));
        const unsigned long long bytes = final ? (nbits + 7) >> 3 : ((nbits + 3 + 7) >> 3) + 4;
        sizes[seg] = (int32_t)bytes;
        adler[2 * (size_t)seg] = (uint32_t)((1ull + sums[0]) % PN_ADLER);
        adler[2 * (size_t)seg + 1] = (uint32_t)(((unsigned long long)len + sums[1]) % PN_ADLER);
        my_plan[0] = w.at;
        my_plan[1] = dl;
        my_plan[2] = 0;
        my_plan[3] = 0;
    }
    __syncthreads();                                   // the histogram has been read: the table takes its place
    if (tid == 0) assign_codes(lit_len, PN_LIT, codes);
    __syncthreads();
    for (int i = tid; i < PN_LIT; i += PN_THREADS) my_plan[PN_CODES_AT + i] = codes[i];
    for (int i = tid; i < PN_HDR_WORDS; i += PN_THREADS) my_plan[PN_HDR_AT + i] = bits[i];
}

// n frames of H rows of row_bytes in segments of seg_rows -> the segments of one frame, or 0 where the extents are outside the limits
long long png_segments(int32_t n, int32_t H, int32_t row_bytes, int32_t seg_rows) {
    if (n <= 0 || H <= 0 || row_bytes <= 0 || seg_rows <= 0) return 0;
    if ((long long)n * H * row_bytes > 0x7fffffffLL) return 0;
    if ((long long)(seg_rows < H ? seg_rows : H) * row_bytes > VK_PNG_MAX_SEGMENT_BYTES) return 0;
    return ((long long)H + seg_rows - 1) / seg_rows;
}

}  // namespace

extern "C" int vk_png_filter_u8(const void* frames, void* rows, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!frames || !rows || n <= 0 || H <= 0 || W <= 0 || H > VK_PNG_MAX_EXTENT || W > VK_PNG_MAX_EXTENT) return VK_EINVAL;
    if ((long long)n * H * (3LL * W + 1) > 0x7fffffffLL) return VK_EINVAL;    // (also bounds the grid: n H workgroups)
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)(n * H)), dim3(PN_THREADS), 0, (hipStream_t)stream, (const uint8_t*)frames, (uint8_t*)rows, H,
                       3 * W);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_png_deflate_plan(const void* rows, int32_t* sizes, uint32_t* adler, uint32_t* plan, int32_t n, int32_t H, int32_t row_bytes,
                                   int32_t seg_rows, int32_t segments, void* stream) {
    const long long segs = png_segments(n, H, row_bytes, seg_rows);
    if (!rows || !sizes || !adler || !plan || segs == 0 || segs * n != (long long)segments) return VK_EINVAL;
    if (!aligned_to(sizes, 4) || !aligned_to(adler, 4) || !aligned_to(plan, 4)) return VK_EINVAL;
    hipLaunchKernelGGL(png_deflate_kernel<false>, dim3((unsigned)segments), dim3(PN_THREADS), 0, (hipStream_t)stream, (const uint8_t*)rows, sizes, adler,
                       plan, (const int64_t*)nullptr, (uint8_t*)nullptr, 0LL, H, row_bytes, seg_rows, (int)segs);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_png_deflate_write(const void* rows, const uint32_t* plan, const int64_t* offsets, void* out, int64_t out_bytes, int32_t n, int32_t H,
                                    int32_t row_bytes, int32_t seg_rows, int32_t segments, void* stream) {
    const long long segs = png_segments(n, H, row_bytes, seg_rows);
    if (!rows || !plan || !offsets || !out || segs == 0 || segs * n != (long long)segments) return VK_EINVAL;
    if (out_bytes <= 0 || out_bytes > 0x7fffffffLL) return VK_EINVAL;
    if (!aligned_to(plan, 4) || !aligned_to(offsets, 8)) return VK_EINVAL;
    hipLaunchKernelGGL(png_deflate_kernel<true>, dim3((unsigned)segments), dim3(PN_THREADS), 0, (hipStream_t)stream, (const uint8_t*)rows,
                       (int32_t*)nullptr, (uint32_t*)nullptr, const_cast<uint32_t*>(plan), offsets, (uint8_t*)out, (long long)out_bytes, H, row_bytes,
                       seg_rows, (int)segs);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
