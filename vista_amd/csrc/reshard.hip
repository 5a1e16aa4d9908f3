// Exchange packing of the frame-sharded step (gfx950): every gather / scatter around an all-to-all of vista_amd/parallel.py in ONE launch.
//   vk_copy_row_boxes : copies up to VK_RESHARD_MAX_BOXES strided 3-D boxes of whole rows from `src` to `dst`.
// A re-shard plan (frames <-> pixels, their chunked form, the halo frames, a rank's rows of a replicated tensor) is a union of at most one box
// per peer rank: rows (b, t, s) of a box go from  src_row + b*src_stride_b + t*src_stride_t + s  to  dst_row + b*dst_stride_b + t*dst_stride_t + s,
// so the `ns` rows of one (b, t) are one contiguous run of ns * row_bytes bytes on both sides. The plan travels BY VALUE in the kernel argument
// (no index tensors, nothing for the caller to keep alive, capturable). An HBM copy: 16-byte loads and stores over one flat list of 16-byte
// units, four loads in flight per thread, values in registers only (no LDS). No storage-type dependence: the same object code goes into both libraries.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_UNROLL = 4;
// memory-bound grid: enough 256-thread blocks to fill the chip (256 CUs x 8 blocks), the rest of the work by grid stride
constexpr long long RS_MAX_BLOCKS = 256LL * 8;

// What the kernel needs of a VkRowBox, in 16-byte units: a run = the ns rows of one (b, t).
struct DevBox {
    int64_t src_unit, dst_unit;                        // first unit of the box on either side
    int64_t src_stride_b, src_stride_t, dst_stride_b, dst_stride_t;   // in units
    int64_t run_units;                                 // ns * row_units
    int32_t nt, pad;
};
struct DevPlan {
    int32_t n, pad;
    int64_t first[VK_RESHARD_MAX_BOXES + 1];           // prefix sum of the boxes' unit counts (empty boxes dropped by the host)
    DevBox box[VK_RESHARD_MAX_BOXES];
};

template <typename IDX>
__device__ __forceinline__ void box_units(const DevBox& bx, int64_t local, int64_t& s, int64_t& d) {
    const IDX l = (IDX)local;
    const IDX run = l / (IDX)bx.run_units;
    const IDX in_run = l - run * (IDX)bx.run_units;
    const IDX b = run / (IDX)bx.nt;
    const IDX t = run - b * (IDX)bx.nt;
    s = bx.src_unit + (int64_t)b * bx.src_stride_b + (int64_t)t * bx.src_stride_t + (int64_t)in_run;
    d = bx.dst_unit + (int64_t)b * bx.dst_stride_b + (int64_t)t * bx.dst_stride_t + (int64_t)in_run;
}

// Unit u of the flat work list -> its source and destination unit. The box is found by counting the prefix sums at or below u (a uniform loop
// over scalar loads of the argument). The 64 units of a wave are consecutive, so nearly always they share one box: every lane computes with
// the FIRST lane's box, whose index is wave-uniform, so its fields come through the scalar path and the divisors are uniform. Only the lanes of
// a wave that straddles a box boundary redo the arithmetic with their own box, indexing the argument per lane.
template <typename IDX>
__device__ __forceinline__ void locate(const DevPlan& p, int64_t u, int64_t& s, int64_t& d) {
    int k = 0;
    for (int i = 1; i < p.n; ++i) k += (u >= p.first[i]) ? 1 : 0;
    const int ku = __builtin_amdgcn_readfirstlane(k);
    box_units<IDX>(p.box[ku], u - p.first[ku], s, d);   // (a lane of another box gets numbers it throws away: run_units and nt are >= 1)
    if (k != ku) box_units<IDX>(p.box[k], u - p.first[k], s, d);
}

// IDX = uint32_t when the whole work list has fewer than 2^32 units (every real plan): the two divisions per unit are 32-bit.
// Four units per thread and trip while all four lie inside the list: all four addresses first, then the four loads back to back, then the
// four stores, so nothing but registers holds the values. The last, partial trip of a thread copies its units one at a time.
template <typename IDX>
__global__ void __launch_bounds__(RS_THREADS) copy_row_boxes_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const DevPlan p) {
    const int64_t total = p.first[p.n];
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    static_assert(RS_UNROLL == 4, "the body below is written out for four slots");
    int64_t u0 = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    for (; u0 + 3 * stride < total; u0 += 4 * stride) {
        int64_t s0, s1, s2, s3, d0, d1, d2, d3;
        locate<IDX>(p, u0, s0, d0);
        locate<IDX>(p, u0 + stride, s1, d1);
        locate<IDX>(p, u0 + 2 * stride, s2, d2);
        locate<IDX>(p, u0 + 3 * stride, s3, d3);
        const uint4 v0 = src[s0];
        const uint4 v1 = src[s1];
        const uint4 v2 = src[s2];
        const uint4 v3 = src[s3];
        dst[d0] = v0;
        dst[d1] = v1;
        dst[d2] = v2;
        dst[d3] = v3;
    }
#pragma unroll 1
    for (; u0 < total; u0 += stride) {
        int64_t s, d;
        locate<IDX>(p, u0, s, d);
        dst[d] = src[s];
    }
}

// lo / hi = smallest / largest row a non-empty box touches; false on int64 overflow
__host__ bool box_row_range(int64_t row, int64_t stride_b, int64_t stride_t, int32_t nb, int32_t nt, int32_t ns, int64_t* lo, int64_t* hi) {
    int64_t eb, et;
    if (__builtin_mul_overflow(stride_b, (int64_t)(nb - 1), &eb) || __builtin_mul_overflow(stride_t, (int64_t)(nt - 1), &et)) return false;
    int64_t l = row, h = row;
    if (__builtin_add_overflow(l, eb < 0 ? eb : 0, &l) || __builtin_add_overflow(l, et < 0 ? et : 0, &l)) return false;
    if (__builtin_add_overflow(h, eb > 0 ? eb : 0, &h) || __builtin_add_overflow(h, et > 0 ? et : 0, &h)) return false;
    if (__builtin_add_overflow(h, (int64_t)(ns - 1), &h)) return false;
    *lo = l;
    *hi = h;
    return true;
}

}  // namespace

extern "C" int vk_copy_row_boxes(const void* src, void* dst, const VkRowBoxes* boxes, int64_t src_rows, int64_t dst_rows, int32_t row_bytes,
                                 void* stream) {
    if (!src || !dst || !boxes) return VK_EINVAL;
    if ((((size_t)src) & 15) != 0 || (((size_t)dst) & 15) != 0) return VK_EINVAL;
    if (row_bytes <= 0 || (row_bytes & 15) != 0 || src_rows < 0 || dst_rows < 0) return VK_EINVAL;
    const int32_t n = boxes->n;
    if (n < 1 || n > VK_RESHARD_MAX_BOXES) return VK_EINVAL;
    const int64_t ru = row_bytes / 16;
    // a unit index is row * ru + the unit inside the row: every index and every stride in units stays below 2^60
    const int64_t max_rows = ((int64_t)1 << 60) / ru;
    if (src_rows > max_rows || dst_rows > max_rows) return VK_EINVAL;
    DevPlan p;
    p.n = 0;
    p.pad = 0;
    p.first[0] = 0;
    for (int i = 0; i < n; ++i) {
        const VkRowBox& b = boxes->box[i];
        if (b.nb < 0 || b.nt < 0 || b.ns < 0) return VK_EINVAL;
        if (b.nb == 0 || b.nt == 0 || b.ns == 0) continue;   // a zero-size box (a rank whose pixel slice is empty) is legal and skipped
        int64_t lo, hi;
        if (!box_row_range(b.src_row, b.src_stride_b, b.src_stride_t, b.nb, b.nt, b.ns, &lo, &hi) || lo < 0 || hi >= src_rows) return VK_EINVAL;
        if (!box_row_range(b.dst_row, b.dst_stride_b, b.dst_stride_t, b.nb, b.nt, b.ns, &lo, &hi) || lo < 0 || hi >= dst_rows) return VK_EINVAL;
        // (a stride that is used -- nb or nt > 1 -- is below the row count in magnitude for a box that is in range; an unused one is dropped)
        DevBox& d = p.box[p.n];
        d.src_unit = b.src_row * ru;
        d.dst_unit = b.dst_row * ru;
        d.src_stride_b = b.nb > 1 ? b.src_stride_b * ru : 0;
        d.src_stride_t = b.nt > 1 ? b.src_stride_t * ru : 0;
        d.dst_stride_b = b.nb > 1 ? b.dst_stride_b * ru : 0;
        d.dst_stride_t = b.nt > 1 ? b.dst_stride_t * ru : 0;
        d.run_units = (int64_t)b.ns * ru;
        d.nt = b.nt;
        d.pad = 0;
        int64_t units;
        if (__builtin_mul_overflow((int64_t)b.nb * b.nt, d.run_units, &units) || units > ((int64_t)1 << 60) - p.first[p.n]) return VK_EINVAL;
        p.first[p.n + 1] = p.first[p.n] + units;
        ++p.n;
    }
    if (p.n == 0) return VK_OK;   // nothing but empty boxes: no launch
    for (int i = p.n; i < VK_RESHARD_MAX_BOXES; ++i) {
        p.first[i + 1] = p.first[p.n];
        p.box[i] = DevBox{0, 0, 0, 0, 0, 0, 1, 1, 0};
    }
    const int64_t total = p.first[p.n];
    long long grid = (total + (long long)RS_THREADS * RS_UNROLL - 1) / ((long long)RS_THREADS * RS_UNROLL);
    if (grid > RS_MAX_BLOCKS) grid = RS_MAX_BLOCKS;
    if (total < ((int64_t)1 << 32))
        hipLaunchKernelGGL(copy_row_boxes_kernel<uint32_t>, dim3((unsigned)grid), dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint4*)src,
                           (uint4*)dst, p);
    else
        hipLaunchKernelGGL(copy_row_boxes_kernel<uint64_t>, dim3((unsigned)grid), dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint4*)src,
                           (uint4*)dst, p);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
