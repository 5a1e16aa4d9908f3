// Image I/O of the sampling front door (gfx950): the two ends of a run that touch 8-bit pictures.
//   vk_lanczos_resize_u8  : crop + Pillow's 8-bit LANCZOS resize (integer two-pass, bit-exact) + ToTensor + x*2-1   (sample.py:174-201)
//   vk_frames_to_u8       : fp32 NCHW frames -> uint8 HWC frames or one make_grid canvas                            (sample_utils.py:96-137)
// Both are HBM-bound element kernels: a thread owns four neighbouring output pixels so that the 8-bit side moves 12 bytes and the fp32 side
// 16 bytes at a time wherever the row width allows it. No storage-type dependence: the same object code goes into both libraries.
#include "common.h"
#include "vista_hip.h"

namespace {

constexpr int IO_THREADS = 256;
constexpr int PRECISION_BITS = 32 - 8 - 2;   // Pillow's fixed-point weight scale for 8-bit channels (Resample.c)

__host__ inline int io_grid(long long n) {
    long long g = (n + IO_THREADS - 1) / IO_THREADS;
    const long long cap = 256LL * 32;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}
#define IO_GRID_STRIDE(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

__device__ __forceinline__ uint32_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- pass 1: rows of the crop box -> rows of out_w pixels. src (n, src_h, src_w, 3) u8; tmp (n, crop_h, out_w, 3) u8.
// bounds[2*xx] = first source column of the crop, bounds[2*xx+1] = tap count; coef[xx*ksize + t] the fixed-point weights.
__global__ void lanczos_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp, const int* __restrict__ bounds,
                                 const int* __restrict__ coef, int ksize, int n_img, int src_h, int src_w, int left, int top, int crop_h,
                                 int out_w) {
    const int groups = (out_w + 3) >> 2;
    const long long total = (long long)n_img * crop_h * groups;
    const bool wide = (out_w & 3) == 0;   // every 4-pixel group is whole and its 12 bytes start on a 4-byte boundary
    IO_GRID_STRIDE(i, total) {
        const int g = (int)(i % groups);
        const long long iy = i / groups;
        const int y = (int)(iy % crop_h);
        const int img = (int)(iy / crop_h);
        const uint8_t* row = src + (((size_t)img * src_h + (top + y)) * src_w + left) * 3;
        uint8_t* dst = tmp + (((size_t)img * crop_h + y) * out_w + g * 4) * 3;
        uint32_t px[12];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xx = g * 4 + e;
            int r = 1 << (PRECISION_BITS - 1), gch = r, b = r;
            if (xx < out_w) {
                const int x0 = bounds[2 * xx], cnt = bounds[2 * xx + 1];
                const int* k = coef + (size_t)xx * ksize;
                const uint8_t* p = row + (size_t)x0 * 3;
                for (int t = 0; t < cnt; ++t) {
                    const int w = k[t];
                    r += (int)p[3 * t] * w;
                    gch += (int)p[3 * t + 1] * w;
                    b += (int)p[3 * t + 2] * w;
                }
            }
            px[3 * e] = clip8(r);
            px[3 * e + 1] = clip8(gch);
            px[3 * e + 2] = clip8(b);
        }
        if (wide) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int q = 0; q < 3; ++q) d32[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | (px[4 * q + 3] << 24);
        } else {
            const int valid = min(4, out_w - g * 4) * 3;
            for (int q = 0; q < valid; ++q) dst[q] = (uint8_t)px[q];
        }
    }
}

// ---- pass 2: columns of tmp -> out (n, 3, out_h, out_w) fp32 through the 256-entry value table (k/255*2-1 as the host computed it).
__global__ void lanczos_v_kernel(const uint8_t* __restrict__ tmp, float* __restrict__ out, const int* __restrict__ bounds,
                                 const int* __restrict__ coef, int ksize, const float* __restrict__ lut, int n_img, int crop_h, int out_h,
                                 int out_w) {
    const int groups = (out_w + 3) >> 2;
    const long long total = (long long)n_img * out_h * groups;
    const bool wide = (out_w & 3) == 0;
    IO_GRID_STRIDE(i, total) {
        const int g = (int)(i % groups);
        const long long iy = i / groups;
        const int yy = (int)(iy % out_h);
        const int img = (int)(iy / out_h);
        const int y0 = bounds[2 * yy], cnt = bounds[2 * yy + 1];
        const int* k = coef + (size_t)yy * ksize;
        int acc[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) acc[q] = 1 << (PRECISION_BITS - 1);
        const size_t row_bytes = (size_t)out_w * 3;
        const uint8_t* p = tmp + ((size_t)img * crop_h + y0) * row_bytes + (size_t)g * 12;
        if (wide) {
            for (int t = 0; t < cnt; ++t) {
                const int w = k[t];
                const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p + t * row_bytes);   // (out_w % 4 == 0: row_bytes and g*12 are multiples of 4)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t v = p32[q];
                    acc[4 * q] += (int)(v & 0xffu) * w;
                    acc[4 * q + 1] += (int)((v >> 8) & 0xffu) * w;
                    acc[4 * q + 2] += (int)((v >> 16) & 0xffu) * w;
                    acc[4 * q + 3] += (int)(v >> 24) * w;
                }
            }
        } else {
            const int valid = min(4, out_w - g * 4) * 3;
            for (int t = 0; t < cnt; ++t) {
                const int w = k[t];
                const uint8_t* pr = p + t * row_bytes;
                for (int q = 0; q < valid; ++q) acc[q] += (int)pr[q] * w;
            }
        }
        const size_t plane = (size_t)out_h * out_w;
        float* o = out + (size_t)img * 3 * plane + (size_t)yy * out_w + g * 4;
        if (wide) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4 v;
                v.x = lut[clip8(acc[c])];
                v.y = lut[clip8(acc[3 + c])];
                v.z = lut[clip8(acc[6 + c])];
                v.w = lut[clip8(acc[9 + c])];
                *reinterpret_cast<float4*>(o + c * plane) = v;
            }
        } else {
            const int nx = min(4, out_w - g * 4);
            for (int e = 0; e < nx; ++e)
                for (int c = 0; c < 3; ++c) o[c * plane + e] = lut[clip8(acc[3 * e + c])];
        }
    }
}

// numpy's float32 expressions of perform_save_locally, one rounding per operation (no contraction into an FMA), then the truncating cast.
__device__ __forceinline__ uint32_t to_u8(float x, int real) {
    float v = real ? __fmul_rn(255.0f, __fadd_rn(x, 1.0f)) * 0.5f : __fmul_rn(255.0f, x);   // (* 0.5f is exact: the reference divides by 2.0)
    return (uint32_t)((int)v) & 0xffu;
}

// ---- frames / grid: x (n, 3, H, W) fp32 -> canvas (rows, cols, 3) u8. pad = 0: rows = n*H, cols = W (n separate frames, back to back).
// pad > 0: the make_grid canvas, tile k at (k / xmaps * (H + pad) + pad, k % xmaps * (W + pad) + pad), everything else the map of 0.
__global__ void frames_to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int n_img, int H, int W, int xmaps, int pad,
                                    int rows, int cols, int real) {
    const int groups = (cols + 3) >> 2;
    const long long total = (long long)rows * groups;
    const bool wide = (cols & 3) == 0;
    const size_t plane = (size_t)H * W;
    const uint32_t pad_byte = to_u8(0.0f, real);
    IO_GRID_STRIDE(i, total) {
        const int g = (int)(i % groups);
        const int r = (int)(i / groups);
        uint32_t px[12];
        if (pad == 0 && wide) {   // whole, 16-byte aligned groups of one frame row
            const int img = r / H, y = r - img * H;
            const float* p = x + (size_t)img * 3 * plane + (size_t)y * W + g * 4;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(p + c * plane);
                px[c] = to_u8(v.x, real);
                px[3 + c] = to_u8(v.y, real);
                px[6 + c] = to_u8(v.z, real);
                px[9 + c] = to_u8(v.w, real);
            }
        } else {
            const int th = H + pad, tw = W + pad;
            const int ty = pad ? r / th : r / H;
            const int y = pad ? r - ty * th - pad : r - ty * H;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cx = g * 4 + e;
                const int tx = pad ? cx / tw : 0;
                const int xx = pad ? cx - tx * tw - pad : cx;
                const int k = pad ? ty * xmaps + tx : ty;
                const bool inside = cx < cols && y >= 0 && xx >= 0 && tx < xmaps && k < n_img;
                if (inside) {
                    const float* p = x + (size_t)k * 3 * plane + (size_t)y * W + xx;
                    px[3 * e] = to_u8(p[0], real);
                    px[3 * e + 1] = to_u8(p[plane], real);
                    px[3 * e + 2] = to_u8(p[2 * plane], real);
                } else {
                    px[3 * e] = px[3 * e + 1] = px[3 * e + 2] = pad_byte;
                }
            }
        }
        uint8_t* dst = out + ((size_t)r * cols + g * 4) * 3;
        if (wide) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int q = 0; q < 3; ++q) d32[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | (px[4 * q + 3] << 24);
        } else {
            const int valid = min(4, cols - g * 4) * 3;
            for (int q = 0; q < valid; ++q) dst[q] = (uint8_t)px[q];
        }
    }
}

}  // namespace

extern "C" int vk_lanczos_resize_u8(const void* src, void* tmp, float* out, const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x,
                                    const int32_t* bounds_y, const int32_t* coef_y, int32_t ksize_y, const float* lut256, int32_t n_img,
                                    int32_t src_h, int32_t src_w, int32_t left, int32_t top, int32_t crop_h, int32_t crop_w, int32_t out_h,
                                    int32_t out_w, void* stream) {
    if (!src || !tmp || !out || !bounds_x || !coef_x || !bounds_y || !coef_y || !lut256) return VK_EINVAL;
    if (n_img <= 0 || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0 || ksize_x <= 0 || ksize_y <= 0) return VK_EINVAL;
    if (crop_h <= 0 || crop_w <= 0 || left < 0 || top < 0 || (long long)left + crop_w > src_w || (long long)top + crop_h > src_h) return VK_EINVAL;
    if ((((size_t)tmp) & 3) != 0 || (((size_t)out) & 15) != 0) return VK_EINVAL;
    hipLaunchKernelGGL(lanczos_h_kernel, dim3(io_grid((long long)n_img * crop_h * ((out_w + 3) / 4))), dim3(IO_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)src, (uint8_t*)tmp, (const int*)bounds_x, (const int*)coef_x, ksize_x, n_img, src_h, src_w, left, top, crop_h,
                       out_w);
    VK_CHECK_LAUNCH();
    hipLaunchKernelGGL(lanczos_v_kernel, dim3(io_grid((long long)n_img * out_h * ((out_w + 3) / 4))), dim3(IO_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)tmp, out, (const int*)bounds_y, (const int*)coef_y, ksize_y, lut256, n_img, crop_h, out_h, out_w);
    VK_CHECK_LAUNCH();
    return VK_OK;
}

extern "C" int vk_frames_to_u8(const float* x, void* out, int32_t n_img, int32_t H, int32_t W, int32_t xmaps, int32_t pad, int32_t real,
                               void* stream) {
    if (!x || !out || n_img <= 0 || H <= 0 || W <= 0 || pad < 0 || (real != 0 && real != 1)) return VK_EINVAL;
    if (pad > 0 && (xmaps <= 0 || xmaps > n_img)) return VK_EINVAL;
    if ((((size_t)x) & 15) != 0 || (((size_t)out) & 3) != 0) return VK_EINVAL;
    long long rows, cols;
    if (pad == 0) {
        rows = (long long)n_img * H;
        cols = W;
    } else {
        const long long ymaps = (n_img + xmaps - 1) / xmaps;
        rows = ymaps * (H + pad) + pad;
        cols = (long long)xmaps * (W + pad) + pad;
    }
    if (rows > 0x7fffffffLL || cols > 0x7fffffffLL) return VK_EINVAL;
    hipLaunchKernelGGL(frames_to_u8_kernel, dim3(io_grid(rows * ((cols + 3) / 4))), dim3(IO_THREADS), 0, (hipStream_t)stream, x, (uint8_t*)out,
                       n_img, H, W, pad ? xmaps : 1, pad, (int)rows, (int)cols, real);
    VK_CHECK_LAUNCH();
    return VK_OK;
}
