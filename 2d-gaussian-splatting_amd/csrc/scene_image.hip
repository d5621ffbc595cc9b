// scene_image.hip — the capture loader's image path (include/surfel_scene.h, SCENE.md): Pillow's 8-bit BICUBIC resampling (tables on the
// host, the two passes on the device), the u8 -> float planar conversion with the alpha split, and the Blender RGBA composite.
// Everything is exact: int32 accumulation of u8 x 2^22-scaled weights, one correctly rounded fp32 division, fp64 for the composite.
// Compiled without contraction (build.py), so the fp64 expressions below round operation by operation like their numpy restatement
// (tests/scene_oracle.py).  No atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_scene.h"
#include "side_util.h"

namespace surfel {

constexpr int PREC = SURFEL_SCENE_PRECISION_BITS;
constexpr int ST = 256;      // threads per workgroup
constexpr int HX = 64;       // horizontal pass: output columns per workgroup (one per lane) ...
constexpr int HR = ST / 64;  // ... times rows (one per wave)

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> PREC;      // arithmetic shift
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ float unit(uint8_t v) { return __fdiv_rn((float)v, 255.0f); }

// one finished pixel: interleaved bytes (an intermediate) or v / 255 into the planes (and the mask when C = 4)
template <int C, bool FLOAT_OUT>
__device__ __forceinline__ void store_pixel(const int (&acc)[C], int64_t pix, int64_t plane, uint8_t* __restrict__ dst_u8,
                                            float* __restrict__ planes, float* __restrict__ mask) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint8_t v = clip8(acc[c]);
        if (!FLOAT_OUT)
            dst_u8[pix * C + c] = v;
        else if (c < 3)
            planes[c * plane + pix] = unit(v);
        else
            mask[pix] = unit(v);
    }
}

// ---- horizontal pass ------------------------------------------------------------------------------------------------------------------
// A workgroup owns HX output columns of HR rows.  The source bytes those columns read (first tap of the first column to last tap of
// the last one) are staged per row in LDS as packed bytes: wave r copies row r with aligned dword loads, placed in LDS at the same
// offset mod 4 as in memory; the ragged head and tail of a row (C = 3, odd W) go byte by byte, so nothing outside the span is read.
// Lane l then owns column x0 + l: its taps are consecutive LDS bytes, its weights coeffs[tap][column] (tap-major: coalesced).
template <int C, bool FLOAT_OUT>
__global__ void __launch_bounds__(ST) resample_h_kernel(int H, int W, int W2, int ksize, int cap_px, int pitch, const uint8_t* __restrict__ src,
                                                        const int2* __restrict__ bounds, const int* __restrict__ coeffs,
                                                        uint8_t* __restrict__ dst_u8, float* __restrict__ planes, float* __restrict__ mask) {
    extern __shared__ uint32_t s_words[];
    uint8_t* s_bytes = reinterpret_cast<uint8_t*>(s_words);
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int x0 = blockIdx.x * HX, y = blockIdx.y * HR + r;
    const int xl = min(x0 + HX, W2) - 1;
    const int2 bf = bounds[x0], bl = bounds[xl];
    const int s0 = min(max(bf.x, 0), W);
    const int s1 = min(min(max(bl.x + bl.y, s0), W), s0 + cap_px);      // a table that is not this axis's cannot leave the row or the LDS
    const int span = (s1 - s0) * C;
    uint8_t* row = s_bytes + r * pitch;
    int mis = 0;
    if (y < H) {
        const uint8_t* g = src + ((int64_t)y * W + s0) * C;
        mis = (int)(reinterpret_cast<uintptr_t>(g) & 3);
        const int head = min((4 - mis) & 3, span);
        const int nd = (span - head) >> 2;
        const int tail = head + 4 * nd;
        const uint32_t* g4 = reinterpret_cast<const uint32_t*>(g + head);
        uint32_t* s4 = reinterpret_cast<uint32_t*>(row + mis + head);
        for (int i = lane; i < nd; i += 64) s4[i] = g4[i];
        if (lane < head) row[mis + lane] = g[lane];
        if (lane >= 32 && tail + lane - 32 < span) row[mis + tail + lane - 32] = g[tail + lane - 32];
    }
    __syncthreads();
    const int x = x0 + lane;
    if (y >= H || x >= W2) return;
    const int2 b = bounds[x];
    int n = b.y;
    if (b.x < s0 || n < 0 || n > ksize || b.x + n > s1) n = 0;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (PREC - 1);
    const uint8_t* p = row + mis + (b.x - s0) * C;
    const int* k = coeffs + x;
    for (int t = 0; t < n; t++) {
        const int w = k[(int64_t)t * W2];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += (int)p[t * C + c] * w;
    }
    store_pixel<C, FLOAT_OUT>(acc, (int64_t)y * W2 + x, (int64_t)H * W2, dst_u8, planes, mask);
}

// ---- vertical pass --------------------------------------------------------------------------------------------------------------------
// One thread per output pixel, lanes along x: every tap row is one coalesced read of C bytes per lane, and the row's bounds and weights
// are the same for the whole workgroup (blockIdx.y = output row).
template <int C, bool FLOAT_OUT>
__global__ void __launch_bounds__(ST) resample_v_kernel(int H, int W, int H2, int ksize, const uint8_t* __restrict__ src,
                                                        const int2* __restrict__ bounds, const int* __restrict__ coeffs,
                                                        uint8_t* __restrict__ dst_u8, float* __restrict__ planes, float* __restrict__ mask) {
    const int x = blockIdx.x * ST + threadIdx.x, y2 = blockIdx.y;
    if (x >= W) return;
    const int2 b = bounds[y2];
    int n = b.y;
    if (b.x < 0 || n < 0 || n > ksize || b.x + n > H) n = 0;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (PREC - 1);
    const uint8_t* p = src + ((int64_t)b.x * W + x) * C;
    const int64_t step = (int64_t)W * C;
    for (int t = 0; t < n; t++, p += step) {
        const int w = coeffs[(int64_t)t * H2 + y2];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += (int)p[c] * w;
    }
    store_pixel<C, FLOAT_OUT>(acc, (int64_t)y2 * W + x, (int64_t)H2 * W, dst_u8, planes, mask);
}

// ---- conversion alone (no pass runs) and the composite -------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(ST) to_float_kernel(int64_t hw, const uint8_t* __restrict__ src, float* __restrict__ planes, float* __restrict__ mask) {
    const int64_t pix = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (pix >= hw) return;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float f = unit(src[pix * C + c]);
        if (c < 3)
            planes[c * hw + pix] = f;
        else
            mask[pix] = f;
    }
}

__global__ void __launch_bounds__(ST) composite_kernel(int64_t hw, double bg, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
    const int64_t pix = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (pix >= hw) return;
    const double na = (double)src[pix * 4 + 3] / 255.0;
    const double rest = bg * (1.0 - na);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double arr = ((double)src[pix * 4 + c] / 255.0) * na + rest;
        dst[pix * 3 + c] = (uint8_t)(int)(arr * 255.0);
    }
}

namespace {

inline bool bad_edge(int v) { return v <= 0; }
inline bool big_edge(int v) { return v > SURFEL_SCENE_MAX_EDGE; }

double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Axis {
    double scale, filterscale, support;
    int ksize;
};

Axis axis_of(int in_size, int out_size) {
    Axis a;
    a.scale = (double)in_size / out_size;
    a.filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * a.filterscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}

int check_pass(const char* what, int H, int W, int C, int out, int ksize, const void* src, const void* bounds, const void* coeffs, const void* dst_u8,
               const void* planes, const void* mask) {
    if (bad_edge(H) || bad_edge(W) || bad_edge(out) || (C != 1 && C != 3 && C != 4) || ksize <= 0 || !src || !bounds || !coeffs ||
        (!dst_u8 && (!planes || (C == 4 && !mask))))
        return api_fail(SURFEL_E_INVALID, what);
    if (big_edge(H) || big_edge(W) || big_edge(out) || ksize > SURFEL_SCENE_MAX_KSIZE)
        return api_fail(SURFEL_E_LIMIT, "scene resample: an image edge exceeds SURFEL_SCENE_MAX_EDGE or ksize exceeds SURFEL_SCENE_MAX_KSIZE");
    return 0;
}

}  // namespace
}  // namespace surfel

using namespace surfel;

extern "C" {

int surfel_scene_resample_table(int in_size, int out_size, int* bounds, int* coeffs, int64_t capacity) {
    if (bad_edge(in_size) || bad_edge(out_size) || (!bounds) != (!coeffs)) return api_fail(SURFEL_E_INVALID, "scene_resample_table: bad arguments");
    if (big_edge(in_size) || big_edge(out_size)) return api_fail(SURFEL_E_LIMIT, "scene_resample_table: an image edge exceeds SURFEL_SCENE_MAX_EDGE");
    const Axis a = axis_of(in_size, out_size);
    if (a.ksize > SURFEL_SCENE_MAX_KSIZE) return api_fail(SURFEL_E_LIMIT, "scene_resample_table: ksize exceeds SURFEL_SCENE_MAX_KSIZE (a reduction beyond 48 x)");
    if (!bounds) return a.ksize;
    if (capacity < (int64_t)a.ksize * out_size) return api_fail(SURFEL_E_INVALID, "scene_resample_table: coeffs holds fewer than ksize * out_size ints");
    const double ss = 1.0 / a.filterscale;
    double kk[SURFEL_SCENE_MAX_KSIZE];
    for (int xx = 0; xx < out_size; xx++) {
        const double center = (xx + 0.5) * a.scale;
        double ww = 0.0;
        int xmin = (int)(center - a.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + a.support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; x++) {
            const double w = bicubic((x + xmin - center + 0.5) * ss);
            kk[x] = w;
            ww += w;
        }
        for (int x = 0; x < a.ksize; x++) {
            double k = 0.0;
            if (x < xmax) k = ww != 0.0 ? kk[x] / ww : kk[x];
            coeffs[(int64_t)x * out_size + xx] = k < 0 ? (int)(-0.5 + k * (1 << PREC)) : (int)(0.5 + k * (1 << PREC));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return a.ksize;
}

#define SCENE_PASS(KERNEL, GRID, LDS, ...)                                                                                         \
    do {                                                                                                                           \
        const hipStream_t s_ = static_cast<hipStream_t>(stream);                                                                   \
        if (dst_u8) {                                                                                                              \
            if (C == 1) hipLaunchKernelGGL((KERNEL<1, false>), GRID, dim3(ST), LDS, s_, __VA_ARGS__);                              \
            else if (C == 3) hipLaunchKernelGGL((KERNEL<3, false>), GRID, dim3(ST), LDS, s_, __VA_ARGS__);                         \
            else hipLaunchKernelGGL((KERNEL<4, false>), GRID, dim3(ST), LDS, s_, __VA_ARGS__);                                     \
        } else {                                                                                                                   \
            if (C == 1) hipLaunchKernelGGL((KERNEL<1, true>), GRID, dim3(ST), LDS, s_, __VA_ARGS__);                               \
            else if (C == 3) hipLaunchKernelGGL((KERNEL<3, true>), GRID, dim3(ST), LDS, s_, __VA_ARGS__);                          \
            else hipLaunchKernelGGL((KERNEL<4, true>), GRID, dim3(ST), LDS, s_, __VA_ARGS__);                                      \
        }                                                                                                                          \
    } while (0)

int surfel_scene_resample_h(int H, int W, int C, int W2, int ksize, const uint8_t* src, const int* bounds, const int* coeffs, uint8_t* dst_u8,
                            float* dst_planes, float* dst_mask, void* stream) {
    const int rc = check_pass("scene_resample_h: bad arguments", H, W, C, W2, ksize, src, bounds, coeffs, dst_u8, dst_planes, dst_mask);
    if (rc < 0) return rc;
    const Axis a = axis_of(W, W2);
    if (a.ksize != ksize) return api_fail(SURFEL_E_INVALID, "scene_resample_h: ksize is not that of (W, W2)");
    // source samples under HX consecutive outputs: centres (HX - 1) * scale apart, support (+ rounding) on either side
    const int cap_px = (int)fmin((double)W, ceil((HX - 1) * a.scale + 2.0 * a.support) + 2.0);
    const int pitch = (cap_px * C + 3 + 3) & ~3;
    const size_t lds = (size_t)HR * pitch;
    if (lds > 64 * 1024) return api_fail(SURFEL_E_LIMIT, "scene_resample_h: the source span of a strip exceeds the LDS");
    const dim3 grid((unsigned)((W2 + HX - 1) / HX), (unsigned)((H + HR - 1) / HR));
    SCENE_PASS(resample_h_kernel, grid, lds, H, W, W2, ksize, cap_px, pitch, src, reinterpret_cast<const int2*>(bounds), coeffs, dst_u8, dst_planes,
               dst_mask);
    return launched("resample_h_kernel");
}

int surfel_scene_resample_v(int H, int W, int C, int H2, int ksize, const uint8_t* src, const int* bounds, const int* coeffs, uint8_t* dst_u8,
                            float* dst_planes, float* dst_mask, void* stream) {
    const int rc = check_pass("scene_resample_v: bad arguments", H, W, C, H2, ksize, src, bounds, coeffs, dst_u8, dst_planes, dst_mask);
    if (rc < 0) return rc;
    if (axis_of(H, H2).ksize != ksize) return api_fail(SURFEL_E_INVALID, "scene_resample_v: ksize is not that of (H, H2)");
    const dim3 grid((unsigned)((W + ST - 1) / ST), (unsigned)H2);
    SCENE_PASS(resample_v_kernel, grid, 0, H, W, H2, ksize, src, reinterpret_cast<const int2*>(bounds), coeffs, dst_u8, dst_planes, dst_mask);
    return launched("resample_v_kernel");
}

int surfel_scene_to_float(int H, int W, int C, const uint8_t* src, float* dst_planes, float* dst_mask, void* stream) {
    if (bad_edge(H) || bad_edge(W) || (C != 1 && C != 3 && C != 4) || !src || !dst_planes || (C == 4 && !dst_mask))
        return api_fail(SURFEL_E_INVALID, "scene_to_float: bad arguments");
    if (big_edge(H) || big_edge(W)) return api_fail(SURFEL_E_LIMIT, "scene_to_float: an image edge exceeds SURFEL_SCENE_MAX_EDGE");
    const int64_t hw = (int64_t)H * W;
    const dim3 grid((unsigned)((hw + ST - 1) / ST));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C == 1) hipLaunchKernelGGL(to_float_kernel<1>, grid, dim3(ST), 0, s, hw, src, dst_planes, dst_mask);
    else if (C == 3) hipLaunchKernelGGL(to_float_kernel<3>, grid, dim3(ST), 0, s, hw, src, dst_planes, dst_mask);
    else hipLaunchKernelGGL(to_float_kernel<4>, grid, dim3(ST), 0, s, hw, src, dst_planes, dst_mask);
    return launched("to_float_kernel");
}

int surfel_scene_composite(int H, int W, int white, const uint8_t* src, uint8_t* dst, void* stream) {
    if (bad_edge(H) || bad_edge(W) || !src || !dst) return api_fail(SURFEL_E_INVALID, "scene_composite: bad arguments");
    if (big_edge(H) || big_edge(W)) return api_fail(SURFEL_E_LIMIT, "scene_composite: an image edge exceeds SURFEL_SCENE_MAX_EDGE");
    const int64_t hw = (int64_t)H * W;
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((hw + ST - 1) / ST)), dim3(ST), 0, static_cast<hipStream_t>(stream), hw, white ? 1.0 : 0.0, src,
                       dst);
    return launched("composite_kernel");
}

}  // extern "C"
