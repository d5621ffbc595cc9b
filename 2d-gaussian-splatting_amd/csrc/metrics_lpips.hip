// metrics_lpips.hip — image-quality evaluation: the VGG16 feature stack of LPIPS as an implicit GEMM on the f32-input MFMA, its pool,
// the LPIPS tap and the squared-error partial sums of PSNR (include/surfel_metrics.h, METRICS.md).  Everything is fp32; a metric's
// third decimal is what gets reported.  v_mfma_f32_32x32x2_f32 is bit-for-bit a k-ordered fmaf chain, so a result depends on the
// k order alone (tap by tap, channel by channel), not on the tiling.  No atomics; no scratch.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_metrics.h"
#include "block_ops.h"
#include "side_util.h"

namespace surfel {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT = 256;                    // threads per workgroup
constexpr int CT = 16;                     // output tile edge of the convolution (16 x 16 pixels = M 256)
constexpr int CH = CT + 2;                 // the tile with its one-pixel halo
constexpr int CPS = 352;                   // floats between two channel planes of the staged tile (>= CH * CH; 352 % 64 == 32: the two
                                           // k of one MFMA step read different LDS bank halves)
constexpr int CN = 64;                     // output channels per workgroup (N)
constexpr int NPART = SURFEL_METRICS_PARTIALS;

// ---- preparation -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT) lpips_prepare_kernel(int64_t hw, const float* __restrict__ x, const float* __restrict__ y,
                                                           float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (p >= hw) return;
    const float* src = blockIdx.y == 0 ? x : y;
    float4 v;
    v.x = (src[p] - (-.030f)) / .458f;
    v.y = (src[hw + p] - (-.088f)) / .448f;
    v.z = (src[2 * hw + p] - (-.188f)) / .450f;
    v.w = 0.f;
    reinterpret_cast<float4*>(out)[(int64_t)blockIdx.y * hw + p] = v;
}

// ---- 3 x 3 convolution + bias + ReLU ---------------------------------------------------------------------------------------------------
// One workgroup: a 16 x 16 pixel tile of one image times 64 output channels.  Wave w owns tile rows 4w .. 4w + 3 as two M tiles of
// 32 pixels (2 rows x 16 columns) times two N tiles of 32 channels: four independent 32 x 32 accumulators.  The input channels come in
// chunks of KC: the tile with its halo is staged as s_in[channel][18 x 18] (zero outside the image: the padding of the arithmetic), the
// weights as s_w[tap][channel][64].  Lane l of v_mfma_f32_32x32x2_f32 holds A[pixel l & 31][k = l >> 5] and B[k = l >> 5][channel l & 31].
template <int KC>
__global__ void __launch_bounds__(MT) lpips_conv3x3_kernel(int H, int W, int cin, int cout, const float* __restrict__ in,
                                                           const float* __restrict__ weight, const float* __restrict__ bias,
                                                           float* __restrict__ out) {
    __shared__ float s_in[KC * CPS];
    __shared__ __attribute__((aligned(16))) float s_w[9 * KC * CN];
    const int tiles_x = (W + CT - 1) / CT;
    const int x0 = (blockIdx.x % tiles_x) * CT, y0 = (blockIdx.x / tiles_x) * CT;
    const int n0 = blockIdx.y * CN;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

    int base_a[2];
#pragma unroll
    for (int m = 0; m < 2; m++) base_a[m] = (4 * wave + 2 * m + (li >> 4)) * CH + (li & 15);

    constexpr int K4 = KC / 4;
    for (int c0 = 0; c0 < cin; c0 += KC) {
        __syncthreads();
        for (int idx = tid; idx < CH * CH * K4; idx += MT) {
            const int pix = idx / K4, c4 = idx % K4;
            const int gy = y0 - 1 + pix / CH, gx = x0 - 1 + pix % CH;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(in + (img + (int64_t)gy * W + gx) * cin + c0 + 4 * c4);
            s_in[(4 * c4 + 0) * CPS + pix] = v.x;
            s_in[(4 * c4 + 1) * CPS + pix] = v.y;
            s_in[(4 * c4 + 2) * CPS + pix] = v.z;
            s_in[(4 * c4 + 3) * CPS + pix] = v.w;
        }
        for (int idx = tid; idx < 9 * KC * (CN / 4); idx += MT) {
            const int row = idx / (CN / 4), col4 = idx % (CN / 4);      // row = tap * KC + k
            const int tap = row / KC, k = row % KC;
            *reinterpret_cast<float4*>(s_w + row * CN + 4 * col4) =
                *reinterpret_cast<const float4*>(weight + ((int64_t)tap * cin + c0 + k) * cout + n0 + 4 * col4);
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int off = (tap / 3) * CH + (tap % 3);
#pragma unroll
            for (int kk = 0; kk < KC; kk += 2) {
                const int k = kk + lh;
                const float a0 = s_in[k * CPS + base_a[0] + off], a1 = s_in[k * CPS + base_a[1] + off];
                const float b0 = s_w[(tap * KC + k) * CN + li], b1 = s_w[(tap * KC + k) * CN + 32 + li];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // C/D of the 32 x 32 forms: column (channel) = lane & 31, row (pixel of the M tile) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int co = n0 + 32 * n + li;
        const float b = bias[co];
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int gy = y0 + 4 * wave + 2 * m + (row >> 4), gx = x0 + (row & 15);
                if (gy < H && gx < W) out[(img + (int64_t)gy * W + gx) * cout + co] = fmaxf(acc[m][n][r] + b, 0.f);
            }
    }
}

// ---- 2 x 2 max-pool ---------------------------------------------------------------------------------------------------------------------
__device__ inline float4 max4(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }

__global__ void __launch_bounds__(MT) lpips_pool_kernel(int H, int W, int C4, const float4* __restrict__ in, float4* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t total = (int64_t)2 * Ho * Wo * C4;
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int xo = (int)(p % Wo);
    p /= Wo;
    const int yo = (int)(p % Ho), img = (int)(p / Ho);
    const int64_t a = (((int64_t)img * H + 2 * yo) * W + 2 * xo) * C4 + c;
    const int64_t row = (int64_t)W * C4;
    out[i] = max4(max4(in[a], in[a + C4]), max4(in[a + row], in[a + row + C4]));
}

// ---- the LPIPS tap ---------------------------------------------------------------------------------------------------------------------
// G = min(64, C / 4) lanes share a pixel, each holding up to two float4 of either image's features.
__global__ void __launch_bounds__(MT) lpips_tap_kernel(int64_t hw, int C, const float* __restrict__ feat, const float* __restrict__ lin,
                                                       float* __restrict__ partials) {
    __shared__ float sh[MT];
    const int G = C / 4 < 64 ? C / 4 : 64;
    const int per_block = MT / G;
    const int sub = threadIdx.x % G, slot = threadIdx.x / G;
    float4 w[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int c4 = sub + j * G;
        w[j] = 4 * c4 < C ? reinterpret_cast<const float4*>(lin)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float acc[1] = {0.f};
    // (every lane of a wave runs the same number of iterations: the shuffles below need them all; a pixel past the end reads nothing)
    for (int64_t p0 = (int64_t)blockIdx.x * per_block; p0 < hw; p0 += (int64_t)gridDim.x * per_block) {
        const int64_t p = p0 + slot;
        float4 fx[2], fy[2];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int c4 = sub + j * G;
            fx[j] = fy[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < hw && 4 * c4 < C) {
                fx[j] = reinterpret_cast<const float4*>(feat + p * C)[c4];
                fy[j] = reinterpret_cast<const float4*>(feat + (hw + p) * C)[c4];
            }
            sx += (fx[j].x * fx[j].x + fx[j].y * fx[j].y) + (fx[j].z * fx[j].z + fx[j].w * fx[j].w);
            sy += (fy[j].x * fy[j].x + fy[j].y * fy[j].y) + (fy[j].z * fy[j].z + fy[j].w * fy[j].w);
        }
        for (int o = G / 2; o > 0; o >>= 1) {
            sx += __shfl_xor(sx, o);
            sy += __shfl_xor(sy, o);
        }
        const float dx = sqrtf(sx) + 1e-10f, dy = sqrtf(sy) + 1e-10f;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const float d0 = fx[j].x / dx - fy[j].x / dy, d1 = fx[j].y / dx - fy[j].y / dy;
            const float d2 = fx[j].z / dx - fy[j].z / dy, d3 = fx[j].w / dx - fy[j].w / dy;
            s += (w[j].x * (d0 * d0) + w[j].y * (d1 * d1)) + (w[j].z * (d2 * d2) + w[j].w * (d3 * d3));
        }
        for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (sub == 0) acc[0] += s;
    }
    block_tree_sum<MT>(acc, sh);      // in a fixed order
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// ---- squared error ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MT) sq_err_kernel(int64_t n, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ partials) {
    __shared__ float sh[MT];
    float acc[1] = {0.f};
    for (int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT) {
        const float d = a[i] - b[i];
        acc[0] += d * d;
    }
    block_tree_sum<MT>(acc, sh);      // in a fixed order
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {
inline bool bad_size(int H, int W) { return H <= 0 || W <= 0; }
inline bool too_large(int H, int W) { return H > SURFEL_LPIPS_MAX_EDGE || W > SURFEL_LPIPS_MAX_EDGE; }
}  // namespace

extern "C" {

int64_t surfel_lpips_workspace_bytes(int H, int W, int64_t budget_bytes) {
    if (bad_size(H, W)) return api_fail(SURFEL_E_INVALID, "lpips_workspace_bytes: bad arguments");
    if (too_large(H, W)) return api_fail(SURFEL_E_LIMIT, "lpips_workspace_bytes: an image edge exceeds SURFEL_LPIPS_MAX_EDGE");
    const int64_t act = (((int64_t)2 * H * W * 64 * 4) + 255) / 256 * 256;
    const int64_t bytes = 2 * act + (int64_t)6 * NPART * 4;
    if (bytes > budget_bytes) return api_fail(SURFEL_E_LIMIT, "lpips_workspace_bytes: the activations of this image size exceed the byte budget (raise the budget)");
    return bytes;
}

int surfel_lpips_prepare(int H, int W, const float* x, const float* y, float* out, void* stream) {
    if (bad_size(H, W) || !x || !y || !out) return api_fail(SURFEL_E_INVALID, "lpips_prepare: bad arguments");
    if (too_large(H, W)) return api_fail(SURFEL_E_LIMIT, "lpips_prepare: an image edge exceeds SURFEL_LPIPS_MAX_EDGE");
    const int64_t hw = (int64_t)H * W;
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3((unsigned)((hw + MT - 1) / MT), 2), dim3(MT), 0, static_cast<hipStream_t>(stream), hw, x, y, out);
    return launched("lpips_prepare_kernel");
}

int surfel_lpips_conv3x3(int H, int W, int cin, int cout, const float* in, const float* weight, const float* bias, float* out, void* stream) {
    if (bad_size(H, W) || !in || !weight || !bias || !out || in == out) return api_fail(SURFEL_E_INVALID, "lpips_conv3x3: bad arguments");
    if ((cin != 4 && (cin <= 0 || cin % 16)) || cout <= 0 || cout % CN)
        return api_fail(SURFEL_E_INVALID, "lpips_conv3x3: cin must be 4 or a multiple of 16, cout a multiple of 64");
    if (too_large(H, W) || cin > 4096 || cout > 4096) return api_fail(SURFEL_E_LIMIT, "lpips_conv3x3: an image edge exceeds SURFEL_LPIPS_MAX_EDGE or a layer has more than 4096 channels");
    const dim3 grid((unsigned)(((W + CT - 1) / CT) * ((H + CT - 1) / CT)), (unsigned)(cout / CN), 2);
    if (cin == 4)
        hipLaunchKernelGGL(lpips_conv3x3_kernel<4>, grid, dim3(MT), 0, static_cast<hipStream_t>(stream), H, W, cin, cout, in, weight, bias, out);
    else
        hipLaunchKernelGGL(lpips_conv3x3_kernel<16>, grid, dim3(MT), 0, static_cast<hipStream_t>(stream), H, W, cin, cout, in, weight, bias, out);
    return launched("lpips_conv3x3_kernel");
}

int surfel_lpips_pool(int H, int W, int C, const float* in, float* out, void* stream) {
    if (bad_size(H, W) || C <= 0 || C % 4 || !in || !out || in == out) return api_fail(SURFEL_E_INVALID, "lpips_pool: bad arguments");
    if (too_large(H, W) || C > 4096) return api_fail(SURFEL_E_LIMIT, "lpips_pool: an image edge exceeds SURFEL_LPIPS_MAX_EDGE or more than 4096 channels");
    const int64_t total = (int64_t)2 * (H / 2) * (W / 2) * (C / 4);
    if (total == 0) return 0;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total + MT - 1) / MT)), dim3(MT), 0, static_cast<hipStream_t>(stream), H, W, C / 4,
                       reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out));
    return launched("lpips_pool_kernel");
}

int surfel_lpips_tap(int H, int W, int C, const float* feat, const float* lin, float* partials, void* stream) {
    if (bad_size(H, W) || !feat || !lin || !partials) return api_fail(SURFEL_E_INVALID, "lpips_tap: bad arguments");
    if (C != 64 && C != 128 && C != 256 && C != 512) return api_fail(SURFEL_E_INVALID, "lpips_tap: C must be 64, 128, 256 or 512");
    if (too_large(H, W)) return api_fail(SURFEL_E_LIMIT, "lpips_tap: an image edge exceeds SURFEL_LPIPS_MAX_EDGE");
    hipLaunchKernelGGL(lpips_tap_kernel, dim3(NPART), dim3(MT), 0, static_cast<hipStream_t>(stream), (int64_t)H * W, C, feat, lin, partials);
    return launched("lpips_tap_kernel");
}

int surfel_sq_err_partials(int64_t n, const float* a, const float* b, float* partials, void* stream) {
    if (n < 0 || !partials || (n > 0 && (!a || !b))) return api_fail(SURFEL_E_INVALID, "sq_err_partials: bad arguments");
    hipLaunchKernelGGL(sq_err_kernel, dim3(NPART), dim3(MT), 0, static_cast<hipStream_t>(stream), n, a, b, partials);
    return launched("sq_err_kernel");
}

}  // extern "C"
