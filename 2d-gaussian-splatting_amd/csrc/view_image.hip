// view_image.hip — the image kernels of the live viewer (include/surfel_view.h, VIEWER.md): a scalar map (an input plane, or the Sobel
// gradient magnitude of three planes) -> its minimum and maximum on the device -> interleaved 8-bit turbo pixels.
// Compiled without contraction (build.py): every operation rounds once, like its numpy restatement (tests/view_oracle.py).
// Three launches per image: the key reset (one store pair), the map / reduction pass, the colouring pass.  lo and hi stay on the
// device as order-preserving integer keys, merged with integer atomics: no floating-point sum, so the bytes do not change from run to run.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/surfel_view.h"
#include "block_ops.h"
#include "side_util.h"
#include "vis_pixels.h"
#include "vis_turbo_table.h"

namespace surfel {

constexpr int VW_T = 256;                 // threads per workgroup
constexpr int VW_TW = 32, VW_TH = 8;      // pixels per workgroup of the gradient pass: one per thread, half a wave per tile row
constexpr int VW_LW = VW_TW + 2, VW_LH = VW_TH + 2;      // the tile with its one-pixel halo; rows of 34 floats: a wave reads two
                                                         // rows, 32 consecutive banks each, and the LDS serves the two halves apart
constexpr uint32_t KEY_NONE_LO = 0xffffffffu, KEY_NONE_HI = 0u;      // identities of min / max: no float that is not NaN has these keys
static_assert(VW_T == VW_TW * VW_TH, "one pixel per thread");

__global__ void view_reset_kernel(uint32_t* __restrict__ keys) {
    if (threadIdx.x == 0) {
        keys[0] = KEY_NONE_LO;
        keys[1] = KEY_NONE_HI;
    }
}

// (lo, hi) of the workgroup's lanes into keys[0], keys[1]: xor-shuffles inside the wave, the four waves' results through LDS, one atomic
// min and one atomic max by thread 0.  Every thread of the workgroup calls it.
__device__ __forceinline__ void merge_keys(uint32_t lo, uint32_t hi, uint32_t* __restrict__ keys) {
    __shared__ uint32_t s_lo[VW_T / 64], s_hi[VW_T / 64];
    lo = wave_min(lo); hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < VW_T / 64; w++) {
            lo = min(lo, s_lo[w]);
            hi = max(hi, s_hi[w]);
        }
        if (lo != KEY_NONE_LO) atomicMin(&keys[0], lo);      // (a workgroup of NaNs has nothing to add)
        if (hi != KEY_NONE_HI) atomicMax(&keys[1], hi);
    }
}

// Alpha, Depth: the map is there; four pixels per lane
__global__ void __launch_bounds__(VW_T) view_minmax_kernel(int64_t hw, const float* __restrict__ map, uint32_t* __restrict__ keys) {
    const int64_t i = ((int64_t)blockIdx.x * VW_T + threadIdx.x) * PX;
    uint32_t lo = KEY_NONE_LO, hi = KEY_NONE_HI;
    if (i < hw) {
        float v[PX];
        load4(map, i, hw, v);
#pragma unroll
        for (int j = 0; j < PX; j++)
            if (i + j < hw && v[j] == v[j]) {
                const uint32_t k = order_key(v[j]);
                lo = min(lo, k);
                hi = max(hi, k);
            }
    }
    merge_keys(lo, hi, keys);
}

// Edge, Curvature: gradient_map (Sobel / 4 with zero padding per channel, L2 over the channels) of planes * scale + bias
__global__ void __launch_bounds__(VW_T) view_gradient_kernel(int H, int W, const float* __restrict__ planes, float scale, float bias,
                                                             float* __restrict__ m, uint32_t* __restrict__ keys) {
    __shared__ float s_t[3][VW_LH][VW_LW];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * VW_TW, y0 = blockIdx.y * VW_TH;
    const int64_t hw = (int64_t)H * W;
    for (int k = t; k < 3 * VW_LH * VW_LW; k += VW_T) {
        const int c = k / (VW_LH * VW_LW), r = k % (VW_LH * VW_LW);
        const int ly = r / VW_LW, lx = r % VW_LW;
        const int gy = y0 + ly - 1, gx = x0 + lx - 1;
        float v = 0.0f;                                   // the padding is 0 whatever scale and bias are
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = __fadd_rn(__fmul_rn(planes[c * hw + (int64_t)gy * W + gx], scale), bias);
        s_t[c][ly][lx] = v;
    }
    __syncthreads();
    const int lx = t & (VW_TW - 1), ly = t / VW_TW;
    const int px = x0 + lx, py = y0 + ly;
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a = s_t[c][ly][lx], b = s_t[c][ly][lx + 1], cc = s_t[c][ly][lx + 2];
        const float d = s_t[c][ly + 1][lx], f = s_t[c][ly + 1][lx + 2];
        const float g = s_t[c][ly + 2][lx], h = s_t[c][ly + 2][lx + 1], i = s_t[c][ly + 2][lx + 2];
        const float gx = __fadd_rn(__fadd_rn(__fmul_rn(__fsub_rn(cc, a), 0.25f), __fmul_rn(__fsub_rn(f, d), 0.5f)), __fmul_rn(__fsub_rn(i, g), 0.25f));
        const float gy = __fadd_rn(__fadd_rn(__fmul_rn(__fsub_rn(g, a), 0.25f), __fmul_rn(__fsub_rn(h, b), 0.5f)), __fmul_rn(__fsub_rn(i, cc), 0.25f));
        const float q = __fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy));
        s = c == 0 ? q : __fadd_rn(s, q);
    }
    const float mag = __fsqrt_rn(s);
    uint32_t lo = KEY_NONE_LO, hi = KEY_NONE_HI;
    if (px < W && py < H) {
        m[(int64_t)py * W + px] = mag;
        if (mag == mag) lo = hi = order_key(mag);
    }
    merge_keys(lo, hi, keys);
}

// colormap + clamp * 255 + byte + permute: the table sits in LDS (one read per pixel at a data-dependent index)
__global__ void __launch_bounds__(VW_T) view_colour_kernel(int64_t hw, const float* __restrict__ m, const uint32_t* __restrict__ keys,
                                                           uint8_t* __restrict__ dst) {
    __shared__ uint32_t s_tab[256];
    static_assert(VW_T == 256, "one table entry per thread");
    s_tab[threadIdx.x] = VIS_TURBO[threadIdx.x];
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * VW_T + threadIdx.x) * PX;
    if (i >= hw) return;
    const float lo = order_value(keys[0]), hi = order_value(keys[1]);      // (NaN, NaN) when no pixel had a value
    const float range = __fsub_rn(hi, lo);
    float v[PX];
    load4(m, i, hw, v);
    uint32_t c[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const float tt = __fdiv_rn(__fsub_rn(v[j], lo), range);
        int k = 0;                                        // a NaN t: entry 0
        if (tt == tt) {
            k = (int)rintf(__fmul_rn(tt, 255.0f));        // t is in [0, 1]: lo <= v <= hi and the roundings are monotonic
            k = k < 0 ? 0 : (k > 255 ? 255 : k);
        }
        c[j] = s_tab[k];
    }
    const uint32_t w[3] = {c[0] | c[1] << 24, c[1] >> 8 | c[2] << 16, c[2] >> 16 | c[3] << 8};
    store_bytes<3>(dst + i * 3, (int)min((int64_t)PX, hw - i) * 3, w);
}

namespace {

constexpr int VIEW_MAX_EDGE = 65536;

inline int view_check(const char* who, int H, int W, const void* src, const void* dst, const void* scratch, int64_t scratch_bytes) {
    const std::string name(who);
    if (H <= 0 || W <= 0 || !src || !dst || !scratch || (reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 3))
        return api_fail(SURFEL_E_INVALID, (name + ": bad arguments").c_str());
    if (H > VIEW_MAX_EDGE || W > VIEW_MAX_EDGE) return api_fail(SURFEL_E_LIMIT, (name + ": an image edge exceeds 65536").c_str());
    if (scratch_bytes < SURFEL_VIEW_SCRATCH_BYTES(H, W))
        return api_fail(SURFEL_E_INVALID, (name + ": scratch holds fewer than SURFEL_VIEW_SCRATCH_BYTES(H, W)").c_str());
    return 0;
}

inline unsigned view_blocks(int64_t hw) { return blocks_for(hw, (int64_t)VW_T * PX); }

}  // namespace
}  // namespace surfel

using namespace surfel;

extern "C" {

int surfel_view_scalar(int H, int W, const float* map, uint8_t* dst, void* scratch, int64_t scratch_bytes, void* stream) {
    if (const int rc = view_check("view_scalar", H, W, map, dst, scratch, scratch_bytes)) return rc;
    const int64_t hw = (int64_t)H * W;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* keys = static_cast<uint32_t*>(scratch);
    hipLaunchKernelGGL(view_reset_kernel, dim3(1), dim3(64), 0, s, keys);
    hipLaunchKernelGGL(view_minmax_kernel, dim3(view_blocks(hw)), dim3(VW_T), 0, s, hw, map, keys);
    hipLaunchKernelGGL(view_colour_kernel, dim3(view_blocks(hw)), dim3(VW_T), 0, s, hw, map, keys, dst);
    return launched("view_scalar kernels");
}

int surfel_view_gradient(int H, int W, const float* planes, float scale, float bias, uint8_t* dst, void* scratch, int64_t scratch_bytes,
                         void* stream) {
    if (const int rc = view_check("view_gradient", H, W, planes, dst, scratch, scratch_bytes)) return rc;
    const int64_t hw = (int64_t)H * W;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* keys = static_cast<uint32_t*>(scratch);
    float* m = reinterpret_cast<float*>(static_cast<char*>(scratch) + 64);
    hipLaunchKernelGGL(view_reset_kernel, dim3(1), dim3(64), 0, s, keys);
    hipLaunchKernelGGL(view_gradient_kernel, dim3((W + VW_TW - 1) / VW_TW, (H + VW_TH - 1) / VW_TH), dim3(VW_T), 0, s, H, W, planes, scale, bias, m, keys);
    hipLaunchKernelGGL(view_colour_kernel, dim3(view_blocks(hw)), dim3(VW_T), 0, s, hw, m, keys, dst);
    return launched("view_gradient kernels");
}

}  // extern "C"
