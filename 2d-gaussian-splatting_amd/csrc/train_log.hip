// train_log.hip — the device half of the training log (include/surfel_log.h, LOG.md): the step ring's append and the report panels.
// Compiled without contraction (build.py, and the pragma below for a build that forgets the flag): the round-to-nearest intrinsics are
// plain operators to the compiler, and a fused 0.4 * v + 0.6 * ema would not be the Python restatement's (tests/log_oracle.py).
// The extrema of the colour-mapped panels are taken as view_image.hip takes them: order-preserving integer keys, merged with integer
// atomics, so the bytes do not change from run to run.  (Its reset and reduction kernels are restated here: without relocatable device
// code a kernel of another translation unit cannot be launched from this one.)
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_log.h"
#include "block_ops.h"
#include "log_jet_table.h"
#include "side_util.h"
#include "vis_pixels.h"
#include "vis_turbo_table.h"

#pragma clang fp contract(off)

namespace surfel {

int log_fail(int code, const char* what) { return api_fail(code, what); }      // for log_events.cpp, which sees no HIP header

struct LogState {      // SURFEL_LOG_STATE_BYTES
    double ema_dist, ema_normal;
    int64_t count, reserved;
};
struct LogRecord {     // SURFEL_LOG_RECORD_BYTES
    int32_t iteration, points;
    float reg_loss, total_loss, ema_dist, ema_normal, raw_total;
    uint32_t seq;
};
static_assert(sizeof(LogState) == SURFEL_LOG_STATE_BYTES && sizeof(LogRecord) == SURFEL_LOG_RECORD_BYTES, "the layouts of surfel_log.h");

// train.py:97-98: ema = 0.4 * v + 0.6 * ema on Python floats: two products and a sum, each rounded
__device__ __forceinline__ double log_ema(double ema, float v) { return __dadd_rn(__dmul_rn(0.4, (double)v), __dmul_rn(0.6, ema)); }

__global__ void __launch_bounds__(64) log_append_kernel(LogState* __restrict__ state, LogRecord* __restrict__ ring, int capacity, int iteration,
                                                        int points, const float* __restrict__ scalars, float lambda_normal, float lambda_dist) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float ll1 = scalars[0], normal_err = scalars[2], dist = scalars[3], photometric = scalars[4], total = scalars[5];
    const double ema_dist = log_ema(state->ema_dist, __fmul_rn(lambda_dist, dist));
    const double ema_normal = log_ema(state->ema_normal, __fmul_rn(lambda_normal, normal_err));
    const int64_t count = state->count;
    LogRecord r;
    r.iteration = iteration;
    r.points = points;
    r.reg_loss = ll1;
    r.total_loss = photometric;
    r.ema_dist = (float)ema_dist;
    r.ema_normal = (float)ema_normal;
    r.raw_total = total;
    r.seq = (uint32_t)count;
    ring[count % capacity] = r;
    state->ema_dist = ema_dist;
    state->ema_normal = ema_normal;
    state->count = count + 1;
}

// ---- panels ---------------------------------------------------------------------------------------------------------------------------
constexpr int LP_T = 256;                 // threads per workgroup
constexpr uint32_t LP_NONE_LO = 0xffffffffu, LP_NONE_HI = 0u;      // identities of min / max: no float that is not NaN has these keys

__global__ void log_reset_kernel(uint32_t* __restrict__ keys) {
    if (threadIdx.x == 0) {
        keys[0] = LP_NONE_LO;
        keys[1] = LP_NONE_HI;
    }
}

// (lo, hi) of the pixels that are not NaN into keys[0], keys[1]; four pixels per lane
__global__ void __launch_bounds__(LP_T) log_minmax_kernel(int64_t hw, const float* __restrict__ map, uint32_t* __restrict__ keys) {
    __shared__ uint32_t s_lo[LP_T / 64], s_hi[LP_T / 64];
    const int64_t i = ((int64_t)blockIdx.x * LP_T + threadIdx.x) * PX;
    uint32_t lo = LP_NONE_LO, hi = LP_NONE_HI;
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
    lo = wave_min(lo); hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < LP_T / 64; w++) {
            lo = min(lo, s_lo[w]);
            hi = max(hi, s_hi[w]);
        }
        if (lo != LP_NONE_LO) atomicMin(&keys[0], lo);      // (a workgroup of NaNs has nothing to add)
        if (hi != LP_NONE_HI) atomicMax(&keys[1], hi);
    }
}

// numpy's (x * 255).clip(0, 255).astype(uint8), NaN -> 0
__device__ __forceinline__ uint32_t log_quantize(float x) {
    const float y = __fmul_rn(x, 255.0f);
    return y >= 255.0f ? 255u : (y > 0.0f ? (uint32_t)(int)y : 0u);
}

// matplotlib's bin of a normalised value: min(int(t * 256), 255), below the range and NaN entry 0
__device__ __forceinline__ int log_bin(float t) {
    const float s = __fmul_rn(t, 256.0f);
    return s >= 255.0f ? 255 : (s > 0.0f ? (int)s : 0);
}

// the three little-endian words of four interleaved RGB pixels c[j] = r | g << 8 | b << 16
__device__ __forceinline__ void log_store4(uint8_t* __restrict__ dst, int64_t i, int64_t hw, const uint32_t (&c)[PX]) {
    const uint32_t w[3] = {c[0] | c[1] << 24, c[1] >> 8 | c[2] << 16, c[2] >> 16 | c[3] << 8};
    store_bytes<3>(dst + i * 3, (int)min((int64_t)PX, hw - i) * 3, w);
}

// RGB, GRAY, NORMAL: no table, no extrema
template <int MODE>
__global__ void __launch_bounds__(LP_T) log_quantize_kernel(int64_t hw, const float* __restrict__ planes, uint8_t* __restrict__ dst) {
    const int64_t i = ((int64_t)blockIdx.x * LP_T + threadIdx.x) * PX;
    if (i >= hw) return;
    uint32_t c[PX] = {0u, 0u, 0u, 0u};
    constexpr int NC = MODE == SURFEL_LOG_PANEL_GRAY ? 1 : 3;
#pragma unroll
    for (int ch = 0; ch < NC; ch++) {
        float v[PX];
        load4(planes + ch * hw, i, hw, v);
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const float x = MODE == SURFEL_LOG_PANEL_NORMAL ? __fadd_rn(__fmul_rn(v[j], 0.5f), 0.5f) : v[j];
            const uint32_t b = log_quantize(x);
            c[j] |= NC == 1 ? b * 0x010101u : b << (8 * ch);
        }
    }
    log_store4(dst, i, hw, c);
}

// TURBO_MAX, JET_MINMAX: the table sits in LDS (one read per pixel at a data-dependent index)
template <int MODE>
__global__ void __launch_bounds__(LP_T) log_colour_kernel(int64_t hw, const float* __restrict__ map, const uint32_t* __restrict__ keys,
                                                          uint8_t* __restrict__ dst) {
    __shared__ uint32_t s_tab[256];
    static_assert(LP_T == 256, "one table entry per thread");
    s_tab[threadIdx.x] = MODE == SURFEL_LOG_PANEL_TURBO_MAX ? VIS_TURBO[threadIdx.x] : LOG_JET[threadIdx.x];
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * LP_T + threadIdx.x) * PX;
    if (i >= hw) return;
    const float lo = order_value(keys[0]), hi = order_value(keys[1]);      // (NaN, NaN) when no pixel had a value
    bool flat;      // the degenerate cases of surfel_log.h: every pixel is entry 0
    float sub, den;
    if (MODE == SURFEL_LOG_PANEL_TURBO_MAX) {
        flat = !(hi > 0.0f) || isinf(hi);
        sub = 0.0f;
        den = hi;
    } else {
        flat = !(hi > lo) || isinf(hi) || isinf(lo);
        sub = lo;
        den = __fsub_rn(hi, lo);
    }
    float v[PX];
    load4(map, i, hw, v);
    uint32_t c[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const float num = MODE == SURFEL_LOG_PANEL_TURBO_MAX ? v[j] : __fsub_rn(v[j], sub);
        c[j] = s_tab[flat ? 0 : log_bin(__fdiv_rn(num, den))];
    }
    log_store4(dst, i, hw, c);
}

namespace {
constexpr int LOG_MAX_EDGE = 65536;
inline unsigned log_blocks(int64_t hw) { return blocks_for(hw, (int64_t)LP_T * PX); }
}  // namespace

}  // namespace surfel

using namespace surfel;

extern "C" {

int surfel_log_append(void* state, void* ring, int capacity, int iteration, int points, const float* scalars6, float lambda_normal,
                      float lambda_dist, void* stream) {
    if (!state || !ring || !scalars6 || capacity < 1 || (reinterpret_cast<uintptr_t>(state) & 7) || (reinterpret_cast<uintptr_t>(ring) & 3) ||
        (reinterpret_cast<uintptr_t>(scalars6) & 3))
        return api_fail(SURFEL_E_INVALID, "log_append: bad arguments");
    hipLaunchKernelGGL(log_append_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<LogState*>(state),
                       static_cast<LogRecord*>(ring), capacity, iteration, points, scalars6, lambda_normal, lambda_dist);
    return launched("log_append kernel");
}

int surfel_log_panel(int mode, int H, int W, const float* planes, uint8_t* dst, void* scratch, int64_t scratch_bytes, void* stream) {
    if (mode < SURFEL_LOG_PANEL_RGB || mode > SURFEL_LOG_PANEL_JET_MINMAX || H <= 0 || W <= 0 || !planes || !dst || !scratch ||
        (reinterpret_cast<uintptr_t>(planes) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 3))
        return api_fail(SURFEL_E_INVALID, "log_panel: bad arguments");
    if (H > LOG_MAX_EDGE || W > LOG_MAX_EDGE) return api_fail(SURFEL_E_LIMIT, "log_panel: an image edge exceeds 65536");
    if (scratch_bytes < SURFEL_LOG_PANEL_SCRATCH_BYTES) return api_fail(SURFEL_E_INVALID, "log_panel: scratch holds fewer than SURFEL_LOG_PANEL_SCRATCH_BYTES");
    const int64_t hw = (int64_t)H * W;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(log_blocks(hw)), block(LP_T);
    uint32_t* keys = static_cast<uint32_t*>(scratch);
    switch (mode) {
        case SURFEL_LOG_PANEL_RGB: hipLaunchKernelGGL(log_quantize_kernel<SURFEL_LOG_PANEL_RGB>, grid, block, 0, s, hw, planes, dst); break;
        case SURFEL_LOG_PANEL_GRAY: hipLaunchKernelGGL(log_quantize_kernel<SURFEL_LOG_PANEL_GRAY>, grid, block, 0, s, hw, planes, dst); break;
        case SURFEL_LOG_PANEL_NORMAL: hipLaunchKernelGGL(log_quantize_kernel<SURFEL_LOG_PANEL_NORMAL>, grid, block, 0, s, hw, planes, dst); break;
        default:
            hipLaunchKernelGGL(log_reset_kernel, dim3(1), dim3(64), 0, s, keys);
            hipLaunchKernelGGL(log_minmax_kernel, grid, block, 0, s, hw, planes, keys);
            if (mode == SURFEL_LOG_PANEL_TURBO_MAX)
                hipLaunchKernelGGL(log_colour_kernel<SURFEL_LOG_PANEL_TURBO_MAX>, grid, block, 0, s, hw, planes, keys, dst);
            else
                hipLaunchKernelGGL(log_colour_kernel<SURFEL_LOG_PANEL_JET_MINMAX>, grid, block, 0, s, hw, planes, keys, dst);
    }
    return launched("log_panel kernels");
}

}  // extern "C"
