// frame_vis.hip — the frame kernels of the trajectory renderer (include/surfel_vis.h, RENDER.md): fp32 planes -> interleaved 8-bit
// pixels, exact order statistics of a frame (what np.percentile selects), and the turbo-coloured log-depth frame.
// Compiled without contraction (build.py): v * scale + bias rounds twice, like its numpy restatement (tests/path_oracle.py).
// The two conversion kernels move every byte once; the selection reads the frame four times and keeps its counters in LDS.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_vis.h"
#include "side_util.h"
#include "vis_pixels.h"
#include "vis_turbo_table.h"

namespace surfel {

constexpr int VT = 256;      // threads per workgroup
constexpr int NR = SURFEL_VIS_MAX_RANKS;

template <int C>
__global__ void __launch_bounds__(VT) vis_quantize_kernel(int64_t hw, const float* __restrict__ planes, float scale, float bias, uint8_t* __restrict__ dst) {
    const int64_t i = ((int64_t)blockIdx.x * VT + threadIdx.x) * PX;
    if (i >= hw) return;
    uint32_t q[C][PX];
#pragma unroll
    for (int c = 0; c < C; c++) {
        float v[PX];
        load4(planes + c * hw, i, hw, v);
#pragma unroll
        for (int j = 0; j < PX; j++) q[c][j] = quant8(v[j], scale, bias);
    }
    uint32_t w[C];
    if (C == 1) {
        w[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[0][3] << 24;
    } else {      // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        w[0] = q[0][0] | q[1][0] << 8 | q[2][0] << 16 | q[0][1] << 24;
        w[1] = q[1][1] | q[2][1] << 8 | q[0][2] << 16 | q[1][2] << 24;
        w[2] = q[2][2] | q[0][3] << 8 | q[1][3] << 16 | q[2][3] << 24;
    }
    store_bytes<C>(dst + i * C, (int)min((int64_t)PX, hw - i) * C, w);
}

// depth frame of create_videos: the table sits in LDS (one read per pixel at a data-dependent index)
__global__ void __launch_bounds__(VT) vis_depth_turbo_kernel(int64_t hw, const float* __restrict__ depth, double base, double range, uint8_t* __restrict__ dst) {
    __shared__ uint32_t s_tab[256];
    static_assert(VT == 256, "one table entry per thread");
    s_tab[threadIdx.x] = VIS_TURBO[threadIdx.x];
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * VT + threadIdx.x) * PX;
    if (i >= hw) return;
    float v[PX];
    load4(depth, i, hw, v);
    uint32_t c[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const float x = logf(v[j]);
        double t = ((double)x - base) / range;
        c[j] = 0u;                              // a NaN t: matplotlib's `bad` colour, (0, 0, 0)
        if (t == t) {
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            const int k = (int)(t * 256.0);
            c[j] = s_tab[k > 255 ? 255 : k];
        }
    }
    const uint32_t w[3] = {c[0] | c[1] << 24, c[1] >> 8 | c[2] << 16, c[2] >> 16 | c[3] << 8};
    store_bytes<3>(dst + i * 3, (int)min((int64_t)PX, hw - i) * 3, w);
}

// ---- order statistics ------------------------------------------------------------------------------------------------------------------
// selection state behind the histograms in the caller's scratch.  prefix[j]: the key bytes of rank j decided so far; rank[j]: its rank
// among the elements that share them.  Ranks whose prefixes are equal (neighbouring order statistics, mostly) share one histogram:
// slot[j] indexes uprefix[0 .. nuniq).
struct OrderState {
    uint32_t prefix[NR], rank[NR], slot[NR], uprefix[NR], nuniq, pad[31];
};
struct OrderRanks {
    uint32_t r[NR];
};
static_assert(SURFEL_VIS_ORDER_SCRATCH_BYTES == NR * 256 * 4 + sizeof(OrderState), "scratch layout");

__global__ void __launch_bounds__(VT) vis_order_init_kernel(uint32_t* __restrict__ hist, OrderState* __restrict__ st, OrderRanks ranks, int m) {
    const int t = threadIdx.x;
#pragma unroll
    for (int u = 0; u < NR; u++) hist[u * 256 + t] = 0u;
    if (t < NR) {
        st->prefix[t] = 0u;
        st->rank[t] = t < m ? ranks.r[t] : 0u;
        st->slot[t] = 0u;
        st->uprefix[t] = 0u;
    }
    if (t == 0) st->nuniq = 1u;
}

// one element into the LDS counters; called by all 64 lanes of a wave together (valid = this lane holds an element).  The lanes that
// agree with the first counting lane's digit are counted by that lane in one add: depth frames put most of a wave into one bin of
// the leading bytes, and 64 adds to one LDS address would serialise.
__device__ __forceinline__ void order_count(uint32_t* s_h, const uint32_t* s_up, int nu, int shift, uint32_t key, bool valid) {
    const int lane = threadIdx.x & 63;
    const uint32_t hi = shift == 24 ? 0u : key >> (shift + 8);
    const int d = (int)((key >> shift) & 255u);
    for (int u = 0; u < nu; u++) {
        const bool mine = valid && hi == s_up[u];
        const unsigned long long any = __ballot(mine);
        if (any == 0ull) continue;
        const int leader = __ffsll(any) - 1;
        const int d0 = __shfl(d, leader);
        const bool same = mine && d == d0;
        const unsigned long long group = __ballot(same);
        if (lane == leader)
            atomicAdd(&s_h[u * 256 + d0], (uint32_t)__popcll(group));
        else if (mine && !same)
            atomicAdd(&s_h[u * 256 + d], 1u);
    }
}

__global__ void __launch_bounds__(VT) vis_order_hist_kernel(int64_t n, const float* __restrict__ x, int shift, uint32_t* __restrict__ hist,
                                                            const OrderState* __restrict__ st) {
    __shared__ uint32_t s_h[NR * 256];
    __shared__ uint32_t s_up[NR];
    const int t = threadIdx.x;
    const int nu = min((int)st->nuniq, NR);
    for (int k = t; k < nu * 256; k += VT) s_h[k] = 0u;
    if (t < NR) s_up[t] = st->uprefix[t];
    __syncthreads();
    // x[0 .. head) up to the first 16-byte boundary, then n4 groups of four, then the rest: head + tail < 8 elements
    const int64_t head = min(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2));
    const int64_t n4 = (n - head) >> 2;
    const float4* body = reinterpret_cast<const float4*>(x + head);
    for (int64_t g0 = (int64_t)blockIdx.x * VT; g0 < n4; g0 += (int64_t)gridDim.x * VT) {      // (uniform trip count: every lane stays in)
        const bool valid = g0 + t < n4;
        float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (valid) f = body[g0 + t];
        order_count(s_h, s_up, nu, shift, order_key(f.x), valid);
        order_count(s_h, s_up, nu, shift, order_key(f.y), valid);
        order_count(s_h, s_up, nu, shift, order_key(f.z), valid);
        order_count(s_h, s_up, nu, shift, order_key(f.w), valid);
    }
    if (blockIdx.x == 0 && t < 64) {      // one wave, whole
        const int64_t rest = n - head - 4 * n4;
        int64_t e = -1;
        if (t < head) e = t;
        else if (t - head < rest) e = head + 4 * n4 + (t - head);
        order_count(s_h, s_up, nu, shift, order_key(e >= 0 ? x[e] : 0.0f), e >= 0);
    }
    __syncthreads();
    for (int k = t; k < nu * 256; k += VT) {
        const uint32_t c = s_h[k];
        if (c) atomicAdd(&hist[k], c);
    }
}

// one workgroup: per rank, the bin of its histogram that holds it (inclusive scan over the 256 bins); the histograms are cleared for
// the next pass and the shared slots recomputed.  After the last byte the prefix is the key: out[j] <- its value.
__global__ void __launch_bounds__(VT) vis_order_narrow_kernel(uint32_t* __restrict__ hist, OrderState* __restrict__ st, int m, int last,
                                                              float* __restrict__ out) {
    __shared__ uint32_t s_scan[256];
    __shared__ uint32_t s_prefix[NR], s_rank[NR];
    const int t = threadIdx.x;
    if (t < NR) {      // (a rank behind the last element cannot occur: checked on the host)
        s_prefix[t] = (st->prefix[t] << 8) | 255u;
        s_rank[t] = 0u;
    }
    for (int j = 0; j < m; j++) {
        const uint32_t r = st->rank[j];
        const uint32_t c = hist[st->slot[j] * 256 + t];
        s_scan[t] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t v = t >= off ? s_scan[t - off] : 0u;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        const uint32_t incl = s_scan[t], excl = incl - c;
        if (excl <= r && r < incl) {
            s_prefix[j] = (st->prefix[j] << 8) | (uint32_t)t;
            s_rank[j] = r - excl;
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NR; u++) hist[u * 256 + t] = 0u;
    if (t == 0) {
        uint32_t nu = 0;
        for (int j = 0; j < m; j++) {
            st->prefix[j] = s_prefix[j];
            st->rank[j] = s_rank[j];
            if (j > 0 && s_prefix[j] == s_prefix[j - 1]) {
                st->slot[j] = st->slot[j - 1];
            } else {
                st->uprefix[nu] = s_prefix[j];
                st->slot[j] = nu++;
            }
        }
        st->nuniq = nu;
    }
    if (last && t < m) out[t] = order_value(s_prefix[t]);
}

namespace {

constexpr int VIS_MAX_EDGE = 65536;

inline unsigned pixel_blocks(int64_t hw) { return blocks_for(hw, (int64_t)VT * PX); }

}  // namespace
}  // namespace surfel

using namespace surfel;

extern "C" {

int surfel_vis_quantize(int C, int H, int W, const float* planes, float scale, float bias, uint8_t* dst, void* stream) {
    if ((C != 1 && C != 3) || H <= 0 || W <= 0 || !planes || !dst || (reinterpret_cast<uintptr_t>(planes) & 3))
        return api_fail(SURFEL_E_INVALID, "vis_quantize: bad arguments");
    if (H > VIS_MAX_EDGE || W > VIS_MAX_EDGE) return api_fail(SURFEL_E_LIMIT, "vis_quantize: an image edge exceeds 65536");
    const int64_t hw = (int64_t)H * W;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C == 1) hipLaunchKernelGGL(vis_quantize_kernel<1>, dim3(pixel_blocks(hw)), dim3(VT), 0, s, hw, planes, scale, bias, dst);
    else hipLaunchKernelGGL(vis_quantize_kernel<3>, dim3(pixel_blocks(hw)), dim3(VT), 0, s, hw, planes, scale, bias, dst);
    return launched("vis_quantize_kernel");
}

int surfel_vis_order_stats(int64_t n, const float* x, int m, const int64_t* ranks, float* out, void* scratch, int64_t scratch_bytes,
                           void* stream) {
    if (n <= 0 || !x || m < 1 || m > NR || !ranks || !out || !scratch || (reinterpret_cast<uintptr_t>(x) & 3) ||
        (reinterpret_cast<uintptr_t>(scratch) & 3))
        return api_fail(SURFEL_E_INVALID, "vis_order_stats: bad arguments");
    if (scratch_bytes < SURFEL_VIS_ORDER_SCRATCH_BYTES) return api_fail(SURFEL_E_INVALID, "vis_order_stats: scratch holds fewer than SURFEL_VIS_ORDER_SCRATCH_BYTES");
    if (n > 0xffffffffll) return api_fail(SURFEL_E_LIMIT, "vis_order_stats: more than 2^32 - 1 elements");
    OrderRanks r = {};
    for (int j = 0; j < m; j++) {
        if (ranks[j] < 0 || ranks[j] >= n || (j > 0 && ranks[j] < ranks[j - 1]))
            return api_fail(SURFEL_E_INVALID, "vis_order_stats: ranks must be ascending and in [0, n)");
        r.r[j] = (uint32_t)ranks[j];
    }
    const hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* hist = static_cast<uint32_t*>(scratch);
    OrderState* st = reinterpret_cast<OrderState*>(hist + NR * 256);
    const int64_t groups = (n / 4 + VT - 1) / VT;
    const unsigned blocks = (unsigned)(groups < 1 ? 1 : (groups > 2048 ? 2048 : groups));
    hipLaunchKernelGGL(vis_order_init_kernel, dim3(1), dim3(VT), 0, s, hist, st, r, m);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(vis_order_hist_kernel, dim3(blocks), dim3(VT), 0, s, n, x, shift, hist, st);
        hipLaunchKernelGGL(vis_order_narrow_kernel, dim3(1), dim3(VT), 0, s, hist, st, m, shift == 0 ? 1 : 0, out);
    }
    return launched("vis_order_stats kernels");
}

int surfel_vis_depth_turbo(int H, int W, const float* depth, double lo, double hi, uint8_t* dst, void* stream) {
    if (H <= 0 || W <= 0 || !depth || !dst || (reinterpret_cast<uintptr_t>(depth) & 3)) return api_fail(SURFEL_E_INVALID, "vis_depth_turbo: bad arguments");
    if (H > VIS_MAX_EDGE || W > VIS_MAX_EDGE) return api_fail(SURFEL_E_LIMIT, "vis_depth_turbo: an image edge exceeds 65536");
    const int64_t hw = (int64_t)H * W;
    // (a NaN limit makes the range NaN, and with it every t)
    hipLaunchKernelGGL(vis_depth_turbo_kernel, dim3(pixel_blocks(hw)), dim3(VT), 0, static_cast<hipStream_t>(stream), hw, depth, lo < hi ? lo : hi,
                       fabs(hi - lo), dst);
    return launched("vis_depth_turbo_kernel");
}

}  // extern "C"
