// surfel_contrib.hip — contribution pass: per-surfel blend-weight statistics of one rendered view (gfx950).  CONTRIB.md states the
// definitions; include/surfel_contrib.h the interface.  No interface of the reference is replaced: the reference prunes by opacity and
// screen size only (scene/gaussian_model.py).
#include "surfel_common.h"
#include "surfel_contrib_kernel.h"

namespace surfel {

// ---------------------------------------------------------------------------------------------
// contrib: one workgroup (4 waves) per 16x16 tile, the walk of blend_fwd_kernel (surfel_forward.hip) — 256 instances staged per
// batch, one DPP row of 16 lanes per 4x4 sub-tile walking its own bitmask, the same pair_hit, the same T recurrence and the same
// termination rule — so the composited pairs are the forward's, pair for pair.  No image is written.  What is kept instead, for every
// composited pair, is w = alpha * T:
//   * the 16 lanes of a row visit ONE staged instance: their weights are reduced over the row (DPP row_shr scan, lane 15 holds the
//     row's value) and lane 15 adds them to LDS accumulators indexed by staged instance (ds_add_u32 / ds_max_u32: 16 rows, 4 waves);
//   * behind a batch's walk, thread t — which staged instance t and still holds its surfel id — flushes instance t with one set of
//     global integer atomics, if any pixel of the tile touched it.
// Every accumulator is an integer combined by a commutative, associative operation: the same bytes on every run, for every order of
// tiles and of views.
// ---------------------------------------------------------------------------------------------
constexpr int CW = 8;             // 32-bit mask words per staged batch of 256
constexpr int CSTRIDE = CW + 2;   // + zero sentinel word, padded so each sub-tile's words start 8-B aligned
constexpr float Q_ONE = 16777216.f;      // 2^24: sum_q counts weights in units of 2^-24

// A tile's 256 pixels add at most 256 * rint(0.99 * 2^24) = 4 252 017 664 < 2^32 to one staged instance: 32-bit LDS sums cannot wrap.
static_assert(256ull * 16609444ull < (1ull << 32), "the per-tile weight sum of one instance fits 32 bits");

// lane 15 of every DPP row <- the row's sum / maximum (Hillis-Steele over row_shr 1, 2, 4, 8; lanes shifted in from outside a row read 0)
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    return v;
}
__device__ __forceinline__ uint32_t row_max(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    return v;
}

template <bool STATS>
__global__ void __launch_bounds__(BLOCK) contrib_kernel(ContribArgs a) {
    __shared__ float4 s_rec[BLOCK * 3];                                       // q0-q2 of the staged records: all a weight needs
    __shared__ __attribute__((aligned(8))) uint32_t s_mask[16 * CSTRIDE];     // [sub-tile][word]
    __shared__ uint32_t s_sum[BLOCK], s_max[BLOCK], s_cnt[BLOCK];             // per staged instance: sum of rint(w 2^24) | max of w's bits | pixels that
                                                                              // touched it (composited or terminated) << 16 | pixels that composited it
    const int tile = block_tile(a.tile_map, a.map_flag, blockIdx.x, a.gx * a.gy);
    if (tile < 0) return;
    const int tx = tile % a.gx, ty = tile / a.gx;
    int lx, ly, sub;
    thread_pixel(threadIdx.x, lx, ly, sub);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pxi = tx * TILE + lx, pyi = ty * TILE + ly;
    const bool inside = pxi < a.W && pyi < a.H;
    const float pxf = (float)pxi, pyf = (float)pyi;
    const uint2 range = a.ranges[tile];
    const int n = (int)(range.y - range.x);
    const uint32_t* mrow = &s_mask[sub * CSTRIDE];

    bool done = !inside;
    float T = 1.f;
    float best_w = 0.f;      // the pixel's heaviest composited weight so far, and its list position (a tie keeps the nearer surfel)
    int best_pos = -1;
    unsigned natomics = 0;   // STATS: global atomics this thread issued
    if (threadIdx.x < 16) s_mask[threadIdx.x * CSTRIDE + CW] = 0u;     // sentinel
    s_sum[threadIdx.x] = 0u; s_max[threadIdx.x] = 0u; s_cnt[threadIdx.x] = 0u;

    for (int base = 0; base < n; base += BLOCK) {
        const int m = min(BLOCK, n - base);
        unsigned ov = 0;
        uint32_t id = 0;
        if ((int)threadIdx.x < m) {
            id = a.point_list[range.x + base + threadIdx.x];
            const float4* __restrict__ src = reinterpret_cast<const float4*>(a.rec + (size_t)id * REC_F);
            const float4 v0 = src[0], v1 = src[1], v2 = src[2], v5 = src[5], v6 = src[6];
            s_rec[threadIdx.x * 3 + 0] = v0; s_rec[threadIdx.x * 3 + 1] = v1; s_rec[threadIdx.x * 3 + 2] = v2;
            ov = subtile_overlap(make_foot(v2, v5, v6), tx * TILE, ty * TILE);
        }
        // per-sub-tile bitmasks of the 64 instances this staging wave holds (words 2*wave, 2*wave+1)
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const unsigned long long b = __ballot((ov >> s) & 1u);
            if (lane == 0) *reinterpret_cast<unsigned long long*>(&s_mask[s * CSTRIDE + 2 * wave]) = b;
        }
        __syncthreads();
        const int nw = (m + 31) >> 5;                 // mask words in use
        int widx = 0;
        uint32_t cur = mrow[0], next = mrow[1];
        {   // a row whose 16 pixels are all saturated skips the batch
            const unsigned long long db = __ballot(done);
            if ((((unsigned)(db >> (lane & 48))) & 0xffffu) == 0xffffu) { cur = 0u; widx = nw; }
        }
        for (;;) {
            if (!__any((cur != 0u) | (widx < nw - 1))) break;
            const bool act = cur != 0u;
            const int j = (widx << 5) + __builtin_ctz(cur | 0x80000000u);      // (uniform over the row: its lanes share the mask)
            cur &= cur - 1u;
            const float4 q0 = s_rec[j * 3 + 0], q1 = s_rec[j * 3 + 1], q2 = s_rec[j * 3 + 2];
            Hit h;
            const bool hit = pair_hit(pxf, pyf, q0, q1, q2, h);
            const float alpha = h.alpha;
            const bool ok = act & (!done) & hit;
            if (__any(ok)) {
                uint32_t q = 0u, bits = 0u, cnt = 0u;
                if (ok) {
                    const float testT = T * (1.f - alpha);
                    cnt = 1u << 16;                       // touched: composited, or terminated by it
                    if (testT < T_EPS) done = true;       // the terminating surfel is not composited
                    else {
                        const float w = alpha * T;
                        q = (uint32_t)__builtin_rintf(w * Q_ONE);
                        bits = __float_as_uint(w);
                        cnt |= 1u;
                        if (w > best_w) { best_w = w; best_pos = base + j; }
                        T = testT;
                    }
                }
                q = row_sum(q); bits = row_max(bits); cnt = row_sum(cnt);
                if ((lane & 15) == 15 && cnt != 0u) {
                    atomicAdd(&s_cnt[j], cnt);
                    if (cnt & 0xffffu) { atomicAdd(&s_sum[j], q); atomicMax(&s_max[j], bits); }
                }
                if (__all(done)) break;
            }
            if (cur == 0u && widx < nw - 1) { widx++; cur = next; next = mrow[widx + 1]; }
        }
        __syncthreads();      // every row has left the batch: the accumulators are final
        {   // flush: thread t holds the surfel id of staged instance t
            const uint32_t cnt = s_cnt[threadIdx.x];
            if (cnt != 0u) {
                const uint32_t comp = cnt & 0xffffu;
#ifndef SURFEL_CONTRIB_NO_FLUSH      // diagnostic build (python build.py --variant noflush -DSURFEL_CONTRIB_NO_FLUSH): the walk without its global atomics — timing only, CONTRIB.md
                if (comp) {
                    atomicAdd(&a.sum_q[id], (unsigned long long)s_sum[threadIdx.x]);
                    atomicAdd(&a.hits[id], (unsigned long long)comp);
                    atomicMax(&a.max_bits[id], s_max[threadIdx.x]);
                    if (STATS) natomics += 3;
                }
                const uint32_t old = atomicMax(&a.stamp[id], a.view_tag);
                if (old < a.view_tag) atomicAdd(&a.views[id], 1u);
                if (STATS) natomics += old < a.view_tag ? 2 : 1;
#endif
                if (comp) { s_sum[threadIdx.x] = 0u; s_max[threadIdx.x] = 0u; }
                s_cnt[threadIdx.x] = 0u;
            }
        }
        // (also the barrier that frees the records, the masks and the accumulators for the next batch)
        if (__syncthreads_count(done) == BLOCK) break;
    }
    // the pixel's dominant surfel.  The 16 pixels of a row often share it: the first lane of every group of equal ids adds the group's size
    int dom = -1;
    if (best_pos >= 0) dom = (int)a.point_list[range.x + best_pos];
    {
        unsigned same = 0, first = 1;
        const int l16 = lane & 15;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int other = __shfl(dom, k, 16);
            if (other == dom) { same++; if (k < l16) first = 0; }
        }
#ifndef SURFEL_CONTRIB_NO_FLUSH
        if (dom >= 0 && first) { atomicAdd(&a.dominant[dom], same); if (STATS) natomics++; }
#else
        asm volatile("" :: "v"(same), "v"(first));
#endif
    }
    if (inside && a.dominant_id) a.dominant_id[(size_t)pyi * a.W + pxi] = dom;
    if (STATS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) natomics += __shfl_xor(natomics, o);
        if (lane == 0) atomicAdd(&a.stats[7], (unsigned long long)natomics);
    }
}

void launch_contrib(const ContribArgs& a, hipStream_t s) {
    if (a.stats) hipLaunchKernelGGL(contrib_kernel<true>, dim3(a.map_len), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL(contrib_kernel<false>, dim3(a.map_len), dim3(BLOCK), 0, s, a);
}

}  // namespace surfel
