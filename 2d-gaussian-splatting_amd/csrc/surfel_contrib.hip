// surfel_contrib.hip — contribution pass: per-surfel blend-weight statistics of one rendered view (gfx950).  CONTRIB.md states the
// definitions; include/surfel_contrib.h the interface.  No interface of the reference is replaced: the reference prunes by opacity and
// screen size only (scene/gaussian_model.py).
#include "surfel_contrib_kernel.h"
#include "surfel_tile_walk.h"

namespace surfel {

// ---------------------------------------------------------------------------------------------
// contrib: one workgroup (4 waves) per 16x16 tile on the walk of surfel_tile_walk.h, which composites the forward's pairs, pair for
// pair.  No image is written.  What is kept instead, for every composited pair, is w = alpha * T:
//   * the 16 lanes of a row visit ONE staged instance: their weights are reduced over the row (DPP row_shr scan, lane 15 holds the
//     row's value) and lane 15 adds them to LDS accumulators indexed by staged instance (ds_add_u32 / ds_max_u32: 16 rows, 4 waves);
//   * behind a batch's walk, thread t — which staged instance t and still holds its surfel id — flushes instance t with one set of
//     global integer atomics, if any pixel of the tile touched it.
// Every accumulator is an integer combined by a commutative, associative operation: the same bytes on every run, for every order of
// tiles and of views.
// ---------------------------------------------------------------------------------------------
template <bool STATS>
__global__ void __launch_bounds__(BLOCK) contrib_kernel(ContribArgs a) {
    __shared__ WalkLds lds;
    __shared__ uint32_t s_sum[BLOCK], s_max[BLOCK], s_cnt[BLOCK];             // per staged instance: sum of rint(w 2^24) | max of w's bits | pixels that
                                                                              // touched it (composited or terminated) << 16 | pixels that composited it
    WalkPixel px;
    if (!walk_pixel(a.frame, px)) return;
    const int lane = threadIdx.x & 63;

    bool done = !px.inside;
    float best_w = 0.f;      // the pixel's heaviest composited weight so far, and its list position (a tie keeps the nearer surfel)
    int best_pos = -1;
    unsigned natomics = 0;   // STATS: global atomics this thread issued
    s_sum[threadIdx.x] = 0u; s_max[threadIdx.x] = 0u; s_cnt[threadIdx.x] = 0u;

    tile_walk(a.frame, px, lds, done,
        [&](int j, int pos, bool ok, bool composited, float w) {
            // (w is 0 where the pair was not composited: it adds nothing and is never the heaviest)
            uint32_t q = (uint32_t)__builtin_rintf(w * WALK_Q_ONE), bits = __float_as_uint(w);
            uint32_t cnt = (ok ? 1u << 16 : 0u) | (composited ? 1u : 0u);      // touched: composited, or terminated by it
            if (w > best_w) { best_w = w; best_pos = pos; }
            q = row_sum(q); bits = row_max(bits); cnt = row_sum(cnt);
            if ((lane & 15) == 15 && cnt != 0u) {
                atomicAdd(&s_cnt[j], cnt);
                if (cnt & 0xffffu) { atomicAdd(&s_sum[j], q); atomicMax(&s_max[j], bits); }
            }
        },
        [&](uint32_t id) {
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
        });
    // the pixel's dominant surfel.  The 16 pixels of a row often share it: the first lane of every group of equal ids adds the group's size
    int dom = -1;
    if (best_pos >= 0) dom = (int)a.frame.point_list[px.range.x + best_pos];
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
    if (px.inside && a.dominant_id) a.dominant_id[(size_t)px.pyi * a.frame.W + px.pxi] = dom;
    if (STATS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) natomics += __shfl_xor(natomics, o);
        if (lane == 0) atomicAdd(&a.stats[7], (unsigned long long)natomics);
    }
}

void launch_contrib(const ContribArgs& a, hipStream_t s) {
    if (a.stats) hipLaunchKernelGGL(contrib_kernel<true>, dim3(a.frame.map_len), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL(contrib_kernel<false>, dim3(a.frame.map_len), dim3(BLOCK), 0, s, a);
}

}  // namespace surfel
