// surfel_select.hip — label pass: per-surfel, per-label sums of the blend weights of one rendered view (gfx950).  SELECT.md states the
// definitions and the layout; include/surfel_select.h the interface.  No interface of the reference is replaced: the reference has no
// segmentation.  The sums are FlashSplat's votes: the optimal label of a surfel under linear blending is the arg-max over labels.
#include "surfel_select_kernel.h"
#include "surfel_tile_walk.h"

namespace surfel {

// ---------------------------------------------------------------------------------------------
// select: the walk of surfel_tile_walk.h, as contrib_kernel (surfel_contrib.hip) runs it, with the weight w = alpha * T of every
// composited pair routed by the pixel's label:
//   * LDS holds one 32-bit counter per (staged instance, label), s_votes[instance * STRIDE + label] with STRIDE = KB + 1 (odd);
//   * a row whose live pixels share one label (decided once per thread, before the walk) reduces its weights over the row and lane 15
//     adds the sum to (instance, that label): the contribution pass's path.  A row with mixed labels adds per lane — the lanes share
//     the instance and differ in label, so their counters lie in different banks (label < 32 = the bank modulus of a 32-bit LDS
//     access) or at one address;
//   * behind a batch's walk, thread t flushes the K counters of instance t (addresses t * STRIDE + k: with an odd stride the 32 lanes
//     of a half-wave read 32 different banks) with one global atomicAdd per non-zero counter.
// A pixel whose label is >= K votes for nothing: it is finished from the start.  Integer accumulators combined by addition only: the
// same bytes on every run, for every order of tiles and of views.
// ---------------------------------------------------------------------------------------------
template <int KB, bool STATS>
__global__ void __launch_bounds__(BLOCK) select_kernel(SelectArgs a) {
    constexpr int STRIDE = KB + 1;      // odd: see the header comment
    __shared__ WalkLds lds;
    __shared__ uint32_t s_votes[BLOCK * STRIDE];                              // [staged instance][label]: sum of rint(w 2^24)

    WalkPixel px;
    if (!walk_pixel(a.frame, px)) return;
    const int lane = threadIdx.x & 63;
    const int K = a.K;

    // the pixel's label: one byte, read only inside the frame (the image ends with its last pixel)
    int lab = 0;
    bool live = false;
    if (px.inside) {
        const int l = (int)a.labels[(size_t)px.pyi * a.frame.W + px.pxi];
        if (l < K) { lab = l; live = true; }
    }
    bool done = !live;
    if (__syncthreads_count(done) == BLOCK) return;      // nothing of this tile votes
    // the row's label: that of its first live lane; the row is uniform when every live lane holds it
    const int rshift = lane & 48;
    const unsigned lv = (unsigned)(__ballot(live) >> rshift) & 0xffffu;
    const int row_lab = __shfl(lab, rshift + __builtin_ctz(lv | 0x10000u), 64);      // (a row without a live lane never adds)
    const unsigned mixed = (unsigned)(__ballot(live && lab != row_lab) >> rshift) & 0xffffu;
    const bool uni = mixed == 0u;
    const int slot = uni ? row_lab : lab;                  // < K <= KB on every lane
    const bool adder = uni ? (lane & 15) == 15 : true;     // who adds: lane 15 the row's sum | every lane its own weight

    unsigned natomics = 0;   // STATS: global atomics this thread issued
#pragma unroll
    for (int k = 0; k < STRIDE; k++) s_votes[k * BLOCK + threadIdx.x] = 0u;

    tile_walk(a.frame, px, lds, done,
        [&](int j, int, bool, bool, float w) {
            const uint32_t q = (uint32_t)__builtin_rintf(w * WALK_Q_ONE);      // (0 where the pair was not composited)
            const uint32_t rs = row_sum(q);
            const uint32_t add = uni ? rs : q;
            if (adder && add != 0u) atomicAdd(&s_votes[j * STRIDE + slot], add);
        },
        [&](uint32_t id) {      // (a thread behind the batch's end holds zeros)
            unsigned long long* __restrict__ dst = a.votes + (size_t)id * (size_t)K;
#pragma unroll
            for (int k = 0; k < KB; k++) {
                if (k < K) {
                    const uint32_t v = s_votes[threadIdx.x * STRIDE + k];
                    if (v != 0u) {
                        atomicAdd(&dst[k], (unsigned long long)v);
                        s_votes[threadIdx.x * STRIDE + k] = 0u;
                        if (STATS) natomics++;
                    }
                }
            }
        });
    if (STATS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) natomics += __shfl_xor(natomics, o);
        if (lane == 0 && natomics) atomicAdd(&a.stats[7], (unsigned long long)natomics);
    }
}

template <int KB>
static void launch_bucket(const SelectArgs& a, hipStream_t s) {
    if (a.stats) hipLaunchKernelGGL((select_kernel<KB, true>), dim3(a.frame.map_len), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((select_kernel<KB, false>), dim3(a.frame.map_len), dim3(BLOCK), 0, s, a);
}

// The buckets: the binary case keeps the contribution pass's LDS (3 KB of counters beside the 12 KB of records), K <= 8 takes 9 KB,
// K <= 32 takes 33 KB.
void launch_select(const SelectArgs& a, hipStream_t s) {
    if (a.K <= 2) launch_bucket<2>(a, s);
    else if (a.K <= 8) launch_bucket<8>(a, s);
    else launch_bucket<SELECT_MAX_LABELS>(a, s);
}

}  // namespace surfel
