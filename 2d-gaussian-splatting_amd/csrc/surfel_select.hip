// surfel_select.hip — label pass: per-surfel, per-label sums of the blend weights of one rendered view (gfx950).  SELECT.md states the
// definitions and the layout; include/surfel_select.h the interface.  No interface of the reference is replaced: the reference has no
// segmentation.  The sums are FlashSplat's votes: the optimal label of a surfel under linear blending is the arg-max over labels.
#include "surfel_common.h"
#include "surfel_select_kernel.h"

namespace surfel {

// ---------------------------------------------------------------------------------------------
// select: the walk of contrib_kernel (surfel_contrib.hip), which is the walk of blend_fwd_kernel — one workgroup per 16x16 tile, 256
// instances staged per batch, one DPP row of 16 lanes per 4x4 sub-tile, the same pair_hit, T recurrence and termination rule — with
// the weight w = alpha * T of every composited pair routed by the pixel's label:
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
constexpr int SW = 8;             // 32-bit mask words per staged batch of 256
constexpr int SSTRIDE = SW + 2;   // + zero sentinel word, padded so each sub-tile's words start 8-B aligned
constexpr float SELECT_Q_ONE = 16777216.f;      // 2^24: votes count weights in units of 2^-24

// A tile's 256 pixels add at most 256 * rint(0.99 * 2^24) = 4 252 017 664 < 2^32 to one (staged instance, label): 32-bit LDS sums cannot wrap.
static_assert(256ull * 16609444ull < (1ull << 32), "the per-tile weight sum of one (instance, label) fits 32 bits");

// lane 15 of every DPP row <- the row's sum (Hillis-Steele over row_shr 1, 2, 4, 8; lanes shifted in from outside a row read 0)
__device__ __forceinline__ uint32_t select_row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    return v;
}

template <int KB, bool STATS>
__global__ void __launch_bounds__(BLOCK) select_kernel(SelectArgs a) {
    constexpr int STRIDE = KB + 1;      // odd: see the header comment
    __shared__ float4 s_rec[BLOCK * 3];                                       // q0-q2 of the staged records: all a weight needs
    __shared__ __attribute__((aligned(8))) uint32_t s_mask[16 * SSTRIDE];     // [sub-tile][word]
    __shared__ uint32_t s_votes[BLOCK * STRIDE];                              // [staged instance][label]: sum of rint(w 2^24)

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
    const uint32_t* mrow = &s_mask[sub * SSTRIDE];
    const int K = a.K;

    // the pixel's label: one byte, read only inside the frame (the image ends with its last pixel)
    int lab = 0;
    bool live = false;
    if (inside) {
        const int l = (int)a.labels[(size_t)pyi * a.W + pxi];
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

    float T = 1.f;
    unsigned natomics = 0;   // STATS: global atomics this thread issued
    if (threadIdx.x < 16) s_mask[threadIdx.x * SSTRIDE + SW] = 0u;     // sentinel
#pragma unroll
    for (int k = 0; k < STRIDE; k++) s_votes[k * BLOCK + threadIdx.x] = 0u;

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
            if (lane == 0) *reinterpret_cast<unsigned long long*>(&s_mask[s * SSTRIDE + 2 * wave]) = b;
        }
        __syncthreads();
        const int nw = (m + 31) >> 5;                 // mask words in use
        int widx = 0;
        uint32_t cur = mrow[0], next = mrow[1];
        {   // a row whose 16 pixels are all finished skips the batch
            const unsigned long long db = __ballot(done);
            if ((((unsigned)(db >> rshift)) & 0xffffu) == 0xffffu) { cur = 0u; widx = nw; }
        }
        for (;;) {
            if (!__any((cur != 0u) | (widx < nw - 1))) break;
            const bool act = cur != 0u;
            const int j = (widx << 5) + __builtin_ctz(cur | 0x80000000u);      // <= 255 where act (uniform over the row: its lanes share the mask); only read from otherwise
            cur &= cur - 1u;
            const float4 q0 = s_rec[j * 3 + 0], q1 = s_rec[j * 3 + 1], q2 = s_rec[j * 3 + 2];
            Hit h;
            const bool hit = pair_hit(pxf, pyf, q0, q1, q2, h);
            const float alpha = h.alpha;
            const bool ok = act & (!done) & hit;
            if (__any(ok)) {
                uint32_t q = 0u;
                if (ok) {
                    const float testT = T * (1.f - alpha);
                    if (testT < T_EPS) done = true;       // the terminating surfel is not composited
                    else {
                        const float w = alpha * T;
                        q = (uint32_t)__builtin_rintf(w * SELECT_Q_ONE);
                        T = testT;
                    }
                }
                const uint32_t rs = select_row_sum(q);
                const uint32_t add = uni ? rs : q;
                if (adder && add != 0u) atomicAdd(&s_votes[j * STRIDE + slot], add);
                if (__all(done)) break;
            }
            if (cur == 0u && widx < nw - 1) { widx++; cur = next; next = mrow[widx + 1]; }
        }
        __syncthreads();      // every row has left the batch: the counters are final
        {   // flush: thread t holds the surfel id of staged instance t (a thread behind the batch's end holds zeros)
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
        }
        // (also the barrier that frees the records, the masks and the counters for the next batch)
        if (__syncthreads_count(done) == BLOCK) break;
    }
    if (STATS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) natomics += __shfl_xor(natomics, o);
        if (lane == 0 && natomics) atomicAdd(&a.stats[7], (unsigned long long)natomics);
    }
}

template <int KB>
static void launch_bucket(const SelectArgs& a, hipStream_t s) {
    if (a.stats) hipLaunchKernelGGL((select_kernel<KB, true>), dim3(a.map_len), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((select_kernel<KB, false>), dim3(a.map_len), dim3(BLOCK), 0, s, a);
}

// The buckets: the binary case keeps the contribution pass's LDS (3 KB of counters beside the 12 KB of records), K <= 8 takes 9 KB,
// K <= 32 takes 33 KB.
void launch_select(const SelectArgs& a, hipStream_t s) {
    if (a.K <= 2) launch_bucket<2>(a, s);
    else if (a.K <= 8) launch_bucket<8>(a, s);
    else launch_bucket<SELECT_MAX_LABELS>(a, s);
}

}  // namespace surfel
