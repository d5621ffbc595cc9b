// surfel_tile_walk.h — the batch-synchronous tile walk of the passes that run behind a forward: the contribution pass
// (surfel_contrib.hip) and the label pass (surfel_select.hip).  It is the walk of blend_fwd_kernel (surfel_forward.hip) — one workgroup
// (4 waves) per 16x16 tile, 256 instances staged per batch, one DPP row of 16 lanes per 4x4 sub-tile walking its own bitmask, the same
// pair_hit, the same T recurrence and the same termination rule — so the pairs it composites are the forward's, pair for pair.  A pass
// supplies what is kept of a pair (visit) and where a batch's sums go (flush); CONTRIB.md states the contract.
#pragma once
#include "surfel_common.h"

namespace surfel {

// what a forward left behind, as both argument blocks carry it
struct WalkFrame {
    int W, H, gx, gy;
    const uint2* ranges; const uint32_t* point_list; const float* rec;      // the forward's tile lists and surfel records
    const int* tile_map; const uint32_t* map_flag; int map_len;             // as BlendFwdArgs: the forward's tile order, the grid size
};

constexpr int WALK_W = 8;                    // 32-bit mask words per staged batch of 256
constexpr int WALK_STRIDE = WALK_W + 2;      // + zero sentinel word, padded so each sub-tile's words start 8-B aligned
constexpr float WALK_Q_ONE = 16777216.f;     // 2^24: the passes sum weights in units of 2^-24

// A tile's 256 pixels add at most 256 * rint(0.99 * 2^24) = 4 252 017 664 < 2^32 to one staged instance: 32-bit LDS sums cannot wrap.
static_assert(256ull * 16609444ull < (1ull << 32), "the per-tile weight sum of one instance fits 32 bits");

// The masks come first, and the alignment puts the block in front of a pass's own LDS arrays (the compiler lays LDS out by alignment,
// then size): the masks then start at LDS address 0 and the 16 ballot stores address them by immediate offsets.  Elsewhere the
// compiler keeps 16 addresses in registers across the batch loop (tests/test_kernel_resources_cpu.py watches the count).
struct __attribute__((aligned(128))) WalkLds {
    uint32_t mask[16 * WALK_STRIDE];      // [sub-tile][word]
    float4 rec[BLOCK * 3];                // q0-q2 of the staged records: all a weight needs
};
static_assert(sizeof(WalkLds) == 16 * WALK_STRIDE * 4 + BLOCK * 48, "no padding: the passes keep their LDS size");
static_assert(WALK_STRIDE % 2 == 0, "a wave's 64-bit ballot lands 8-B aligned in every sub-tile's row");

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

// a thread's tile and pixel
struct WalkPixel {
    int tx, ty, sub;      // the tile, and the thread's 4x4 sub-tile = its DPP row (thread_pixel)
    int pxi, pyi;
    bool inside;          // of the frame
    uint2 range;          // the tile's list in point_list
    int n;                // ... and its length
};

// false: the workgroup has no tile (the grid covers the map's length)
__device__ __forceinline__ bool walk_pixel(const WalkFrame& f, WalkPixel& p) {
    const int tile = block_tile(f.tile_map, f.map_flag, blockIdx.x, f.gx * f.gy);
    if (tile < 0) return false;
    p.tx = tile % f.gx; p.ty = tile / f.gx;
    int lx, ly;
    thread_pixel(threadIdx.x, lx, ly, p.sub);
    p.pxi = p.tx * TILE + lx; p.pyi = p.ty * TILE + ly;
    p.inside = p.pxi < f.W && p.pyi < f.H;
    p.range = f.ranges[tile];
    p.n = (int)(p.range.y - p.range.x);
    return true;
}

// The walk of one tile's list, called by all 256 threads.  done: the pixel takes no pairs (outside the frame, or of no interest to
// the pass); the walk's own copy, by value so that it stays a lane mask, is set when the pixel saturates.
//   visit(j, pos, ok, composited, w)   inside `if (__any(ok))`, for staged instance j (uniform over a DPP row) = list position pos.
//                                      ok: the pixel hits it and was not done; composited: ... and it did not terminate the pixel;
//                                      w = alpha * T where composited, 0 elsewhere.
//   flush(id)                          by every thread, once per batch, behind the barrier that follows the batch's walk: the LDS a
//                                      visit wrote is final.  id: the surfel of staged instance threadIdx.x (0 behind the batch's end).
//                                      The barrier behind it frees the records, the masks and the pass's own LDS for the next batch.
template <class Visit, class Flush>
__device__ __forceinline__ void tile_walk(const WalkFrame& f, const WalkPixel& p, WalkLds& lds, bool done, Visit visit, Flush flush) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float pxf = (float)p.pxi, pyf = (float)p.pyi;
    const uint2 range = p.range;
    const int n = p.n, tx = p.tx, ty = p.ty;
    const uint32_t* mrow = &lds.mask[p.sub * WALK_STRIDE];
    float T = 1.f;
    if (threadIdx.x < 16) lds.mask[threadIdx.x * WALK_STRIDE + WALK_W] = 0u;     // sentinel

    for (int base = 0; base < n; base += BLOCK) {
        const int m = min(BLOCK, n - base);
        unsigned ov = 0;
        uint32_t id = 0;
        if ((int)threadIdx.x < m) {
            id = f.point_list[range.x + base + threadIdx.x];
            const float4* __restrict__ src = reinterpret_cast<const float4*>(f.rec + (size_t)id * REC_F);
            const float4 v0 = src[0], v1 = src[1], v2 = src[2], v5 = src[5], v6 = src[6];
            lds.rec[threadIdx.x * 3 + 0] = v0; lds.rec[threadIdx.x * 3 + 1] = v1; lds.rec[threadIdx.x * 3 + 2] = v2;
            ov = subtile_overlap(make_foot(v2, v5, v6), tx * TILE, ty * TILE);
        }
        // per-sub-tile bitmasks of the 64 instances this staging wave holds (words 2*wave, 2*wave+1)
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const unsigned long long b = __ballot((ov >> s) & 1u);
            // (the compiler stores the two dwords with one ds_write2_b32; told of the 8-B alignment it stores a b64, and the label
            // pass's binary bucket measured 1 - 2 % slower on the garden frame: SELECT.md)
            if (lane == 0) *reinterpret_cast<unsigned long long*>(&lds.mask[s * WALK_STRIDE + 2 * wave]) = b;
        }
        __syncthreads();
        const int nw = (m + 31) >> 5;                 // mask words in use
        int widx = 0;
        uint32_t cur = mrow[0], next = mrow[1];
        {   // a row whose 16 pixels are all done skips the batch
            const unsigned long long db = __ballot(done);
            if ((((unsigned)(db >> (lane & 48))) & 0xffffu) == 0xffffu) { cur = 0u; widx = nw; }
        }
        for (;;) {
            if (!__any((cur != 0u) | (widx < nw - 1))) break;
            const bool act = cur != 0u;
            const int j = (widx << 5) + __builtin_ctz(cur | 0x80000000u);      // <= 255 where act (uniform over the row: its lanes share the mask); only read from otherwise
            cur &= cur - 1u;
            const float4 q0 = lds.rec[j * 3 + 0], q1 = lds.rec[j * 3 + 1], q2 = lds.rec[j * 3 + 2];
            Hit h;
            const bool hit = pair_hit(pxf, pyf, q0, q1, q2, h);
            const float alpha = h.alpha;
            const bool ok = act & (!done) & hit;
            if (__any(ok)) {
                bool composited = false;
                float w = 0.f;
                if (ok) {
                    const float testT = T * (1.f - alpha);
                    if (testT < T_EPS) done = true;       // the terminating surfel is not composited
                    else {
                        w = alpha * T;
                        composited = true;
                        T = testT;
                    }
                }
                visit(j, base + j, ok, composited, w);
                if (__all(done)) break;
            }
            if (cur == 0u && widx < nw - 1) { widx++; cur = next; next = mrow[widx + 1]; }
        }
        __syncthreads();      // every row has left the batch: what the visits accumulated is final
        flush(id);
        // (also the barrier that frees the records, the masks and the pass's accumulators for the next batch)
        if (__syncthreads_count(done) == BLOCK) break;
    }
}

}  // namespace surfel
