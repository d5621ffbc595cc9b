// mesh_repair.hip — manifold cut, fan split and hole fill of a triangle mesh (include/surfel_repair.h, REPAIR.md): kept triangles (mesh_topology.h) -> three
// half-edges each -> sort_words (side_util.h) by (min, max) of the ends, so that a run is an undirected edge -> a lane per
// sorted slot looks two slots to either side: the run's length and directions decide the cut, a run of two is a pair of twins -> fans and
// border loops are orbits of a successor array, labelled and ranked by pointer jumping, one launch per round (orbit_round_kernel) -> the
// extra fans of a vertex are ranked by one sort of (vertex, label) -> filled loops are scattered to offset[loop] + position, a workgroup
// per loop gathers its vertices into LDS and one lane per component adds them in order.
// Compiled with -ffp-contract=off (build.py): the centroid's fp64 sum and division round as their numpy restatement
// (tests/repair_oracle.py).  No floating-point atomic; integer atomics only where any order gives the same (min, max, sums).  wave64;
// LDS for the parked terms of a loop; no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_repair.h"
#include "block_ops.h"
#include "mesh_topology.h"

namespace surfel {

constexpr int RT = 256;                                  // threads per workgroup
constexpr int64_t REPAIR_LIMIT = (int64_t)1 << 31;       // 3 F and V + 3 F stay below
constexpr uint32_t HEAD_BIT = 0x80000000u;               // a fan's key: the head of an open fan is below every other half-edge
constexpr uint32_t NONE = 0xFFFFFFFFu;
enum { T_NONMANIFOLD, T_MISORIENTED, T_LONGEST, T_FILLED, T_FILL_TRIS, T_FILL_VERTS, T_FILL_EDGES, T_WORDS };

// the ends of half-edge 3 t + k of the input: lo < hi, fwd when it runs lo -> hi
__device__ __forceinline__ void repair_edge(const int32_t* __restrict__ tris, uint32_t h, uint32_t* lo, uint32_t* hi, bool* fwd) {
    uint32_t a, b;
    half_edge_ends(tris, h, &a, &b);
    *lo = min(a, b); *hi = max(a, b); *fwd = a < b;
}

struct RepairKey {      // the sort's key (lo, hi) of a half-edge: word 0 = hi, word 1 = lo
    const int32_t* tris;
    __device__ uint32_t operator()(uint32_t h, int word) const {
        uint32_t lo, hi; bool fwd;
        repair_edge(tris, h, &lo, &hi, &fwd);
        return word ? lo : hi;
    }
};

// ---- rules 1-3: kept triangles (mesh_topology.h), the sort's keys, the cut ---------------------------------------------------------------
// after the scan of keep: the three half-edges of kept triangle number m at 3 m ..: key = the larger end, value = 3 t + k
__global__ void __launch_bounds__(RT) repair_emit_kernel(int64_t F, RepairKey key_of, const uint32_t* __restrict__ pos,
                                                         const uint32_t* __restrict__ total, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= F || !scanned_flag(pos, total, t, F)) return;
    const int64_t m = pos[t];
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        key[3 * m + k] = key_of(3u * (uint32_t)t + k, 0);
        val[3 * m + k] = 3u * (uint32_t)t + k;
    }
}

// Rule 3 on the sorted half-edges.  Slot j sees the slots up to two away: its run has more than two members iff three neighbouring slots
// that include j agree, two iff exactly one neighbour agrees.  A run is bad when it has more than two members or two of one direction;
// every triangle with a half-edge in a bad run is cut (cut[] is zeroed before; every writer stores 1).  partner[j]: the other slot of a
// good run of two, NONE otherwise.  The run's first slot counts it: tally[T_NONMANIFOLD], tally[T_MISORIENTED].
__global__ void __launch_bounds__(RT) repair_cut_kernel(int64_t n, const int32_t* __restrict__ tris, const uint32_t* __restrict__ order,
                                                        uint32_t* __restrict__ cut, uint32_t* __restrict__ partner, uint32_t* __restrict__ tally) {
    const int64_t j = (int64_t)blockIdx.x * RT + threadIdx.x;
    uint32_t c_many = 0, c_mis = 0;
    if (j < n) {
        uint32_t lo[5], hi[5]; bool fwd[5], same[5];
#pragma unroll
        for (int d = 0; d < 5; d++) {
            const int64_t q = j + d - 2;
            lo[d] = hi[d] = NONE; fwd[d] = false;
            if (q >= 0 && q < n) repair_edge(tris, order[q], &lo[d], &hi[d], &fwd[d]);
        }
#pragma unroll
        for (int d = 0; d < 5; d++) same[d] = lo[d] == lo[2] && hi[d] == hi[2];      // (NONE is no vertex: a missing slot never agrees)
        const bool many = same[0] || (same[1] && same[3]) || same[4];
        const bool two = !many && (same[1] || same[3]);
        const int pd = same[1] ? 1 : 3;
        const bool mis = two && fwd[pd] == fwd[2];
        if (many || mis) cut[order[j] / 3u] = 1u;
        partner[j] = two && !mis ? (uint32_t)(j + pd - 2) : NONE;
        if (!same[1]) { c_many = many ? 1u : 0u; c_mis = mis ? 1u : 0u; }
    }
    c_many = wave_sum(c_many); c_mis = wave_sum(c_mis);
    if ((threadIdx.x & 63) == 0) {
        if (c_many) atomicAdd(&tally[T_NONMANIFOLD], c_many);
        if (c_mis) atomicAdd(&tally[T_MISORIENTED], c_mis);
    }
}

__global__ void __launch_bounds__(RT) repair_survive_kernel(int64_t F, const uint32_t* __restrict__ kpos, const uint32_t* __restrict__ ktotal,
                                                            const uint32_t* __restrict__ cut, uint32_t* __restrict__ surv) {
    const int64_t t = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= F) return;
    surv[t] = scanned_flag(kpos, ktotal, t, F) && !cut[t] ? 1u : 0u;
}

// after the scan of surv: survivor number m keeps its corners (the split rewrites them later) and names its input triangle
__global__ void __launch_bounds__(RT) repair_compact_kernel(int64_t F, const int32_t* __restrict__ tris, const uint32_t* __restrict__ spos,
                                                            const uint32_t* __restrict__ stotal, uint32_t* __restrict__ hsrc,
                                                            int32_t* __restrict__ tsrc) {
    const int64_t t = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= F || !scanned_flag(spos, stotal, t, F)) return;
    const int64_t m = spos[t];
#pragma unroll
    for (int k = 0; k < 3; k++) hsrc[3 * m + k] = (uint32_t)tris[3 * t + k];
    tsrc[m] = (int32_t)t;
}

// twin[h] of the survivors' half-edges h = 3 m + k: the partner of a good run of two when its triangle survived too, NONE otherwise
__global__ void __launch_bounds__(RT) repair_twin_kernel(int64_t n, int64_t F, const uint32_t* __restrict__ order, const uint32_t* __restrict__ partner,
                                                         const uint32_t* __restrict__ spos, const uint32_t* __restrict__ stotal,
                                                         uint32_t* __restrict__ twin) {
    const int64_t j = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (j >= n) return;
    const uint32_t h0 = order[j], t0 = h0 / 3u;
    if (!scanned_flag(spos, stotal, t0, F)) return;
    uint32_t tw = NONE;
    const uint32_t p = partner[j];
    if (p != NONE) {
        const uint32_t h1 = order[p], t1 = h1 / 3u;
        if (scanned_flag(spos, stotal, t1, F)) tw = 3u * spos[t1] + (h1 - 3u * t1);
    }
    twin[3u * spos[t0] + (h0 - 3u * t0)] = tw;
}

// ---- orbits of a successor array --------------------------------------------------------------------------------------------------------
// One round of pointer jumping.  Before round r (step = 2^r) lab[i] is the smallest key among the 2^r elements from i on along the
// successor array, off[i] the distance to its first occurrence and ptr[i] the element 2^r further on (a terminal element points at
// itself).  The round reads one set of arrays and writes the other.  Equal keys keep the nearer occurrence.  *changed becomes 1 when a
// label moved: a round that moves none has seen every orbit whole.  RANK = false leaves the distances out (fans need the label only).
template <bool RANK>
__global__ void __launch_bounds__(RT) orbit_round_kernel(int64_t n, const uint32_t* __restrict__ ptr_in, const uint32_t* __restrict__ lab_in,
                                                         const uint32_t* __restrict__ off_in, uint32_t* __restrict__ ptr_out,
                                                         uint32_t* __restrict__ lab_out, uint32_t* __restrict__ off_out, uint32_t step,
                                                         uint32_t* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    bool take = false;
    if (i < n) {
        const uint32_t p = ptr_in[i], l = lab_in[i], cl = lab_in[p];
        take = cl < l;
        lab_out[i] = take ? cl : l;
        if (RANK) off_out[i] = take ? off_in[p] + step : off_in[i];
        ptr_out[i] = ptr_in[p];
    }
    if (__any(take) && (threadIdx.x & 63) == 0) *changed = 1u;
}

// ---- rule 4: fans -----------------------------------------------------------------------------------------------------------------------
// r(h) = twin(prev(h)); without it h is the head of an open fan: it points at itself and its key is its id without HEAD_BIT
__global__ void __launch_bounds__(RT) repair_fan_init_kernel(int64_t n, const uint32_t* __restrict__ twin, uint32_t* __restrict__ ptr,
                                                             uint32_t* __restrict__ lab) {
    const int64_t h = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (h >= n) return;
    const uint32_t k = (uint32_t)(h % 3), prev = (uint32_t)h - k + (k == 0u ? 2u : k - 1u);
    const uint32_t tp = twin[prev];
    ptr[h] = tp == NONE ? (uint32_t)h : tp;
    lab[h] = tp == NONE ? (uint32_t)h : (uint32_t)h | HEAD_BIT;
}

// fan[h] = the label without the bit; first[u] = the smallest label among the fans of u (first[] holds NONE before)
__global__ void __launch_bounds__(RT) repair_fan_first_kernel(int64_t n, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ hsrc,
                                                              uint32_t* __restrict__ fan, uint32_t* __restrict__ first) {
    const int64_t h = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (h >= n) return;
    const uint32_t f = lab[h] & ~HEAD_BIT;
    fan[h] = f;
    if (f == (uint32_t)h) atomicMin(&first[hsrc[h]], f);
}

// extra[h] = 1 for the label of a fan that does not keep its vertex's index; border[h] = 1 for a half-edge without a twin
__global__ void __launch_bounds__(RT) repair_flags_kernel(int64_t n, const uint32_t* __restrict__ fan, const uint32_t* __restrict__ hsrc,
                                                          const uint32_t* __restrict__ first, const uint32_t* __restrict__ twin,
                                                          uint32_t* __restrict__ extra, uint32_t* __restrict__ border) {
    const int64_t h = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (h >= n) return;
    extra[h] = fan[h] == (uint32_t)h && first[hsrc[h]] != (uint32_t)h ? 1u : 0u;
    border[h] = twin[h] == NONE ? 1u : 0u;
}

// after the scan of extra: the extra fans in ascending label order, key = their vertex
__global__ void __launch_bounds__(RT) repair_extra_emit_kernel(int64_t n, const uint32_t* __restrict__ epos, const uint32_t* __restrict__ etotal,
                                                               const uint32_t* __restrict__ hsrc, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t h = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (h >= n || !scanned_flag(epos, etotal, h, n)) return;
    key[epos[h]] = hsrc[h];
    val[epos[h]] = (uint32_t)h;
}

// after the stable sort by vertex: rank r in ascending (vertex, label) is the new vertex V + r
__global__ void __launch_bounds__(RT) repair_rank_kernel(int64_t S, int64_t V, const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                         uint32_t* __restrict__ new_index, int32_t* __restrict__ split_source) {
    const int64_t r = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (r >= S) return;
    new_index[val[r]] = (uint32_t)(V + r);
    split_source[r] = (int32_t)key[r];
}

__global__ void __launch_bounds__(RT) repair_corner_kernel(int64_t n, const uint32_t* __restrict__ fan, const uint32_t* __restrict__ hsrc,
                                                           const uint32_t* __restrict__ first, const uint32_t* __restrict__ new_index,
                                                           int32_t* __restrict__ corner) {
    const int64_t h = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (h >= n) return;
    const uint32_t u = hsrc[h], f = fan[h];
    corner[h] = (int32_t)(first[u] == f ? u : new_index[f]);
}

// ---- rule 5: loops ----------------------------------------------------------------------------------------------------------------------
// after the scan of border: border half-edge number b, and border_out[its source] = b (one writer per vertex of the split mesh)
__global__ void __launch_bounds__(RT) repair_border_emit_kernel(int64_t n, const uint32_t* __restrict__ bpos, const uint32_t* __restrict__ btotal,
                                                                const int32_t* __restrict__ corner, int32_t* __restrict__ half_edge,
                                                                uint32_t* __restrict__ border_out) {
    const int64_t h = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (h >= n || !scanned_flag(bpos, btotal, h, n)) return;
    half_edge[bpos[h]] = (int32_t)h;
    border_out[corner[h]] = bpos[h];
}

// succ[b] = the border half-edge that leaves b's destination (it exists, REPAIR.md; one that did not would end its path on itself)
__global__ void __launch_bounds__(RT) repair_loop_init_kernel(int64_t nb, const int32_t* __restrict__ half_edge, const int32_t* __restrict__ corner,
                                                              const uint32_t* __restrict__ border_out, uint32_t* __restrict__ succ,
                                                              uint32_t* __restrict__ ptr, uint32_t* __restrict__ lab, uint32_t* __restrict__ off) {
    const int64_t b = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (b >= nb) return;
    const uint32_t h = (uint32_t)half_edge[b], k = h % 3u, next = h - k + (k == 2u ? 0u : k + 1u);
    uint32_t s = border_out[corner[next]];
    if (s >= (uint32_t)nb) s = (uint32_t)b;
    succ[b] = s; ptr[b] = s; lab[b] = (uint32_t)b; off[b] = 0u;
}

__global__ void __launch_bounds__(RT) repair_start_kernel(int64_t nb, const uint32_t* __restrict__ lab, uint32_t* __restrict__ start) {
    const int64_t b = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (b < nb) start[b] = lab[b] == (uint32_t)b ? 1u : 0u;
}

// after the scan of start: loop l = lpos[its start]; its length is the distance from the start's successor back to the start, plus one.
// What rule 6 adds for it under `cap` goes to the three arrays the offsets are scanned from, and to the tallies.
__global__ void __launch_bounds__(RT) repair_length_kernel(int64_t nb, int64_t cap, const uint32_t* __restrict__ lpos, const uint32_t* __restrict__ ltotal,
                                                           const uint32_t* __restrict__ succ, const uint32_t* __restrict__ off,
                                                           int32_t* __restrict__ lengths, uint32_t* __restrict__ g, uint32_t* __restrict__ tr,
                                                           uint32_t* __restrict__ ce, uint32_t* __restrict__ tally) {
    const int64_t b = (int64_t)blockIdx.x * RT + threadIdx.x;
    uint32_t c[T_WORDS] = {0, 0, 0, 0, 0, 0, 0};
    if (b < nb && scanned_flag(lpos, ltotal, b, nb)) {
        const uint32_t l = lpos[b], L = off[succ[b]] + 1u;
        const bool filled = (int64_t)L <= cap;
        lengths[l] = (int32_t)L;
        g[l] = filled ? L : 0u;
        tr[l] = filled ? (L == 3u ? 1u : L) : 0u;
        ce[l] = filled && L > 3u ? 1u : 0u;
        c[T_LONGEST] = L; c[T_FILLED] = filled ? 1u : 0u; c[T_FILL_TRIS] = tr[l]; c[T_FILL_VERTS] = ce[l]; c[T_FILL_EDGES] = g[l];
    }
    c[T_LONGEST] = wave_max(c[T_LONGEST]);
#pragma unroll
    for (int k = T_FILLED; k < T_WORDS; k++) c[k] = wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0) {
        if (c[T_LONGEST]) atomicMax(&tally[T_LONGEST], c[T_LONGEST]);
#pragma unroll
        for (int k = T_FILLED; k < T_WORDS; k++)
            if (c[k]) atomicAdd(&tally[k], c[k]);
    }
}

// loop[b], position[b]; the half-edges of a filled loop leave their source vertex at fill_offset[loop] + position
__global__ void __launch_bounds__(RT) repair_assign_kernel(int64_t nb, int64_t cap, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ off,
                                                           const uint32_t* __restrict__ lpos, const int32_t* __restrict__ lengths,
                                                           const uint32_t* __restrict__ gofs, const int32_t* __restrict__ half_edge,
                                                           const int32_t* __restrict__ corner, int32_t* __restrict__ loop, int32_t* __restrict__ position,
                                                           uint32_t* __restrict__ fill_vertex) {
    const int64_t b = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (b >= nb) return;
    const uint32_t l = lpos[lab[b]], L = (uint32_t)lengths[l], d = off[b], pos = d == 0u ? 0u : L - d;
    loop[b] = (int32_t)l;
    position[b] = (int32_t)pos;
    if ((int64_t)L <= cap && (int64_t)gofs[l] + pos < nb) fill_vertex[gofs[l] + pos] = (uint32_t)corner[half_edge[b]];
}

// ---- rules 6, 7: the outputs ------------------------------------------------------------------------------------------------------------
// rows V .. V + S + C of the vertex arrays: a split copy repeats its source's words; vertex_source for every row
__global__ void __launch_bounds__(RT) repair_vertices_kernel(int64_t V, int64_t S, int64_t C, const int32_t* __restrict__ split_source,
                                                             float* __restrict__ out_verts, float* __restrict__ out_colors,
                                                             int32_t* __restrict__ vertex_source) {
    const int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (v >= V + S + C) return;
    int32_t from = -1;
    if (v < V) from = (int32_t)v;
    else if (v < V + S) {
        from = split_source[v - V];
        uint32_t* p = reinterpret_cast<uint32_t*>(out_verts);
        p[3 * v] = p[3 * (int64_t)from]; p[3 * v + 1] = p[3 * (int64_t)from + 1]; p[3 * v + 2] = p[3 * (int64_t)from + 2];
        if (out_colors) {
            uint32_t* q = reinterpret_cast<uint32_t*>(out_colors);
            q[3 * v] = q[3 * (int64_t)from]; q[3 * v + 1] = q[3 * (int64_t)from + 1]; q[3 * v + 2] = q[3 * (int64_t)from + 2];
        }
    }
    vertex_source[v] = from;
}

// A workgroup per loop; only a filled loop of more than three edges has a centroid.  RT lanes gather RT of the loop's vertices at once
// and park them, lanes 0..2 add the parked terms of their position component in ascending order from +0.0, lanes 3..5 those of the
// colour: the bits of the sequential sum (rule 6), as the long rows of mesh_smooth.hip.  The rows below V + S are complete before.
__global__ void __launch_bounds__(RT) repair_centroid_kernel(int64_t cap, int64_t first_row, const int32_t* __restrict__ lengths,
                                                             const uint32_t* __restrict__ gofs, const uint32_t* __restrict__ cofs,
                                                             const uint32_t* __restrict__ fill_vertex, float* __restrict__ out_verts,
                                                             float* __restrict__ out_colors) {
    __shared__ float s_p[6][RT + 1];
    const int tid = threadIdx.x;
    const int64_t l = blockIdx.x;
    const int32_t L = lengths[l];
    if (L <= 3 || (int64_t)L > cap) return;      // (the same for every thread)
    const int64_t g0 = gofs[l], row = first_row + cofs[l];
    const int lanes = out_colors ? 6 : 3;
    double acc = 0.0;
    for (int32_t base = 0; base < L; base += RT) {
        const int n = L - base < RT ? L - base : RT;
        if (tid < n) {
            const int64_t v = fill_vertex[g0 + base + tid];
#pragma unroll
            for (int k = 0; k < 3; k++) s_p[k][tid] = out_verts[3 * v + k];
            if (out_colors) {
#pragma unroll
                for (int k = 0; k < 3; k++) s_p[3 + k][tid] = out_colors[3 * v + k];
            }
        }
        __syncthreads();
        if (tid < lanes)
            for (int k = 0; k < n; k++) acc += (double)s_p[tid][k];
        __syncthreads();
    }
    if (tid < lanes) {
        const float r = (float)(acc / (double)L);
        if (tid < 3) out_verts[3 * row + tid] = r; else out_colors[3 * row + tid - 3] = r;
    }
}

// a lane per border half-edge: its fill triangle (dst, src, centroid), or for a loop of three the one triangle at position 0
__global__ void __launch_bounds__(RT) repair_fill_kernel(int64_t nb, int64_t cap, int64_t Fs, int64_t first_row, const int32_t* __restrict__ loop,
                                                         const int32_t* __restrict__ position, const int32_t* __restrict__ lengths,
                                                         const uint32_t* __restrict__ gofs, const uint32_t* __restrict__ tofs,
                                                         const uint32_t* __restrict__ cofs, const uint32_t* __restrict__ fill_vertex,
                                                         int32_t* __restrict__ out_tris, int32_t* __restrict__ triangle_source) {
    const int64_t b = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (b >= nb) return;
    const int32_t l = loop[b], L = lengths[l], pos = position[b];
    if ((int64_t)L > cap) return;
    const uint32_t* fv = fill_vertex + gofs[l];
    int64_t t;
    int32_t tri[3];
    if (L == 3) {
        if (pos != 0) return;
        t = Fs + tofs[l];
        tri[0] = (int32_t)fv[0]; tri[1] = (int32_t)fv[2]; tri[2] = (int32_t)fv[1];
    } else {
        t = Fs + tofs[l] + pos;
        tri[0] = (int32_t)fv[pos + 1 == L ? 0 : pos + 1]; tri[1] = (int32_t)fv[pos]; tri[2] = (int32_t)(first_row + cofs[l]);
    }
    out_tris[3 * t] = tri[0]; out_tris[3 * t + 1] = tri[1]; out_tris[3 * t + 2] = tri[2];
    triangle_source[t] = -1 - l;
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, RT); }

// the two sets of arrays the rounds alternate between, and the rounds themselves: one launch and one read of the flag per round
struct Orbit {
    static constexpr int MAX_ROUNDS = 32;
    uint32_t *ptr[2], *lab[2], *off[2], *changed;
    int cur = 0;
    bool take(surfel_alloc_fn alloc, void* user, int64_t n) {
        for (int k = 0; k < 2; k++) { ptr[k] = surfel::take<uint32_t>(alloc, user, n); lab[k] = surfel::take<uint32_t>(alloc, user, n); off[k] = surfel::take<uint32_t>(alloc, user, n); }
        changed = surfel::take<uint32_t>(alloc, user, MAX_ROUNDS);      // (a flag per round, zeroed once per run)
        return ptr[0] && ptr[1] && lab[0] && lab[1] && off[0] && off[1] && changed;
    }
    // the caller has filled set 0; returns the rounds run (at least one for n > 0), negative on a failure
    int run(const char* what, int64_t n, bool rank, hipStream_t st) {
        cur = 0;
        int rounds = 0;
        uint32_t step = 1;
        if (n > 0 && hipMemsetAsync(changed, 0, MAX_ROUNDS * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
        while (n > 0 && rounds < MAX_ROUNDS) {      // (2^31 elements are seen whole after 31 rounds)
            uint32_t moved = 0;
            hipLaunchKernelGGL(rank ? orbit_round_kernel<true> : orbit_round_kernel<false>, dim3(grid(n)), dim3(RT), 0, st, n, ptr[cur], lab[cur],
                               off[cur], ptr[cur ^ 1], lab[cur ^ 1], off[cur ^ 1], step, changed + rounds);
            cur ^= 1;
            rounds++;
            if (int rc = read_words(what, changed + rounds - 1, &moved, 1, st)) return rc;
            if (!moved) break;
            step <<= 1;
        }
        return rounds;
    }
};

struct Stages {
    hipEvent_t ev[SURFEL_REPAIR_STAGES + 1];
    int n = 0;
    bool on;
    hipStream_t st;
    Stages(bool on_, hipStream_t st_) : on(on_), st(st_) {}
    ~Stages() { for (int k = 0; k < n; k++) (void)hipEventDestroy(ev[k]); }
    void mark() {
        if (!on || n > SURFEL_REPAIR_STAGES) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
        n++;
        (void)hipEventRecord(ev[n - 1], st);
    }
    void read(float* ms) {
        for (int k = 0; k < SURFEL_REPAIR_STAGES; k++) ms[k] = 0.0f;
        if (!on || n < 2 || hipEventSynchronize(ev[n - 1]) != hipSuccess) return;
        for (int k = 0; k + 1 < n; k++) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    }
};
}  // namespace

extern "C" {

int surfel_repair_analyze(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                          int64_t max_hole_edges, surfel_repair_plan* plan, int64_t* counts, float* stage_ms, void* stream) {
    const char* what = "repair_analyze";
    if (!alloc || V < 0 || F < 0 || max_hole_edges < 0 || !plan || !counts || (V > 0 && !verts) || (F > 0 && !tris))
        return api_fail(SURFEL_E_INVALID, "repair_analyze: bad arguments");
    if (F >= (REPAIR_LIMIT + 2) / 3 || V >= REPAIR_LIMIT || V + 3 * F >= REPAIR_LIMIT)
        return api_fail(SURFEL_E_LIMIT, "repair_analyze: 3 F or V + 3 F reaches 2^31 (three half-edges per triangle, one vertex per fan)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    *plan = surfel_repair_plan{};
    plan->V = V; plan->F = F; plan->max_hole_edges = max_hole_edges;
    const int64_t cap = max_hole_edges;
    uint32_t kept = 0, Fs = 0, S = 0, nb = 0, nloops = 0, tally[T_WORDS] = {0, 0, 0, 0, 0, 0, 0};
    int label_rounds = 0;
    Stages stages(stage_ms != nullptr, st);
    stages.mark();
    uint32_t* dtally = take<uint32_t>(alloc, user, T_WORDS);
    if (!dtally) return api_fail(SURFEL_E_ALLOC, what);
    if (hipMemsetAsync(dtally, 0, sizeof(tally), st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
    // ---- the sort
    ScanBuf keep;
    if (int rc = mesh_keep(what, alloc, user, V, F, verts, tris, &keep, &kept, st)) return rc;
    const int64_t n = 3 * (int64_t)kept;
    if (kept > 0) {
        SortPairs s(alloc, user, n);
        const ScanBuf surv = take_scan(alloc, user, F);
        uint32_t* cut = take<uint32_t>(alloc, user, F);
        uint32_t* partner = take<uint32_t>(alloc, user, n);
        if (!s.ok() || !surv.flags || !cut || !partner) return api_fail(SURFEL_E_ALLOC, what);
        const RepairKey key_of{tris};
        const int bits[2] = {bit_length(V - 1), bit_length(V - 1)};
        hipLaunchKernelGGL(repair_emit_kernel, dim3(grid(F)), dim3(RT), 0, st, F, key_of, keep.flags, keep.total, s.ka, s.va);
        if (int rc = sort_words(s, key_of, 2, bits, "repair_analyze: sort", st)) return rc;
        stages.mark();
        // ---- the cut, the survivors, the twins
        if (hipMemsetAsync(cut, 0, (size_t)F * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
        hipLaunchKernelGGL(repair_cut_kernel, dim3(grid(n)), dim3(RT), 0, st, n, tris, s.va, cut, partner, dtally);
        hipLaunchKernelGGL(repair_survive_kernel, dim3(grid(F)), dim3(RT), 0, st, F, keep.flags, keep.total, cut, surv.flags);
        surv.scan(st);
        if (int rc = read_words(what, surv.total, &Fs, 1, st)) return rc;
        if (int rc = launched("repair_cut_kernel")) return rc;
        if (Fs > 0) {
            const int64_t nh = 3 * (int64_t)Fs;
            uint32_t* hsrc = take<uint32_t>(alloc, user, nh);
            uint32_t* twin = take<uint32_t>(alloc, user, nh);
            uint32_t* fan = take<uint32_t>(alloc, user, nh);
            uint32_t* first = take<uint32_t>(alloc, user, V);
            uint32_t* new_index = take<uint32_t>(alloc, user, nh);
            const ScanBuf extra = take_scan(alloc, user, nh), border = take_scan(alloc, user, nh);
            Orbit orbit;
            plan->triangles = take<int32_t>(alloc, user, nh);
            plan->triangle_source = take<int32_t>(alloc, user, Fs);
            if (!orbit.take(alloc, user, nh) || !hsrc || !twin || !fan || !first || !new_index || !extra.flags || !border.flags || !plan->triangles ||
                !plan->triangle_source)
                return api_fail(SURFEL_E_ALLOC, what);
            hipLaunchKernelGGL(repair_compact_kernel, dim3(grid(F)), dim3(RT), 0, st, F, tris, surv.flags, surv.total, hsrc, plan->triangle_source);
            hipLaunchKernelGGL(repair_twin_kernel, dim3(grid(n)), dim3(RT), 0, st, n, F, s.va, partner, surv.flags, surv.total, twin);
            stages.mark();
            // ---- fans and the split
            hipLaunchKernelGGL(repair_fan_init_kernel, dim3(grid(nh)), dim3(RT), 0, st, nh, twin, orbit.ptr[0], orbit.lab[0]);
            if (int rc = orbit.run(what, nh, false, st); rc < 0) return rc;
            if (hipMemsetAsync(first, 0xFF, (size_t)V * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
            hipLaunchKernelGGL(repair_fan_first_kernel, dim3(grid(nh)), dim3(RT), 0, st, nh, orbit.lab[orbit.cur], hsrc, fan, first);
            hipLaunchKernelGGL(repair_flags_kernel, dim3(grid(nh)), dim3(RT), 0, st, nh, fan, hsrc, first, twin, extra.flags, border.flags);
            extra.scan(st);
            border.scan(st);
            if (int rc = read_words(what, extra.total, &S, 1, st, false)) return rc;
            if (int rc = read_words(what, border.total, &nb, 1, st)) return rc;
            if (int rc = launched("repair_flags_kernel")) return rc;
            if (S > 0) {
                SortPairs e(alloc, user, S);
                plan->split_source = take<int32_t>(alloc, user, S);
                if (!e.ok() || !plan->split_source) return api_fail(SURFEL_E_ALLOC, what);
                hipLaunchKernelGGL(repair_extra_emit_kernel, dim3(grid(nh)), dim3(RT), 0, st, nh, extra.flags, extra.total, hsrc, e.ka, e.va);
                if (e.sort(bit_length(V - 1), st) < 0) return api_fail(SURFEL_E_LIMIT, "repair_analyze: sort");
                hipLaunchKernelGGL(repair_rank_kernel, dim3(grid(S)), dim3(RT), 0, st, (int64_t)S, V, e.ka, e.va, new_index, plan->split_source);
            }
            hipLaunchKernelGGL(repair_corner_kernel, dim3(grid(nh)), dim3(RT), 0, st, nh, fan, hsrc, first, new_index, plan->triangles);
            stages.mark();
            // ---- loops
            if (nb > 0) {
                uint32_t* border_out = take<uint32_t>(alloc, user, V + (int64_t)S);
                uint32_t* succ = take<uint32_t>(alloc, user, nb);
                const ScanBuf start = take_scan(alloc, user, nb);
                plan->half_edge = take<int32_t>(alloc, user, nb);
                plan->loop = take<int32_t>(alloc, user, nb);
                plan->position = take<int32_t>(alloc, user, nb);
                plan->fill_vertex = take<uint32_t>(alloc, user, nb);
                if (!border_out || !succ || !start.flags || !plan->half_edge || !plan->loop || !plan->position || !plan->fill_vertex)
                    return api_fail(SURFEL_E_ALLOC, what);
                if (hipMemsetAsync(border_out, 0xFF, (size_t)(V + (int64_t)S) * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
                hipLaunchKernelGGL(repair_border_emit_kernel, dim3(grid(nh)), dim3(RT), 0, st, nh, border.flags, border.total, plan->triangles,
                                   plan->half_edge, border_out);
                hipLaunchKernelGGL(repair_loop_init_kernel, dim3(grid(nb)), dim3(RT), 0, st, (int64_t)nb, plan->half_edge, plan->triangles, border_out, succ,
                                   orbit.ptr[0], orbit.lab[0], orbit.off[0]);
                label_rounds = orbit.run(what, nb, true, st);
                if (label_rounds < 0) return label_rounds;
                hipLaunchKernelGGL(repair_start_kernel, dim3(grid(nb)), dim3(RT), 0, st, (int64_t)nb, orbit.lab[orbit.cur], start.flags);
                start.scan(st);
                if (int rc = read_words(what, start.total, &nloops, 1, st)) return rc;
                if (int rc = launched("repair_start_kernel")) return rc;
                stages.mark();
                // ---- the fill's bookkeeping (nb > 0: there is a loop)
                const ScanBuf g = take_scan(alloc, user, nloops), tr = take_scan(alloc, user, nloops), ce = take_scan(alloc, user, nloops);
                plan->lengths = take<int32_t>(alloc, user, nloops);
                if (!g.flags || !tr.flags || !ce.flags || !plan->lengths) return api_fail(SURFEL_E_ALLOC, what);
                hipLaunchKernelGGL(repair_length_kernel, dim3(grid(nb)), dim3(RT), 0, st, (int64_t)nb, cap, start.flags, start.total, succ, orbit.off[orbit.cur],
                                   plan->lengths, g.flags, tr.flags, ce.flags, dtally);
                g.scan(st);
                tr.scan(st);
                ce.scan(st);
                hipLaunchKernelGGL(repair_assign_kernel, dim3(grid(nb)), dim3(RT), 0, st, (int64_t)nb, cap, orbit.lab[orbit.cur], orbit.off[orbit.cur], start.flags,
                                   plan->lengths, g.flags, plan->half_edge, plan->triangles, plan->loop, plan->position, plan->fill_vertex);
                plan->fill_offset = g.flags; plan->triangle_offset = tr.flags; plan->centroid_offset = ce.flags;
            }
        }
        stages.mark();
        if (int rc = read_words(what, dtally, tally, T_WORDS, st)) return rc;
        if (int rc = launched("repair_assign_kernel")) return rc;
    }
    if (stage_ms) stages.read(stage_ms);
    plan->survivors = Fs; plan->split = S; plan->border = nb; plan->loops = nloops;
    plan->fill_triangles = tally[T_FILL_TRIS]; plan->fill_vertices = tally[T_FILL_VERTS];
    counts[0] = kept; counts[1] = F - kept; counts[2] = (int64_t)kept - Fs; counts[3] = tally[T_NONMANIFOLD]; counts[4] = tally[T_MISORIENTED];
    counts[5] = S; counts[6] = nloops; counts[7] = nb; counts[8] = tally[T_LONGEST]; counts[9] = tally[T_FILLED];
    counts[10] = tally[T_FILL_TRIS]; counts[11] = tally[T_FILL_VERTS]; counts[12] = (int64_t)nb - tally[T_FILL_EDGES]; counts[13] = label_rounds;
    return 0;
}

int surfel_repair_emit(const surfel_repair_plan* plan, const float* verts, const float* colors, float* out_verts, float* out_colors,
                       int32_t* out_tris, int32_t* vertex_source, int32_t* triangle_source, int32_t* loop_lengths, void* stream) {
    const char* what = "repair_emit";
    if (!plan) return api_fail(SURFEL_E_INVALID, "repair_emit: bad arguments");
    const int64_t V = plan->V, S = plan->split, C = plan->fill_vertices, Fs = plan->survivors, Ff = plan->fill_triangles, nb = plan->border;
    const int64_t cap = plan->max_hole_edges, rows = V + S + C;
    if (V < 0 || S < 0 || C < 0 || Fs < 0 || Ff < 0 || nb < 0 || plan->loops < 0 || (colors == nullptr) != (out_colors == nullptr) ||
        (V > 0 && !verts) || (rows > 0 && (!out_verts || !vertex_source)) || (Fs + Ff > 0 && (!out_tris || !triangle_source)) ||
        (plan->loops > 0 && !loop_lengths) || (Fs > 0 && (!plan->triangles || !plan->triangle_source)) || (S > 0 && !plan->split_source) ||
        (nb > 0 && (!plan->loop || !plan->position || !plan->lengths || !plan->fill_vertex || !plan->fill_offset || !plan->triangle_offset ||
                    !plan->centroid_offset)))
        return api_fail(SURFEL_E_INVALID, "repair_emit: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool ok = true;
    if (V > 0) {
        ok = ok && hipMemcpyAsync(out_verts, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, st) == hipSuccess;
        if (colors) ok = ok && hipMemcpyAsync(out_colors, colors, (size_t)V * 12, hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    if (Fs > 0) {
        ok = ok && hipMemcpyAsync(out_tris, plan->triangles, (size_t)Fs * 12, hipMemcpyDeviceToDevice, st) == hipSuccess;
        ok = ok && hipMemcpyAsync(triangle_source, plan->triangle_source, (size_t)Fs * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    if (plan->loops > 0) ok = ok && hipMemcpyAsync(loop_lengths, plan->lengths, (size_t)plan->loops * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (!ok) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
    if (rows > 0)
        hipLaunchKernelGGL(repair_vertices_kernel, dim3(grid(rows)), dim3(RT), 0, st, V, S, C, plan->split_source, out_verts, out_colors, vertex_source);
    if (C > 0)
        hipLaunchKernelGGL(repair_centroid_kernel, dim3((unsigned)plan->loops), dim3(RT), 0, st, cap, V + S, plan->lengths, plan->fill_offset,
                           plan->centroid_offset, plan->fill_vertex, out_verts, out_colors);
    if (Ff > 0)
        hipLaunchKernelGGL(repair_fill_kernel, dim3(grid(nb)), dim3(RT), 0, st, nb, cap, Fs, V + S, plan->loop, plan->position, plan->lengths,
                           plan->fill_offset, plan->triangle_offset, plan->centroid_offset, plan->fill_vertex, out_tris, triangle_source);
    return launched("repair_fill_kernel");
}

int surfel_repair_loops(const surfel_repair_plan* plan, int32_t* half_edge, int32_t* loop, int32_t* position, int32_t* lengths, void* stream) {
    const char* what = "repair_loops";
    if (!plan || plan->border < 0 || plan->loops < 0 || (plan->border > 0 && (!half_edge || !loop || !position || !plan->half_edge || !plan->loop || !plan->position)) ||
        (plan->loops > 0 && (!lengths || !plan->lengths)))
        return api_fail(SURFEL_E_INVALID, "repair_loops: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nb = (size_t)plan->border * 4;
    bool ok = true;
    if (plan->border > 0)
        ok = hipMemcpyAsync(half_edge, plan->half_edge, nb, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(loop, plan->loop, nb, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(position, plan->position, nb, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (plan->loops > 0) ok = ok && hipMemcpyAsync(lengths, plan->lengths, (size_t)plan->loops * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    return ok ? 0 : api_fail(SURFEL_E_HIP, what, hipGetLastError());
}

}  // extern "C"
