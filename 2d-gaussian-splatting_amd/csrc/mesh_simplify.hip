// mesh_simplify.hip — mesh simplification by quadric vertex clustering (include/surfel_simplify.h, SIMPLIFY.md): vertices -> 63-bit cell
// keys -> sort_words (side_util.h) -> run heads and a scan number the occupied cells; triangles mapped through the cells, those that
// repeat a cell dropped, later copies of a rotated triple dropped after a three-word sort; per used cell one wave sums the plane
// quadrics of the cell's (triangle, corner) incidences and its members in a fixed order in fp64 and solves the regularised 3 x 3 system
// in closed form.
// Compiled with -ffp-contract=off (build.py): the fp32 cell index and every fp64 operation of the sums and the solve round once, as
// their numpy restatement (tests/simplify_oracle.py).  No floating-point atomic: the bounds are integer atomics on order-preserving keys,
// every sum is a store pass (the sort) plus a per-destination sum pass.  wave64; LDS in the bounds reduction and for the parked terms; no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "../../include/surfel_simplify.h"
#include "block_ops.h"
#include "side_util.h"

namespace surfel {

constexpr int ST = 256;                                        // threads per workgroup
constexpr int AXIS_BITS = SURFEL_SIMPLIFY_AXIS_BITS;
constexpr uint32_t AXIS_MASK = (1u << AXIS_BITS) - 1u;
constexpr uint64_t KEY_NONE = ~0ull;                           // the key of a vertex that belongs to no cell: behind every cell key (63 bits)
constexpr uint32_t BOUND_NONE_LO = 0xffffffffu, BOUND_NONE_HI = 0u;      // identities of min / max: the order key of no finite float
constexpr int64_t SIMP_MAX_V = ((int64_t)1 << 30) - 2;         // the sort's limit
constexpr int64_t SIMP_MAX_F = (((int64_t)1 << 30) - 2) / 3;   // three incidences per triangle in one sort

struct SimpGrid { float ox, oy, oz, cell; };

__device__ __forceinline__ uint32_t simp_order_key(float v) {      // unsigned order = float order (finite v)
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

// cell index of one coordinate: floor((v - origin) / cell) in fp32, one rounding per operation; false outside [0, 2^AXIS_BITS) (and for NaN)
__device__ __forceinline__ bool simp_axis(float v, float o, float cell, uint32_t* out) {
    const float q = floorf(__fdiv_rn(__fsub_rn(v, o), cell));
    if (!(q >= 0.0f && q < (float)(1u << AXIS_BITS))) return false;
    *out = (uint32_t)q;
    return true;
}

__global__ void simp_bounds_reset_kernel(uint32_t* __restrict__ keys) {
    if (threadIdx.x < 6) keys[threadIdx.x] = threadIdx.x < 3 ? BOUND_NONE_LO : BOUND_NONE_HI;
}

// keys[0..2] = min, keys[3..5] = max of the order keys of the finite vertices: xor-shuffles inside the wave, the waves through LDS, one
// integer atomic per workgroup and component
__global__ void __launch_bounds__(ST) simp_bounds_kernel(int64_t V, const float* __restrict__ verts, uint32_t* __restrict__ keys) {
    __shared__ uint32_t s_k[ST / 64][6];
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    uint32_t k[6] = {BOUND_NONE_LO, BOUND_NONE_LO, BOUND_NONE_LO, BOUND_NONE_HI, BOUND_NONE_HI, BOUND_NONE_HI};
    if (i < V) {
        const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
        if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) {
            k[0] = k[3] = simp_order_key(x);
            k[1] = k[4] = simp_order_key(y);
            k[2] = k[5] = simp_order_key(z);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { k[c] = wave_min(k[c]); k[c + 3] = wave_max(k[c + 3]); }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < 6; c++) s_k[threadIdx.x >> 6][c] = k[c];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        uint32_t v = s_k[0][c];
        for (int w = 1; w < ST / 64; w++) v = c < 3 ? min(v, s_k[w][c]) : max(v, s_k[w][c]);
        if (c < 3) { if (v != BOUND_NONE_LO) atomicMin(&keys[c], v); }
        else if (v != BOUND_NONE_HI) atomicMax(&keys[c], v);
    }
}

// ---- clusters ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ST) simp_key_kernel(int64_t V, const float* __restrict__ verts, SimpGrid g, uint64_t* __restrict__ key64,
                                                      uint32_t* __restrict__ key_lo, uint32_t* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (i >= V) return;
    const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    uint32_t ix, iy, iz;
    uint64_t key = KEY_NONE;
    if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && simp_axis(x, g.ox, g.cell, &ix) && simp_axis(y, g.oy, g.cell, &iy) &&
        simp_axis(z, g.oz, g.cell, &iz))
        key = (uint64_t)iz << (2 * AXIS_BITS) | (uint64_t)iy << AXIS_BITS | ix;
    key64[i] = key;
    key_lo[i] = key_word(key, 0);      // (CellKey's word 0, from the register)
    val[i] = (uint32_t)i;
}

struct CellKey {      // the sort's key of a vertex: the two words of its cell key
    const uint64_t* key64;
    __device__ uint32_t operator()(uint32_t v, int word) const { return key_word(key64[v], word); }
};

// head[j] = 1 where sorted slot j opens an occupied cell
__global__ void __launch_bounds__(ST) simp_head_kernel(int64_t V, const uint64_t* __restrict__ key64, const uint32_t* __restrict__ order,
                                                       uint32_t* __restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (j >= V) return;
    const uint64_t k = key64[order[j]];
    head[j] = k != KEY_NONE && (j == 0 || key64[order[j - 1]] != k) ? 1u : 0u;
}

// after the exclusive scan of the heads: a slot's cell is (the scan's next entry) - 1.  cluster[vertex], and the first slot of every cell
// in cstart[cell] with the number of clustered vertices in cstart[nc] (cstart may be NULL).
__global__ void __launch_bounds__(ST) simp_number_kernel(int64_t V, const uint64_t* __restrict__ key64, const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ excl, const uint32_t* __restrict__ total,
                                                         int32_t* __restrict__ cluster, uint32_t* __restrict__ cstart) {
    const int64_t j = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (j >= V) return;
    const uint32_t v = order[j];
    if (key64[v] == KEY_NONE) { cluster[v] = -1; return; }
    const uint32_t nc = *total;
    const uint32_t next = j + 1 < V ? excl[j + 1] : nc;
    const uint32_t c = next - 1u;
    cluster[v] = (int32_t)c;
    if (!cstart) return;
    if (next != excl[j]) cstart[c] = (uint32_t)j;      // (scanned_flag, with the next entry at hand)
    if (j + 1 == V || key64[order[j + 1]] == KEY_NONE) cstart[nc] = (uint32_t)(j + 1);
}

// ---- triangles --------------------------------------------------------------------------------------------------------------------------
// the three cells of triangle t; false for a triangle rule 1 drops
__device__ __forceinline__ bool simp_tri_cells(int64_t t, int64_t V, const int32_t* __restrict__ tris, const int32_t* __restrict__ cluster, int32_t* c) {
    const int32_t a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || d < 0 || d >= V) return false;
    c[0] = cluster[a]; c[1] = cluster[b]; c[2] = cluster[d];
    return c[0] >= 0 && c[1] >= 0 && c[2] >= 0;
}

// flag[t] = 1 for a triangle whose three cells differ; tally[0] += triangles that pass rule 1 (an integer count: any order gives the same)
__global__ void __launch_bounds__(ST) simp_tri_flag_kernel(int64_t F, int64_t V, const int32_t* __restrict__ tris, const int32_t* __restrict__ cluster,
                                                           uint32_t* __restrict__ flag, uint32_t* __restrict__ tally) {
    const int64_t t = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (t >= F) return;
    int32_t c[3];
    const bool ok = simp_tri_cells(t, V, tris, cluster, c);
    if (ok) atomicAdd(&tally[0], 1u);
    flag[t] = ok && c[0] != c[1] && c[1] != c[2] && c[0] != c[2] ? 1u : 0u;
}

// candidate m = pos[t] of every flagged triangle (ascending t): its triple rotated so that the smallest cell comes first, winding kept;
// the first sort's pairs (third cell, m)
__global__ void __launch_bounds__(ST) simp_cand_kernel(int64_t F, int64_t V, const int32_t* __restrict__ tris, const int32_t* __restrict__ cluster,
                                                       const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total, int32_t* __restrict__ trip,
                                                       uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (t >= F || !scanned_flag(pos, total, t, F)) return;
    const uint32_t m = pos[t];
    int32_t c[3];
    if (!simp_tri_cells(t, V, tris, cluster, c)) return;      // (a flagged triangle passes)
    const int r = c[0] < c[1] ? (c[0] < c[2] ? 0 : 2) : (c[1] < c[2] ? 1 : 2);
    const int32_t r0 = c[r], r1 = c[(r + 1) % 3], r2 = c[(r + 2) % 3];
    trip[3 * (int64_t)m] = r0; trip[3 * (int64_t)m + 1] = r1; trip[3 * (int64_t)m + 2] = r2;
    key[m] = (uint32_t)r2;      // (TripKey's word 0, from the register)
    val[m] = m;
}

struct TripKey {      // the sort's key of a candidate: (first, second, third cell), so word w is the triple's entry 2 - w
    const int32_t* trip;
    __device__ uint32_t operator()(uint32_t m, int word) const { return (uint32_t)trip[3 * (int64_t)m + 2 - word]; }
};

// keep[m] = 1 for the first candidate (lowest m: the sorts are stable) of every run of equal triples
__global__ void __launch_bounds__(ST) simp_dup_kernel(int64_t M, const int32_t* __restrict__ trip, const uint32_t* __restrict__ order,
                                                      uint32_t* __restrict__ keep) {
    const int64_t j = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (j >= M) return;
    const int64_t m = order[j];
    bool first = j == 0;
    if (!first) {
        const int64_t p = order[j - 1];
        first = trip[3 * m] != trip[3 * p] || trip[3 * m + 1] != trip[3 * p + 1] || trip[3 * m + 2] != trip[3 * p + 2];
    }
    keep[m] = first ? 1u : 0u;
}

// after the exclusive scan of keep: used[cell] = 1 for the cells of the survivors (every writer stores the same 1)
__global__ void __launch_bounds__(ST) simp_used_kernel(int64_t M, const int32_t* __restrict__ trip, const uint32_t* __restrict__ kpos,
                                                       const uint32_t* __restrict__ ktotal, uint32_t* __restrict__ used) {
    const int64_t m = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (m >= M || !scanned_flag(kpos, ktotal, m, M)) return;
    used[trip[3 * m]] = 1u; used[trip[3 * m + 1]] = 1u; used[trip[3 * m + 2]] = 1u;
}

// after the exclusive scan of used: the surviving triangles in their original order with the output vertices' numbers
__global__ void __launch_bounds__(ST) simp_tris_out_kernel(int64_t M, const int32_t* __restrict__ trip, const uint32_t* __restrict__ kpos,
                                                           const uint32_t* __restrict__ ktotal, const uint32_t* __restrict__ upos,
                                                           int32_t* __restrict__ tris_out) {
    const int64_t m = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (m >= M || !scanned_flag(kpos, ktotal, m, M)) return;
    const uint32_t o = kpos[m];
    for (int k = 0; k < 3; k++) tris_out[3 * (int64_t)o + k] = (int32_t)upos[trip[3 * m + k]];
}

// ---- sums and solve ---------------------------------------------------------------------------------------------------------------------
// the pairs (cell of the corner, 3 t + corner) of every triangle that passes rule 1; the key nc (behind every cell) for the others
__global__ void __launch_bounds__(ST) simp_incidence_kernel(int64_t F, int64_t V, const int32_t* __restrict__ tris, const int32_t* __restrict__ cluster,
                                                            uint32_t nc, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (t >= F) return;
    int32_t c[3];
    const bool ok = simp_tri_cells(t, V, tris, cluster, c);
    for (int k = 0; k < 3; k++) {
        key[3 * t + k] = ok ? (uint32_t)c[k] : nc;
        val[3 * t + k] = (uint32_t)(3 * t + k);
    }
}

// [istart, iend) of every cell in the sorted incidences (both zeroed before: a cell without a triangle keeps an empty range)
__global__ void __launch_bounds__(ST) simp_ranges_kernel(int64_t n, const uint32_t* __restrict__ key, uint32_t nc, uint32_t* __restrict__ istart,
                                                         uint32_t* __restrict__ iend) {
    const int64_t j = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = key[j];
    if (k >= nc) return;
    if (j == 0 || key[j - 1] != k) istart[k] = (uint32_t)j;
    if (j + 1 == n || key[j + 1] != k) iend[k] = (uint32_t)(j + 1);
}

// One wave per cell (a workgroup of 64): the lanes gather and form the terms of up to 64 members / incidences at once and park them in
// LDS; then lane a adds term a of every parked entry in ascending order — members in ascending vertex id, incidences in ascending
// 3 t + corner, one fp64 addition per term from +0.0 (SIMPLIFY.md §Rules 4): the bits of the sequential sum, with the gathers, not the
// additions, spread over the wave.  Lane 0 solves and stores the output vertex and colour at upos[cell]; cluster_vertex[cell] for every
// cell.  s_t rows are 65 doubles apart: the nine adders read nine different bank pairs.
constexpr int SOLVE_T = 64, SOLVE_TERMS = 9;
__global__ void __launch_bounds__(SOLVE_T) simp_solve_kernel(int64_t nc, int64_t V, SimpGrid g, double lam, const float* __restrict__ verts,
                                                             const float* __restrict__ colors, const int32_t* __restrict__ tris,
                                                             const uint64_t* __restrict__ key64, const uint32_t* __restrict__ order,
                                                             const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ inc,
                                                             const uint32_t* __restrict__ istart, const uint32_t* __restrict__ iend,
                                                             const uint32_t* __restrict__ upos, const uint32_t* __restrict__ utotal,
                                                             int32_t* __restrict__ cluster_vertex, float* __restrict__ verts_out,
                                                             float* __restrict__ colors_out) {
    __shared__ double s_t[SOLVE_TERMS][SOLVE_T + 1];
    __shared__ double s_sum[6 + SOLVE_TERMS];
    const int64_t c = blockIdx.x;      // (the grid has nc workgroups)
    const int lane = threadIdx.x;
    const uint32_t o = upos[c];
    const bool used = scanned_flag(upos, utotal, c, nc);
    if (lane == 0 && cluster_vertex) cluster_vertex[c] = used ? (int32_t)o : -1;
    if (!used) return;      // (the whole workgroup)
    const uint32_t j0 = cstart[c], j1 = cstart[c + 1];
    const uint64_t key = key64[order[j0]];
    const double cell = (double)g.cell;
    const double cx = (double)g.ox + ((double)((uint32_t)key & AXIS_MASK) + 0.5) * cell;
    const double cy = (double)g.oy + ((double)((uint32_t)(key >> AXIS_BITS) & AXIS_MASK) + 0.5) * cell;
    const double cz = (double)g.oz + ((double)(uint32_t)(key >> (2 * AXIS_BITS)) + 0.5) * cell;
    // members: terms (x - cx, y - cy, z - cz, r, g, b); lanes 0..5 add
    double acc = 0.0;
    for (uint32_t base = j0; base < j1; base += SOLVE_T) {
        const uint32_t n = j1 - base < (uint32_t)SOLVE_T ? j1 - base : (uint32_t)SOLVE_T;
        if ((uint32_t)lane < n) {
            const int64_t v = order[base + lane];
            s_t[0][lane] = (double)verts[3 * v] - cx; s_t[1][lane] = (double)verts[3 * v + 1] - cy; s_t[2][lane] = (double)verts[3 * v + 2] - cz;
            if (colors) { s_t[3][lane] = (double)colors[3 * v]; s_t[4][lane] = (double)colors[3 * v + 1]; s_t[5][lane] = (double)colors[3 * v + 2]; }
        }
        __syncthreads();
        if (lane < (colors ? 6 : 3))
#pragma unroll 8
            for (uint32_t k = 0; k < n; k++) acc += s_t[lane][k];
        __syncthreads();
    }
    if (lane < 6) s_sum[lane] = acc;
    // incidences: terms (nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx s, ny s, nz s); lanes 0..8 add
    acc = 0.0;
    const uint32_t i0 = istart[c], i1 = iend[c];
    for (uint32_t base = i0; base < i1; base += SOLVE_T) {
        const uint32_t n = i1 - base < (uint32_t)SOLVE_T ? i1 - base : (uint32_t)SOLVE_T;
        if ((uint32_t)lane < n) {
            const int64_t t = inc[base + lane] / 3u;
            const int64_t a0 = tris[3 * t], a1 = tris[3 * t + 1], a2 = tris[3 * t + 2];      // (in range: the incidence passed rule 1)
            const double p0x = verts[3 * a0], p0y = verts[3 * a0 + 1], p0z = verts[3 * a0 + 2];
            const double ux = (double)verts[3 * a1] - p0x, uy = (double)verts[3 * a1 + 1] - p0y, uz = (double)verts[3 * a1 + 2] - p0z;
            const double wx = (double)verts[3 * a2] - p0x, wy = (double)verts[3 * a2 + 1] - p0y, wz = (double)verts[3 * a2 + 2] - p0z;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            const double s = (nx * (p0x - cx) + ny * (p0y - cy)) + nz * (p0z - cz);
            s_t[0][lane] = nx * nx; s_t[1][lane] = nx * ny; s_t[2][lane] = nx * nz; s_t[3][lane] = ny * ny; s_t[4][lane] = ny * nz; s_t[5][lane] = nz * nz;
            s_t[6][lane] = nx * s; s_t[7][lane] = ny * s; s_t[8][lane] = nz * s;
        }
        __syncthreads();
        if (lane < SOLVE_TERMS)
#pragma unroll 8
            for (uint32_t k = 0; k < n; k++) acc += s_t[lane][k];
        __syncthreads();
    }
    if (lane < SOLVE_TERMS) s_sum[6 + lane] = acc;
    __syncthreads();
    if (lane != 0) return;
    const double cnt = (double)(j1 - j0);
    const double mx = s_sum[0] / cnt, my = s_sum[1] / cnt, mz = s_sum[2] / cnt;
    const double axx = s_sum[6], axy = s_sum[7], axz = s_sum[8], ayy = s_sum[9], ayz = s_sum[10], azz = s_sum[11];
    const double bx = s_sum[12], by = s_sum[13], bz = s_sum[14];
    const double tr = (axx + ayy) + azz;
    double x = mx, y = my, z = mz;
    if (tr != 0.0) {      // (A / tr + lam I) x = b / tr + lam m by cofactors
        const double a = axx / tr + lam, b = axy / tr, cc = axz / tr, d = ayy / tr + lam, e = ayz / tr, f = azz / tr + lam;
        const double r0 = bx / tr + lam * mx, r1 = by / tr + lam * my, r2 = bz / tr + lam * mz;
        const double c00 = d * f - e * e, c01 = cc * e - b * f, c02 = b * e - cc * d, c11 = a * f - cc * cc, c12 = b * cc - a * e, c22 = a * d - b * b;
        const double det = (a * c00 + b * c01) + cc * c02;
        const double qx = ((c00 * r0 + c01 * r1) + c02 * r2) / det, qy = ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                     qz = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        if (__builtin_isfinite(qx) && __builtin_isfinite(qy) && __builtin_isfinite(qz)) { x = qx; y = qy; z = qz; }
    }
    const double h = cell * 0.5;
    x = x < -h ? -h : (x > h ? h : x); y = y < -h ? -h : (y > h ? h : y); z = z < -h ? -h : (z > h ? h : z);
    verts_out[3 * (int64_t)o] = (float)(cx + x); verts_out[3 * (int64_t)o + 1] = (float)(cy + y); verts_out[3 * (int64_t)o + 2] = (float)(cz + z);
    if (colors) {
        colors_out[3 * (int64_t)o] = (float)(s_sum[3] / cnt); colors_out[3 * (int64_t)o + 1] = (float)(s_sum[4] / cnt);
        colors_out[3 * (int64_t)o + 2] = (float)(s_sum[5] / cnt);
    }
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {

inline unsigned grid(int64_t n) { return blocks_for(n, ST); }
inline float key_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// the host's copy of simp_axis: the same two fp32 roundings (this file is compiled without contraction)
inline bool axis_fits(float v, float o, float cell, uint32_t* out) {
    volatile float d = v - o;
    volatile float q = d / cell;
    const float fl = floorf(q);
    if (!(fl >= 0.0f && fl < (float)(1u << AXIS_BITS))) return false;
    *out = (uint32_t)fl;
    return true;
}

int bounds_of(const char* what, int64_t V, const float* verts, surfel_alloc_fn alloc, void* user, float* bounds, hipStream_t st) {
    for (int k = 0; k < 6; k++) bounds[k] = 0.0f;
    if (V == 0) return 0;
    uint32_t* keys = take<uint32_t>(alloc, user, 6);
    if (!keys) return api_fail(SURFEL_E_ALLOC, what);
    hipLaunchKernelGGL(simp_bounds_reset_kernel, dim3(1), dim3(64), 0, st, keys);
    hipLaunchKernelGGL(simp_bounds_kernel, dim3(grid(V)), dim3(ST), 0, st, V, verts, keys);
    uint32_t host[6];
    if (int rc = read_words(what, keys, host, 6, st)) return rc;
    if (int rc = launched("simp_bounds_kernel")) return rc;
    if (host[0] == BOUND_NONE_LO) return 0;
    for (int k = 0; k < 6; k++) bounds[k] = key_float(host[k]);
    return 1;
}

// the state the stages hand on
struct Simp {
    const char* what;
    surfel_alloc_fn alloc; void* user; hipStream_t st;
    int64_t V, F;
    const float* verts; const int32_t* tris;
    SimpGrid g;
    int any;                      // a finite vertex exists
    int bits_hi;                  // bits of the cell key's high word that the vertex sort has to look at
    int64_t nc;                   // occupied cells
    uint64_t* key64; const uint32_t* order; uint32_t* cstart; int32_t* cluster;
    int64_t valid, M, kept;       // triangles that pass rule 1, candidates, survivors
    int32_t* trip; ScanBuf keep;  // the candidates' cell triples, their keep flags (after dedupe_triangles: positions)
    hipEvent_t ev[SURFEL_SIMPLIFY_STAGES + 1]; int nev; bool timed;
};

int stamp(Simp& s) {
    if (!s.timed) return 0;
    if (hipEventCreate(&s.ev[s.nev]) != hipSuccess) return api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
    s.nev++;
    return hipEventRecord(s.ev[s.nev - 1], s.st) == hipSuccess ? 0 : api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
}

void drop_events(Simp& s) {
    for (int k = 0; k < s.nev; k++) (void)hipEventDestroy(s.ev[k]);
    s.nev = 0;
}

// Rule 2: the grid, and the check that every finite vertex's cell index fits (the index is monotone in the coordinate, so the two corners
// of the bounds decide).  Nothing is written before this returns 0.
int set_grid(Simp& s, const float* bounds, const float* origin, float cell) {
    float own[6];
    if (!bounds) {
        const int rc = bounds_of(s.what, s.V, s.verts, s.alloc, s.user, own, s.st);
        if (rc < 0) return rc;
        s.any = rc;
        bounds = own;
    } else {
        s.any = s.V > 0;
    }
    const float* o = origin ? origin : bounds;
    s.g = SimpGrid{o[0], o[1], o[2], cell};
    s.bits_hi = 32;
    if (!s.any) return 0;
    uint32_t top[3];
    for (int k = 0; k < 3; k++) {
        uint32_t lo;
        if (!axis_fits(bounds[k], o[k], cell, &lo) || !axis_fits(bounds[3 + k], o[k], cell, &top[k]))
            return api_fail(SURFEL_E_LIMIT, "simplify: a cell index does not fit SURFEL_SIMPLIFY_AXIS_BITS bits, or a vertex lies below the origin "
                                            "(raise the cell size)");
    }
    // the largest high word of a cell key, and one bit more: the key of a skipped vertex sets it and so sorts behind every cell
    s.bits_hi = bit_length((uint64_t)top[2] << (2 * AXIS_BITS - 32) | top[1] >> (32 - AXIS_BITS)) + 1;
    return 0;
}

// Rule 3: keys, the stable two-word sort, run heads, the scan; cluster[V] and (with_starts) cstart[nc + 1]
int build_clusters(Simp& s, int32_t* cluster, bool with_starts) {
    const int64_t V = s.V;
    s.nc = 0; s.cstart = nullptr; s.order = nullptr;
    s.cluster = cluster ? cluster : take<int32_t>(s.alloc, s.user, V);
    if (!s.cluster) return api_fail(SURFEL_E_ALLOC, s.what);
    if (V == 0) { if (int rc = stamp(s)) return rc; return stamp(s); }
    if (!s.any) {
        if (hipMemsetAsync(s.cluster, 0xFF, (size_t)V * 4, s.st) != hipSuccess) return api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
        if (int rc = stamp(s)) return rc;
        return stamp(s);
    }
    s.key64 = take<uint64_t>(s.alloc, s.user, V);
    SortPairs sp(s.alloc, s.user, V);
    const ScanBuf head = take_scan(s.alloc, s.user, V);
    if (!s.key64 || !sp.ok() || !head.flags) return api_fail(SURFEL_E_ALLOC, s.what);
    hipLaunchKernelGGL(simp_key_kernel, dim3(grid(V)), dim3(ST), 0, s.st, V, s.verts, s.g, s.key64, sp.ka, sp.va);
    if (int rc = stamp(s)) return rc;
    // the 63-bit key by its 32-bit words; the key of a skipped vertex sets every bit of the high word
    const int bits[2] = {32, s.bits_hi};
    if (int rc = sort_words(sp, CellKey{s.key64}, 2, bits, "simplify: sort", s.st)) return rc;
    s.order = sp.va;
    hipLaunchKernelGGL(simp_head_kernel, dim3(grid(V)), dim3(ST), 0, s.st, V, s.key64, s.order, head.flags);
    head.scan(s.st);
    uint32_t nc = 0;
    if (with_starts) {      // (the numbering needs the count to size cstart)
        if (int rc = read_words(s.what, head.total, &nc, 1, s.st)) return rc;
        s.cstart = take<uint32_t>(s.alloc, s.user, (int64_t)nc + 1);
        if (!s.cstart) return api_fail(SURFEL_E_ALLOC, s.what);
    }
    hipLaunchKernelGGL(simp_number_kernel, dim3(grid(V)), dim3(ST), 0, s.st, V, s.key64, s.order, head.flags, head.total, s.cluster, s.cstart);
    if (!with_starts)
        if (int rc = read_words(s.what, head.total, &nc, 1, s.st)) return rc;
    s.nc = nc;
    if (int rc = launched("simp_number_kernel")) return rc;
    return stamp(s);
}

// Rule 7 up to the survivors: flags, candidates, three stable sorts, run heads, the scan of keep
int dedupe_triangles(Simp& s) {
    const int64_t V = s.V, F = s.F;
    s.valid = s.M = s.kept = 0; s.trip = nullptr; s.keep = ScanBuf();
    if (F == 0 || s.nc == 0) return stamp(s);
    const ScanBuf flag = take_scan(s.alloc, s.user, F, 1);
    if (!flag.flags) return api_fail(SURFEL_E_ALLOC, s.what);
    uint32_t* tally = flag.total + 1;      // the triangles that pass rule 1, behind the candidates' total
    if (hipMemsetAsync(tally, 0, 4, s.st) != hipSuccess) return api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
    hipLaunchKernelGGL(simp_tri_flag_kernel, dim3(grid(F)), dim3(ST), 0, s.st, F, V, s.tris, s.cluster, flag.flags, tally);
    flag.scan(s.st);
    uint32_t host[2];      // candidates, triangles that pass rule 1 (adjacent words)
    if (int rc = read_words(s.what, flag.total, host, 2, s.st)) return rc;
    if (int rc = launched("simp_tri_flag_kernel")) return rc;
    const int64_t M = host[0];
    s.M = M; s.valid = host[1];
    if (M == 0) return stamp(s);
    s.trip = take<int32_t>(s.alloc, s.user, 3 * M);
    SortPairs sp(s.alloc, s.user, M);
    s.keep = take_scan(s.alloc, s.user, M);
    if (!s.trip || !sp.ok() || !s.keep.flags) return api_fail(SURFEL_E_ALLOC, s.what);
    hipLaunchKernelGGL(simp_cand_kernel, dim3(grid(F)), dim3(ST), 0, s.st, F, V, s.tris, s.cluster, flag.flags, flag.total, s.trip, sp.ka, sp.va);
    // (first, second, third cell): third, second, first, bit_length(nc - 1) bits each
    const int bits[3] = {bit_length(s.nc - 1), bit_length(s.nc - 1), bit_length(s.nc - 1)};
    if (int rc = sort_words(sp, TripKey{s.trip}, 3, bits, "simplify: sort", s.st)) return rc;
    hipLaunchKernelGGL(simp_dup_kernel, dim3(grid(M)), dim3(ST), 0, s.st, M, s.trip, sp.va, s.keep.flags);
    s.keep.scan(s.st);
    uint32_t kept = 0;
    if (int rc = read_words(s.what, s.keep.total, &kept, 1, s.st)) return rc;
    s.kept = kept;
    if (int rc = launched("simp_dup_kernel")) return rc;
    return stamp(s);
}

void fill_counts(const Simp& s, int64_t nverts, int64_t* counts) {
    counts[0] = s.nc; counts[1] = nverts; counts[2] = s.kept;
    counts[3] = s.F - s.valid; counts[4] = s.valid - s.M; counts[5] = s.M - s.kept;
}

int check_sizes(const char* what, int64_t V, int64_t F, float cell) {
    if (!(cell > 0.0f) || !(cell < INFINITY)) return api_fail(SURFEL_E_INVALID, what);
    if (V > SIMP_MAX_V || F > SIMP_MAX_F) return api_fail(SURFEL_E_LIMIT, "simplify: more than 2^30 - 2 vertices or triangle corners (the sort's limit)");
    return 0;
}

}  // namespace

extern "C" {

int surfel_simplify_bounds(surfel_alloc_fn alloc, void* user, int64_t V, const float* verts, float* bounds, void* stream) {
    if (!alloc || V < 0 || !bounds || (V > 0 && !verts)) return api_fail(SURFEL_E_INVALID, "simplify_bounds: bad arguments");
    if (V > SIMP_MAX_V) return api_fail(SURFEL_E_LIMIT, "simplify_bounds: more than 2^30 - 2 vertices");
    return bounds_of("simplify_bounds", V, verts, alloc, user, bounds, static_cast<hipStream_t>(stream));
}

int64_t surfel_simplify_clusters(surfel_alloc_fn alloc, void* user, int64_t V, const float* verts, const float* bounds, const float* origin,
                                 float cell, int32_t* cluster, void* stream) {
    if (!alloc || V < 0 || (V > 0 && (!verts || !cluster))) return api_fail(SURFEL_E_INVALID, "simplify_clusters: bad arguments");
    if (int rc = check_sizes("simplify_clusters: the cell size must be positive and finite", V, 0, cell)) return rc;
    Simp s{};
    s.what = "simplify_clusters"; s.alloc = alloc; s.user = user; s.st = static_cast<hipStream_t>(stream); s.V = V; s.verts = verts;
    if (int rc = set_grid(s, bounds, origin, cell)) return rc;
    if (int rc = build_clusters(s, cluster, false)) return rc;
    return s.nc;
}

int64_t surfel_simplify_count(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                              const float* bounds, const float* origin, float cell, int64_t* counts, void* stream) {
    if (!alloc || V < 0 || F < 0 || !counts || (V > 0 && !verts) || (F > 0 && !tris)) return api_fail(SURFEL_E_INVALID, "simplify_count: bad arguments");
    if (int rc = check_sizes("simplify_count: the cell size must be positive and finite", V, F, cell)) return rc;
    Simp s{};
    s.what = "simplify_count"; s.alloc = alloc; s.user = user; s.st = static_cast<hipStream_t>(stream); s.V = V; s.F = F; s.verts = verts; s.tris = tris;
    if (int rc = set_grid(s, bounds, origin, cell)) return rc;
    if (int rc = build_clusters(s, nullptr, false)) return rc;
    if (int rc = dedupe_triangles(s)) return rc;
    fill_counts(s, 0, counts);
    return s.kept;
}

int surfel_simplify_mesh(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const float* colors, const int32_t* tris,
                         const float* bounds, const float* origin, float cell, double lam, int32_t* cluster, int32_t* cluster_vertex,
                         float* verts_out, float* colors_out, int32_t* tris_out, int64_t* counts, float* stage_ms, void* stream) {
    if (!alloc || V < 0 || F < 0 || !counts || (V > 0 && (!verts || !verts_out)) || (F > 0 && (!tris || !tris_out)) || (colors && V > 0 && !colors_out) ||
        !(lam > 0.0) || !(lam < INFINITY))
        return api_fail(SURFEL_E_INVALID, "simplify_mesh: bad arguments");
    if (int rc = check_sizes("simplify_mesh: the cell size must be positive and finite", V, F, cell)) return rc;
    Simp s{};
    s.what = "simplify_mesh"; s.alloc = alloc; s.user = user; s.st = static_cast<hipStream_t>(stream); s.V = V; s.F = F; s.verts = verts; s.tris = tris;
    s.timed = stage_ms != nullptr;
    // events: 0 start | 1 keys | 2 sorts | 3 remap and dedupe | 4 compaction | 5 sums and solve
    int rc = stamp(s);
    if (rc == 0) rc = set_grid(s, bounds, origin, cell);
    if (rc == 0) rc = build_clusters(s, cluster, true);
    if (rc == 0) rc = dedupe_triangles(s);
    int64_t nverts = 0;
    const int64_t nc = s.nc, M = s.M;
    hipStream_t st = s.st;
    auto emit = [&]() -> int {      // compaction, then the sums and the solve
        const int64_t n = 3 * F;
        const ScanBuf used = take_scan(alloc, user, nc);
        SortPairs sp(alloc, user, n);
        uint32_t* ranges = take<uint32_t>(alloc, user, 2 * nc);
        if (!used.flags || !sp.ok() || !ranges) return api_fail(SURFEL_E_ALLOC, s.what);
        (void)hipMemsetAsync(used.flags, 0, (size_t)nc * 4, st);
        hipLaunchKernelGGL(simp_used_kernel, dim3(grid(M)), dim3(ST), 0, st, M, s.trip, s.keep.flags, s.keep.total, used.flags);
        used.scan(st);
        hipLaunchKernelGGL(simp_tris_out_kernel, dim3(grid(M)), dim3(ST), 0, st, M, s.trip, s.keep.flags, s.keep.total, used.flags, tris_out);
        uint32_t nv = 0;
        if (int e = read_words(s.what, used.total, &nv, 1, st)) return e;
        nverts = nv;
        if (int e = launched("simp_tris_out_kernel")) return e;
        if (int e = stamp(s)) return e;
        // the (triangle, corner) incidences keyed by the corner's cell, one stable sort: a cell's incidences in ascending 3 t + corner
        hipLaunchKernelGGL(simp_incidence_kernel, dim3(grid(F)), dim3(ST), 0, st, F, V, tris, s.cluster, (uint32_t)nc, sp.ka, sp.va);
        if (sp.sort(bit_length(nc), st) < 0) return api_fail(SURFEL_E_LIMIT, "simplify: sort");      // (nc itself keys the corners without a cell)
        (void)hipMemsetAsync(ranges, 0, (size_t)nc * 8, st);
        hipLaunchKernelGGL(simp_ranges_kernel, dim3(grid(n)), dim3(ST), 0, st, n, sp.ka, (uint32_t)nc, ranges, ranges + nc);
        hipLaunchKernelGGL(simp_solve_kernel, dim3((unsigned)nc), dim3(SOLVE_T), 0, st, nc, V, s.g, lam, verts, colors, tris, s.key64, s.order, s.cstart,
                           sp.va, ranges, ranges + nc, used.flags, used.total, cluster_vertex, verts_out, colors_out);
        if (hipStreamSynchronize(st) != hipSuccess) return api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
        if (int e = launched("simp_solve_kernel")) return e;
        return stamp(s);
    };
    if (rc == 0 && s.kept > 0) {
        rc = emit();
    } else if (rc == 0) {      // no triangle survives: no vertex either
        if (cluster_vertex && nc > 0 && hipMemsetAsync(cluster_vertex, 0xFF, (size_t)nc * 4, st) != hipSuccess) rc = api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
        if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
        if (rc == 0) rc = stamp(s);
        if (rc == 0) rc = stamp(s);
    }
    if (rc == 0) {
        fill_counts(s, nverts, counts);
        if (stage_ms) {
            static const int stage_of[SURFEL_SIMPLIFY_STAGES] = {0, 1, 3, 4, 2};      // the k-th interval of the events is this stage
            for (int k = 0; k < SURFEL_SIMPLIFY_STAGES; k++) stage_ms[k] = 0.0f;
            if (hipEventSynchronize(s.ev[s.nev - 1]) != hipSuccess) rc = api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
            for (int k = 0; rc == 0 && k + 1 < s.nev; k++)
                if (hipEventElapsedTime(&stage_ms[stage_of[k]], s.ev[k], s.ev[k + 1]) != hipSuccess) rc = api_fail(SURFEL_E_HIP, s.what, hipGetLastError());
        }
    }
    drop_events(s);
    return rc;
}

}  // extern "C"
