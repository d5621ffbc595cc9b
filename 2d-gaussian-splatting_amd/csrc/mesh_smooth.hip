// mesh_smooth.hip — vertex adjacency and Laplacian / Taubin smoothing of a triangle mesh (include/surfel_smooth.h, SMOOTH.md): kept
// triangles (mesh_topology.h) -> six directed vertex pairs each -> sort_words by (src, dst) (side_util.h) -> run heads and a scan number the
// unique directed edges -> CSR rows by a search over the edges' sources, the run length beside every neighbour, flags and counts per
// vertex.  A filter step is one launch: a lane per vertex gathers its row in order; a row longer than LONG_ROW is gathered by the whole
// workgroup, a tile of ST entries at a time parked in LDS, and added in the same order.
// Compiled with -ffp-contract=off (build.py): every fp64 operation of a step rounds once, as its numpy restatement
// (tests/smooth_oracle.py).  No floating-point atomic: the sort is the store pass, the row is the per-destination sum.  wave64; LDS for
// the parked terms of long rows; no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_smooth.h"
#include "block_ops.h"
#include "mesh_topology.h"

namespace surfel {

constexpr int ST = 256;                                  // threads per workgroup
constexpr int LONG_ROW = 32;                             // rows above this many entries are gathered by the workgroup
constexpr int64_t SMOOTH_LIMIT = (int64_t)1 << 31;       // V and 6 F stay below

// slot s = 2 h + r: half-edge h (mesh_topology.h), reversed when r = 1
__device__ __forceinline__ void smooth_slot(const int32_t* __restrict__ tris, uint32_t s, uint32_t* src, uint32_t* dst) {
    if (s & 1u) half_edge_ends(tris, s >> 1, dst, src); else half_edge_ends(tris, s >> 1, src, dst);
}

struct SmoothKey {      // the sort's key (src, dst) of a slot: word 0 = dst, word 1 = src
    const int32_t* tris;
    __device__ uint32_t operator()(uint32_t slot, int word) const {
        uint32_t src, dst;
        smooth_slot(tris, slot, &src, &dst);
        return word ? src : dst;
    }
};

// ---- adjacency --------------------------------------------------------------------------------------------------------------------------
// after the exclusive scan of keep (mesh_topology.h): the six pairs of kept triangle number m at 6 m ..: key = dst, value = the slot 6 t + k
__global__ void __launch_bounds__(ST) smooth_emit_kernel(int64_t F, SmoothKey key_of, const uint32_t* __restrict__ pos,
                                                         const uint32_t* __restrict__ total, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (t >= F || !scanned_flag(pos, total, t, F)) return;
    const uint32_t m = pos[t];
#pragma unroll
    for (uint32_t k = 0; k < 6; k++) {
        key[6 * (int64_t)m + k] = key_of(6u * (uint32_t)t + k, 0);
        val[6 * (int64_t)m + k] = 6u * (uint32_t)t + k;
    }
}

// head[j] = 1 where sorted slot j opens a run of equal (src, dst)
__global__ void __launch_bounds__(ST) smooth_head_kernel(int64_t n, const int32_t* __restrict__ tris, const uint32_t* __restrict__ order,
                                                         uint32_t* __restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (j >= n) return;
    uint32_t src, dst, psrc = 0, pdst = 0;
    smooth_slot(tris, order[j], &src, &dst);
    if (j > 0) smooth_slot(tris, order[j - 1], &psrc, &pdst);
    head[j] = j == 0 || src != psrc || dst != pdst ? 1u : 0u;
}

// after the exclusive scan of the heads: directed edge e = epos[j] of every run head j — its source, its destination, its first slot
__global__ void __launch_bounds__(ST) smooth_edge_kernel(int64_t n, const int32_t* __restrict__ tris, const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ epos, const uint32_t* __restrict__ etotal,
                                                         uint32_t* __restrict__ esrc, int32_t* __restrict__ neighbors, uint32_t* __restrict__ estart) {
    const int64_t j = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (j >= n || !scanned_flag(epos, etotal, j, n)) return;
    const uint32_t e = epos[j];
    uint32_t src, dst;
    smooth_slot(tris, order[j], &src, &dst);
    esrc[e] = src;
    neighbors[e] = (int32_t)dst;
    estart[e] = (uint32_t)j;
}

// multiplicity[e] = the run's length (the grid covers n >= E2 threads)
__global__ void __launch_bounds__(ST) smooth_mult_kernel(int64_t n, const uint32_t* __restrict__ etotal, const uint32_t* __restrict__ estart,
                                                         int32_t* __restrict__ multiplicity) {
    const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
    const int64_t E2 = *etotal;
    if (e >= E2) return;
    const uint32_t end = e + 1 < E2 ? estart[e + 1] : (uint32_t)n;
    multiplicity[e] = (int32_t)(end - estart[e]);
}

// offsets[v] = the number of directed edges whose source is below v, v = 0 .. V (the sources ascend: a binary search)
__global__ void __launch_bounds__(ST) smooth_rows_kernel(int64_t V, const uint32_t* __restrict__ etotal, const uint32_t* __restrict__ esrc,
                                                         int32_t* __restrict__ offsets) {
    const int64_t v = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (v > V) return;
    uint32_t lo = 0, hi = *etotal;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)esrc[mid] < v) lo = mid + 1; else hi = mid;
    }
    offsets[v] = (int32_t)lo;
}

// flags[v], and tally += (directed edges of one triangle, of more than two, boundary vertices, isolated vertices), tally[4] = max degree:
// sums inside the wave by xor-shuffles, one integer atomic per wave and count (any order gives the same)
__global__ void __launch_bounds__(ST) smooth_flags_kernel(int64_t V, const int32_t* __restrict__ offsets, const int32_t* __restrict__ multiplicity,
                                                          uint8_t* __restrict__ flags, uint32_t* __restrict__ tally) {
    const int64_t v = (int64_t)blockIdx.x * ST + threadIdx.x;
    uint32_t c[5] = {0, 0, 0, 0, 0};
    if (v < V) {
        const int32_t o0 = offsets[v], o1 = offsets[v + 1];
        for (int32_t e = o0; e < o1; e++) {
            const int32_t m = multiplicity[e];
            c[0] += m == 1 ? 1u : 0u;
            c[1] += m > 2 ? 1u : 0u;
        }
        c[2] = c[0] > 0 ? 1u : 0u;
        c[3] = o1 == o0 ? 1u : 0u;
        c[4] = (uint32_t)(o1 - o0);
        flags[v] = (uint8_t)((c[2] ? SURFEL_SMOOTH_BOUNDARY : 0) | (c[1] ? SURFEL_SMOOTH_NONMANIFOLD : 0) | (c[3] ? SURFEL_SMOOTH_ISOLATED : 0));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = wave_sum(c[k]);
    c[4] = wave_max(c[4]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c[k]) atomicAdd(&tally[k], c[k]);
        if (c[4]) atomicMax(&tally[4], c[4]);
    }
}

// ---- one step ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void smooth_load(const float* __restrict__ p, int64_t j, float* r) {
    r[0] = p[3 * j]; r[1] = p[3 * j + 1]; r[2] = p[3 * j + 2];
}

// rule 4's last two operations, each rounded once
__device__ __forceinline__ float smooth_blend(float own, double s, int cnt, double f) {
    const double x = (double)own, m = s / (double)cnt;
    const double d = m - x;
    const double fd = f * d;
    return (float)(x + fd);
}

// One step (SMOOTH.md §Rules 4).  Lane = vertex: a pinned vertex copies its bits; a row of at most LONG_ROW entries is summed by the lane,
// one fp64 addition per neighbour in the row's order from +0.0.  Longer rows are queued in LDS and then taken one by one by the whole
// workgroup: ST lanes gather ST entries at once and park them, lanes 0..2 add the parked terms of their component in ascending order —
// the bits of the sequential sum, with the gathers, not the additions, spread over the lanes.  Under SURFEL_SMOOTH_CURVE a boundary
// vertex skips the entries whose multiplicity is not 1.
__global__ void __launch_bounds__(ST) smooth_step_kernel(int64_t V, const int32_t* __restrict__ offsets, const int32_t* __restrict__ neighbors,
                                                         const int32_t* __restrict__ multiplicity, const uint8_t* __restrict__ flags, int mode, double f,
                                                         const float* __restrict__ in, float* __restrict__ out) {
    __shared__ float s_p[3][ST + 1];      // (rows ST + 1 floats apart: the three adders read three different banks)
    __shared__ uint32_t s_use[ST];
    __shared__ int s_long[ST];
    __shared__ int s_nlong;
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * ST, i = first + tid;
    if (tid == 0) s_nlong = 0;
    __syncthreads();
    if (i < V) {
        const int32_t o0 = offsets[i], o1 = offsets[i + 1];
        const bool boundary = flags[i] & SURFEL_SMOOTH_BOUNDARY;
        if (o1 == o0 || (mode == SURFEL_SMOOTH_FIXED && boundary)) {      // the input's bit pattern
            const uint32_t* src = reinterpret_cast<const uint32_t*>(in) + 3 * i;
            uint32_t* dst = reinterpret_cast<uint32_t*>(out) + 3 * i;
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        } else if (o1 - o0 > LONG_ROW) {
            s_long[atomicAdd(&s_nlong, 1)] = tid;      // (the queue's order changes no result: every row is summed on its own)
        } else {
            const bool border_only = mode == SURFEL_SMOOTH_CURVE && boundary;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            int cnt = 0;
            for (int32_t e = o0; e < o1; e++) {
                if (border_only && multiplicity[e] != 1) continue;
                float r[3];
                smooth_load(in, neighbors[e], r);
                s0 += (double)r[0]; s1 += (double)r[1]; s2 += (double)r[2];
                cnt++;
            }
            float own[3];
            smooth_load(in, i, own);
            out[3 * i] = smooth_blend(own[0], s0, cnt, f);
            out[3 * i + 1] = smooth_blend(own[1], s1, cnt, f);
            out[3 * i + 2] = smooth_blend(own[2], s2, cnt, f);
        }
    }
    __syncthreads();
    const int nlong = s_nlong;      // (the same for every thread from here on)
    for (int q = 0; q < nlong; q++) {
        const int64_t v = first + s_long[q];
        const int32_t o0 = offsets[v], o1 = offsets[v + 1];
        const bool border_only = mode == SURFEL_SMOOTH_CURVE && (flags[v] & SURFEL_SMOOTH_BOUNDARY);
        double acc = 0.0;
        int cnt = 0;
        for (int32_t base = o0; base < o1; base += ST) {
            const int n = o1 - base < ST ? o1 - base : ST;
            if (tid < n) {
                const bool use = !border_only || multiplicity[base + tid] == 1;
                s_use[tid] = use ? 1u : 0u;
                if (use) {
                    float r[3];
                    smooth_load(in, neighbors[base + tid], r);
                    s_p[0][tid] = r[0]; s_p[1][tid] = r[1]; s_p[2][tid] = r[2];
                }
            }
            __syncthreads();
            if (tid < 3)
                for (int k = 0; k < n; k++)
                    if (s_use[k]) { acc += (double)s_p[tid][k]; cnt++; }
            __syncthreads();
        }
        if (tid < 3) out[3 * v + tid] = smooth_blend(in[3 * v + tid], acc, cnt, f);
    }
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, ST); }
}  // namespace

extern "C" {

int64_t surfel_smooth_adjacency(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                                int32_t* offsets, int32_t* neighbors, int32_t* multiplicity, uint8_t* flags, int64_t* counts, void* stream) {
    const char* what = "smooth_adjacency";
    if (!alloc || V < 0 || F < 0 || !counts || !offsets || (V > 0 && (!verts || !flags)) || (F > 0 && (!tris || !neighbors || !multiplicity)))
        return api_fail(SURFEL_E_INVALID, "smooth_adjacency: bad arguments");
    if (V >= SMOOTH_LIMIT || F >= (SMOOTH_LIMIT + 5) / 6)
        return api_fail(SURFEL_E_LIMIT, "smooth_adjacency: 2^31 or more vertices or directed vertex pairs (six per triangle)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t kept = 0, E2 = 0, tally[5] = {0, 0, 0, 0, 0};
    ScanBuf keep;
    if (int rc = mesh_keep(what, alloc, user, V, F, verts, tris, &keep, &kept, st)) return rc;
    if (kept > 0) {
        const int64_t n = 6 * (int64_t)kept;
        SortPairs s(alloc, user, n);
        const ScanBuf head = take_scan(alloc, user, n);
        uint32_t* esrc = take<uint32_t>(alloc, user, n);
        uint32_t* estart = take<uint32_t>(alloc, user, n);
        uint32_t* dtally = take<uint32_t>(alloc, user, 5);
        if (!s.ok() || !head.flags || !esrc || !estart || !dtally) return api_fail(SURFEL_E_ALLOC, what);
        const SmoothKey key_of{tris};
        const int bits[2] = {bit_length(V - 1), bit_length(V - 1)};
        hipLaunchKernelGGL(smooth_emit_kernel, dim3(grid(F)), dim3(ST), 0, st, F, key_of, keep.flags, keep.total, s.ka, s.va);
        if (int rc = sort_words(s, key_of, 2, bits, "smooth_adjacency: sort", st)) return rc;
        hipLaunchKernelGGL(smooth_head_kernel, dim3(grid(n)), dim3(ST), 0, st, n, tris, s.va, head.flags);
        head.scan(st);
        hipLaunchKernelGGL(smooth_edge_kernel, dim3(grid(n)), dim3(ST), 0, st, n, tris, s.va, head.flags, head.total, esrc, neighbors, estart);
        hipLaunchKernelGGL(smooth_mult_kernel, dim3(grid(n)), dim3(ST), 0, st, n, head.total, estart, multiplicity);
        hipLaunchKernelGGL(smooth_rows_kernel, dim3(grid(V + 1)), dim3(ST), 0, st, V, head.total, esrc, offsets);
        if (hipMemsetAsync(dtally, 0, sizeof(tally), st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
        hipLaunchKernelGGL(smooth_flags_kernel, dim3(grid(V)), dim3(ST), 0, st, V, offsets, multiplicity, flags, dtally);
        if (int rc = read_words(what, dtally, tally, 5, st, false)) return rc;
        if (int rc = read_words(what, head.total, &E2, 1, st)) return rc;
        if (int rc = launched("smooth_flags_kernel")) return rc;
    }
    if (kept == 0) {      // no edge: empty rows, every vertex isolated
        if (hipMemsetAsync(offsets, 0, (size_t)(V + 1) * 4, st) != hipSuccess ||
            (V > 0 && hipMemsetAsync(flags, SURFEL_SMOOTH_ISOLATED, (size_t)V, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
            return api_fail(SURFEL_E_HIP, what, hipGetLastError());
        tally[3] = (uint32_t)V;
    }
    counts[0] = kept; counts[1] = F - kept; counts[2] = E2; counts[3] = tally[0] / 2; counts[4] = tally[1] / 2;
    counts[5] = tally[2]; counts[6] = tally[3]; counts[7] = tally[4];
    return E2;
}

int surfel_smooth_steps(int64_t V, const int32_t* offsets, const int32_t* neighbors, const int32_t* multiplicity, const uint8_t* flags,
                        int mode, int nsteps, const double* factors, const float* attr_in, float* scratch, float* attr_out, void* stream) {
    const char* what = "smooth_steps";
    if (V < 0 || nsteps < 0 || mode < SURFEL_SMOOTH_FREE || mode > SURFEL_SMOOTH_CURVE || (nsteps > 0 && !factors) ||
        (V > 0 && (!offsets || !flags || !attr_in || !attr_out || (nsteps > 1 && !scratch))))
        return api_fail(SURFEL_E_INVALID, "smooth_steps: bad arguments");
    for (int k = 0; k < nsteps; k++)
        if (!(fabs(factors[k]) < INFINITY)) return api_fail(SURFEL_E_INVALID, "smooth_steps: a factor is not finite");
    if (V >= SMOOTH_LIMIT) return api_fail(SURFEL_E_LIMIT, "smooth_steps: 2^31 or more vertices");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (V == 0) return 0;
    if (nsteps == 0) {
        if (hipMemcpyAsync(attr_out, attr_in, (size_t)V * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) return api_fail(SURFEL_E_HIP, what, hipGetLastError());
        return 0;
    }
    const float* src = attr_in;
    for (int k = 0; k < nsteps; k++) {
        float* dst = ((nsteps - 1 - k) & 1) ? scratch : attr_out;      // (the last step writes attr_out)
        hipLaunchKernelGGL(smooth_step_kernel, dim3(grid(V)), dim3(ST), 0, st, V, offsets, neighbors, multiplicity, flags, mode, factors[k], src, dst);
        src = dst;
    }
    return launched("smooth_step_kernel");
}

}  // extern "C"
