// eval_tnt.hip — Tanks-and-Temples-style mesh evaluation: the cloud of a mesh, rigid / similarity transforms, the polygon-volume crop,
// voxel down-sampling, the correspondence sums of the similarity ICP and the distance histogram (include/surfel_eval_tnt.h, TNT.md).
// The neighbour search is eval_geometry.hip's.  Memory-bound gathers; no MFMA.  Compiled with -ffp-contract=off (build.py): the fp64
// decisions (inside / outside, cell of a point, bin of a distance) round exactly as their restatements in tests/tnt_oracle.py.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_eval_tnt.h"
#include "block_ops.h"
#include "side_util.h"

namespace surfel {

constexpr int TT = 256;                    // threads per workgroup
constexpr int TNT_SUM_BLOCKS = 1024;       // partial sums of tnt_corr_sums_kernel
constexpr int TNT_HIST_BLOCKS = 1024;      // workgroups of tnt_hist_kernel (each keeps its own counters in LDS)
constexpr int NS = SURFEL_TNT_CORR_SUMS;
constexpr int AXIS_BITS = SURFEL_TNT_VOXEL_AXIS_BITS;

struct TMat { double m[12]; };             // rows 0..2 of a 4 x 4

// ---- rule 1: the cloud of a mesh -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TT) tnt_mesh_cloud_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                            float* __restrict__ points) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= V + F) return;
    if (i < V) {
        for (int k = 0; k < 3; k++) points[3 * i + k] = verts[3 * i + k];
        return;
    }
    const int64_t t = i - V;
    const int32_t ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
    const bool ok = ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V;
    for (int k = 0; k < 3; k++) {
        float c = NAN;
        if (ok) c = (float)((((double)verts[3 * (int64_t)ia + k] + (double)verts[3 * (int64_t)ib + k]) + (double)verts[3 * (int64_t)ic + k]) / 3.0);
        points[3 * i + k] = c;
    }
}

__global__ void __launch_bounds__(TT) tnt_transform_kernel(int64_t n, const float* points, TMat T, float* out) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= n) return;
    const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
    const float ox = (float)(((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3]);
    const float oy = (float)(((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7]);
    const float oz = (float)(((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11]);
    out[3 * i] = ox; out[3 * i + 1] = oy; out[3 * i + 2] = oz;
}

// ---- rule 2: the crop volume -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TT) tnt_crop_kernel(int64_t n, const float* __restrict__ points, int axis, double axis_min, double axis_max, int nv,
                                                      const double* __restrict__ polygon, uint8_t* __restrict__ mask) {
    __shared__ double poly[2 * SURFEL_TNT_MAX_POLYGON];
    for (int k = threadIdx.x; k < 2 * nv; k += TT) poly[k] = polygon[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= n) return;
    const double p0 = (double)points[3 * i], p1 = (double)points[3 * i + 1], p2 = (double)points[3 * i + 2];
    const double pw = axis == 0 ? p0 : (axis == 1 ? p1 : p2);
    const double pu = axis == 0 ? p1 : p0;
    const double pv = axis == 2 ? p1 : p2;
    bool in = pw >= axis_min && pw <= axis_max;
    if (in) {
        int below = 0;
        bool on = false;
        for (int k = 0; k < nv; k++) {
            const int l = k + 1 < nv ? k + 1 : 0;
            const double au = poly[2 * k], av = poly[2 * k + 1], bu = poly[2 * l], bv = poly[2 * l + 1];
            if ((av < pv && bv >= pv) || (bv < pv && av >= pv)) {
                const double node = au + (pv - av) / (bv - av) * (bu - au);
                below += node < pu;
                on |= node == pu;
            }
        }
        in = (below & 1) && !on;
    }
    mask[i] = in;
}

// ---- rule 3: voxel down-sampling -------------------------------------------------------------------------------------------------------
struct TVox { double ox, oy, oz, voxel; };

// key = x | y << 21 | z << 42 of the point's cell; flags[0] |= 1 when an axis index falls outside [0, 2^21) (or is NaN)
__global__ void __launch_bounds__(TT) tnt_voxel_keys_kernel(int64_t n, const float* __restrict__ points, TVox v, uint32_t* __restrict__ lo,
                                                            uint32_t* __restrict__ hi, uint32_t* __restrict__ ka, uint32_t* __restrict__ va,
                                                            uint32_t* flags) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= n) return;
    const double cx = floor(((double)points[3 * i] - v.ox) / v.voxel), cy = floor(((double)points[3 * i + 1] - v.oy) / v.voxel),
                 cz = floor(((double)points[3 * i + 2] - v.oz) / v.voxel);
    const double lim = (double)(1 << AXIS_BITS);
    uint64_t key = 0;
    if (cx >= 0.0 && cy >= 0.0 && cz >= 0.0 && cx < lim && cy < lim && cz < lim)
        key = (uint64_t)cx | (uint64_t)cy << AXIS_BITS | (uint64_t)cz << (2 * AXIS_BITS);
    else
        atomicOr(flags, 1u);
    lo[i] = key_word(key, 0); hi[i] = key_word(key, 1);
    ka[i] = key_word(key, 0); va[i] = (uint32_t)i;      // (VoxelKey's word 0, from the register)
}

struct VoxelKey {      // the sort's key of a point: the two words of its cell key
    const uint32_t *lo, *hi;
    __device__ uint32_t operator()(uint32_t i, int word) const { return word ? hi[i] : lo[i]; }
};

__device__ inline uint64_t tnt_key_of(const uint32_t* lo, const uint32_t* hi, uint32_t i) { return (uint64_t)hi[i] << 32 | lo[i]; }

// head[j] = 1 when sorted slot j starts a cell; head[n] = 0 (so the exclusive scan of n + 1 words ends with the cell count)
__global__ void __launch_bounds__(TT) tnt_voxel_heads_kernel(int64_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                             const uint32_t* __restrict__ perm, uint32_t* __restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (j > n) return;
    head[j] = j < n && (j == 0 || tnt_key_of(lo, hi, perm[j]) != tnt_key_of(lo, hi, perm[j - 1]));
}

// The thread of a cell's first slot walks the cell: the sort is stable, so that is the input order.
__global__ void __launch_bounds__(TT) tnt_voxel_mean_kernel(int64_t n, const float* __restrict__ points, const uint32_t* __restrict__ lo,
                                                            const uint32_t* __restrict__ hi, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ seg, float* __restrict__ out, uint32_t* __restrict__ counts,
                                                            int32_t* __restrict__ cells) {
    const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (j >= n || seg[j + 1] == seg[j]) return;      // (the exclusive scan steps behind a head)
    const uint64_t key = tnt_key_of(lo, hi, perm[j]);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t k = j;
    for (; k < n && (k == j || seg[k + 1] == seg[k]); k++) {
        const int64_t p = perm[k];
        sx += (double)points[3 * p]; sy += (double)points[3 * p + 1]; sz += (double)points[3 * p + 2];
    }
    const double c = (double)(k - j);
    const int64_t s = seg[j];
    out[3 * s] = (float)(sx / c); out[3 * s + 1] = (float)(sy / c); out[3 * s + 2] = (float)(sz / c);
    if (counts) counts[s] = (uint32_t)(k - j);
    if (cells) {
        const uint32_t m = (1u << AXIS_BITS) - 1u;
        cells[3 * s] = (int32_t)(key & m); cells[3 * s + 1] = (int32_t)((key >> AXIS_BITS) & m); cells[3 * s + 2] = (int32_t)(key >> (2 * AXIS_BITS));
    }
}

// ---- rule 5: the correspondence sums ---------------------------------------------------------------------------------------------------
// partial[NS b + k] = the k-th sum over the elements b * TT + t + j * (blocks * TT)
__global__ void __launch_bounds__(TT) tnt_corr_sums_kernel(int64_t n, const float* __restrict__ source, const int32_t* __restrict__ index, int64_t nt,
                                                           const float* __restrict__ target, double* __restrict__ partial) {
    __shared__ double sh[NS * TT];
    double acc[NS] = {};
    for (int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x; i < n; i += (int64_t)gridDim.x * TT) {
        const int64_t j = index[i];
        if (j < 0 || j >= nt) continue;
        const double x0 = (double)source[3 * i], x1 = (double)source[3 * i + 1], x2 = (double)source[3 * i + 2];
        const double y0 = (double)target[3 * j], y1 = (double)target[3 * j + 1], y2 = (double)target[3 * j + 2];
        const double d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
        acc[0] += 1.0;
        acc[1] += x0; acc[2] += x1; acc[3] += x2;
        acc[4] += y0; acc[5] += y1; acc[6] += y2;
        acc[7] += y0 * x0; acc[8] += y0 * x1; acc[9] += y0 * x2;
        acc[10] += y1 * x0; acc[11] += y1 * x1; acc[12] += y1 * x2;
        acc[13] += y2 * x0; acc[14] += y2 * x1; acc[15] += y2 * x2;
        acc[16] += (x0 * x0 + x1 * x1) + x2 * x2;
        acc[17] += (d0 * d0 + d1 * d1) + d2 * d2;
    }
    block_tree_sum<TT>(acc, sh);      // sums in sh[k * TT]
    if (threadIdx.x < NS) partial[NS * blockIdx.x + threadIdx.x] = sh[threadIdx.x * TT];
}

__global__ void __launch_bounds__(TT) tnt_corr_sums_top_kernel(int nb, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double sh[NS * TT];
    double acc[NS] = {};
    for (int i = threadIdx.x; i < nb; i += TT) {
#pragma unroll
        for (int k = 0; k < NS; k++) acc[k] += partial[NS * i + k];
    }
    block_tree_sum<TT>(acc, sh);      // sums in sh[k * TT]
    if (threadIdx.x < NS) out[threadIdx.x] = sh[threadIdx.x * TT];
}

// ---- rule 8: the histogram ---------------------------------------------------------------------------------------------------------------
// Integer counters only: per-workgroup in LDS, then added to the global ones (exact in any order).  hist[nedges - 1] counts d < bound.
__global__ void __launch_bounds__(TT) tnt_hist_kernel(int64_t n, const float* __restrict__ dist, int nedges, const double* __restrict__ edges,
                                                      double bound, uint32_t* hist) {
    __shared__ double e[SURFEL_TNT_MAX_EDGES];
    __shared__ uint32_t cnt[SURFEL_TNT_MAX_EDGES];
    for (int k = threadIdx.x; k < nedges; k += TT) { e[k] = edges[k]; cnt[k] = 0u; }
    __syncthreads();
    const double first = e[0], last = e[nedges - 1];
    uint32_t below = 0;
    for (int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x; i < n; i += (int64_t)gridDim.x * TT) {
        const double d = (double)dist[i];
        below += d < bound;
        if (!(d >= first && d <= last)) continue;      // (NaN fails both)
        int a = 0, b = nedges - 1;                     // e[a] <= d, and d < e[b] or b is the last edge
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (e[m] <= d) a = m; else b = m;
        }
        atomicAdd(&cnt[a], 1u);
    }
    for (int o = 32; o > 0; o >>= 1) below += __shfl_down(below, o);
    if ((threadIdx.x & 63) == 0 && below) atomicAdd(&cnt[nedges - 1], below);
    __syncthreads();
    for (int k = threadIdx.x; k < nedges; k += TT)
        if (cnt[k]) atomicAdd(&hist[k], cnt[k]);
}

}  // namespace surfel

// ================================================================================================================ C ABI
using namespace surfel;

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, TT); }
constexpr int64_t TNT_MAX_POINTS = ((int64_t)1 << 31) - 1;
}  // namespace

extern "C" {

int surfel_tnt_mesh_cloud(int64_t V, int64_t F, const float* verts, const int32_t* tris, float* points, void* stream) {
    if (V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !tris) || (V + F > 0 && !points)) return api_fail(SURFEL_E_INVALID, "tnt_mesh_cloud: bad arguments");
    if (V > TNT_MAX_POINTS || F > TNT_MAX_POINTS) return api_fail(SURFEL_E_LIMIT, "tnt_mesh_cloud: more than 2^31 - 1 vertices or triangles");
    if (V + F == 0) return 0;
    hipLaunchKernelGGL(tnt_mesh_cloud_kernel, dim3(grid(V + F)), dim3(TT), 0, static_cast<hipStream_t>(stream), V, F, verts, tris, points);
    return launched("tnt_mesh_cloud_kernel");
}

int surfel_tnt_transform(int64_t n, const float* points, const double* T, float* out, void* stream) {
    if (n < 0 || !T || (n > 0 && (!points || !out))) return api_fail(SURFEL_E_INVALID, "tnt_transform: bad arguments");
    if (n == 0) return 0;
    TMat m;
    for (int k = 0; k < 12; k++) m.m[k] = T[k];
    hipLaunchKernelGGL(tnt_transform_kernel, dim3(grid(n)), dim3(TT), 0, static_cast<hipStream_t>(stream), n, points, m, out);
    return launched("tnt_transform_kernel");
}

int surfel_tnt_crop(int64_t n, const float* points, int axis, double axis_min, double axis_max, int nv, const double* polygon, uint8_t* mask,
                    void* stream) {
    if (n < 0 || axis < 0 || axis > 2 || nv < 0 || (nv > 0 && !polygon) || (n > 0 && (!points || !mask)))
        return api_fail(SURFEL_E_INVALID, "tnt_crop: bad arguments");
    if (nv > SURFEL_TNT_MAX_POLYGON) return api_fail(SURFEL_E_LIMIT, "tnt_crop: the polygon has more than SURFEL_TNT_MAX_POLYGON vertices");
    if (n == 0) return 0;
    hipLaunchKernelGGL(tnt_crop_kernel, dim3(grid(n)), dim3(TT), 0, static_cast<hipStream_t>(stream), n, points, axis, axis_min, axis_max, nv, polygon,
                       mask);
    return launched("tnt_crop_kernel");
}

int64_t surfel_tnt_voxel_down_sample(surfel_alloc_fn alloc, void* user, int64_t n, const float* points, double voxel, const double* origin,
                                     int64_t budget_bytes, float* out, uint32_t* counts, int32_t* cells, void* stream) {
    if (!alloc || n < 0 || !(voxel > 0.0) || !(voxel < INFINITY) || !origin || (n > 0 && (!points || !out)))
        return api_fail(SURFEL_E_INVALID, "tnt_voxel_down_sample: bad arguments");
    if (n >= ((int64_t)1 << 30) - 1) return api_fail(SURFEL_E_LIMIT, "tnt_voxel_down_sample: more than 2^30 - 2 points (the sort's limit)");
    const size_t sort_bytes = radix_sort_scratch_bytes((size_t)(n > 0 ? n : 1));
    const int64_t scan_words = ScanBuf::words(n + 1) + 1;      // heads | scan sums | flag
    if (6 * 4 * n + 4 * scan_words + (int64_t)sort_bytes > budget_bytes)
        return api_fail(SURFEL_E_LIMIT, "tnt_voxel_down_sample: the cloud exceeds the byte budget (raise the budget or down-sample the input)");
    if (n == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* lo = take<uint32_t>(alloc, user, n);
    uint32_t* hi = take<uint32_t>(alloc, user, n);
    SortPairs s(alloc, user, n);
    const ScanBuf head = take_scan(alloc, user, n + 1, 1);      // (n + 1 elements: the scan leaves the cell count in head[n])
    if (!lo || !hi || !s.ok() || !head.flags) return api_fail(SURFEL_E_ALLOC, "tnt_voxel_down_sample: allocator returned NULL");
    uint32_t* flag = head.total + 1;
    if (hipMemsetAsync(flag, 0, 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, "tnt_voxel_down_sample: memset", hipGetLastError());
    const TVox v{origin[0], origin[1], origin[2], voxel};
    hipLaunchKernelGGL(tnt_voxel_keys_kernel, dim3(grid(n)), dim3(TT), 0, st, n, points, v, lo, hi, s.ka, s.va, flag);
    const int bits[2] = {32, 3 * AXIS_BITS - 32};      // the 63-bit key by its 32-bit words
    if (int rc = sort_words(s, VoxelKey{lo, hi}, 2, bits, "tnt_voxel_down_sample: sort", st)) return rc;
    const uint32_t* perm = s.va;
    hipLaunchKernelGGL(tnt_voxel_heads_kernel, dim3(grid(n + 1)), dim3(TT), 0, st, n, lo, hi, perm, head.flags);
    head.scan(st);
    uint32_t host[2] = {0, 0};      // cell count, flag
    if (int rc = read_words("tnt_voxel_down_sample: copy", head.flags + n, &host[0], 1, st, false)) return rc;
    if (int rc = read_words("tnt_voxel_down_sample: copy", flag, &host[1], 1, st)) return rc;
    int rc = launched("tnt_voxel_heads_kernel");
    if (rc < 0) return rc;
    if (host[1])
        return api_fail(SURFEL_E_LIMIT, "tnt_voxel_down_sample: a cell index needs more than SURFEL_TNT_VOXEL_AXIS_BITS bits, or a coordinate is not finite "
                                        "or lies below the origin (raise the voxel size)");
    hipLaunchKernelGGL(tnt_voxel_mean_kernel, dim3(grid(n)), dim3(TT), 0, st, n, points, lo, hi, perm, head.flags, out, counts, cells);
    if (hipStreamSynchronize(st) != hipSuccess) return api_fail(SURFEL_E_HIP, "tnt_voxel_down_sample: synchronize", hipGetLastError());
    rc = launched("tnt_voxel_mean_kernel");
    return rc < 0 ? rc : (int64_t)host[0];
}

int surfel_tnt_corr_sums(surfel_alloc_fn alloc, void* user, int64_t n, const float* source, const int32_t* index, int64_t nt, const float* target,
                         double* sums, void* stream) {
    if (!alloc || n < 0 || nt < 0 || !sums || (n > 0 && (!source || !index)) || (nt > 0 && !target))
        return api_fail(SURFEL_E_INVALID, "tnt_corr_sums: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = (int)(grid(n) < (unsigned)TNT_SUM_BLOCKS ? grid(n) : (unsigned)TNT_SUM_BLOCKS);
    double* partial = take<double>(alloc, user, (int64_t)NS * nb);
    if (!partial) return api_fail(SURFEL_E_ALLOC, "tnt_corr_sums: allocator returned NULL");
    if (nb > 0) hipLaunchKernelGGL(tnt_corr_sums_kernel, dim3((unsigned)nb), dim3(TT), 0, st, n, source, index, nt, target, partial);
    hipLaunchKernelGGL(tnt_corr_sums_top_kernel, dim3(1), dim3(TT), 0, st, nb, partial, sums);
    return launched("tnt_corr_sums_top_kernel");
}

int surfel_tnt_histogram(int64_t n, const float* dist, int nedges, const double* edges, double bound, uint32_t* hist, void* stream) {
    if (n < 0 || nedges < 2 || !edges || !hist || (n > 0 && !dist)) return api_fail(SURFEL_E_INVALID, "tnt_histogram: bad arguments");
    if (nedges > SURFEL_TNT_MAX_EDGES) return api_fail(SURFEL_E_LIMIT, "tnt_histogram: more than SURFEL_TNT_MAX_EDGES edges");
    if (n > TNT_MAX_POINTS) return api_fail(SURFEL_E_LIMIT, "tnt_histogram: more than 2^31 - 1 distances");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(hist, 0, (size_t)nedges * 4, st) != hipSuccess) return api_fail(SURFEL_E_HIP, "tnt_histogram: memset", hipGetLastError());
    if (n == 0) return 0;
    const unsigned nb = grid(n) < (unsigned)TNT_HIST_BLOCKS ? grid(n) : (unsigned)TNT_HIST_BLOCKS;
    hipLaunchKernelGGL(tnt_hist_kernel, dim3(nb), dim3(TT), 0, st, n, dist, nedges, edges, bound, hist);
    return launched("tnt_hist_kernel");
}

}  // extern "C"
