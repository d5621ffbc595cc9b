// mesh_topology.h — what the mesh modules agree on about a triangle list: the ends of a half-edge, and rule 1 of SMOOTH.md (REPAIR.md
// adopts it) with its kernel and host pass, so that mesh_smooth.hip and mesh_repair.hip keep the same triangles.
#pragma once
#include "side_util.h"

namespace surfel {

// half-edge h = 3 t + k of triangle t runs from its corner k to its corner (k + 1) % 3
__device__ __forceinline__ void half_edge_ends(const int32_t* __restrict__ tris, uint32_t h, uint32_t* a, uint32_t* b) {
    const uint32_t t = h / 3u, k = h - 3u * t, k1 = k == 2u ? 0u : k + 1u;
    *a = (uint32_t)tris[3 * (int64_t)t + k];
    *b = (uint32_t)tris[3 * (int64_t)t + k1];
}

// rule 1: a triangle is kept when it has three distinct indices in [0, V) and finite vertices
__device__ __forceinline__ bool triangle_kept(int64_t t, int64_t V, const float* __restrict__ verts, const int32_t* __restrict__ tris) {
    const int32_t idx[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    bool ok = idx[0] != idx[1] && idx[1] != idx[2] && idx[0] != idx[2];
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && idx[k] >= 0 && idx[k] < V;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; k++)
            ok = ok && __builtin_isfinite(verts[3 * (int64_t)idx[k]]) && __builtin_isfinite(verts[3 * (int64_t)idx[k] + 1]) &&
                 __builtin_isfinite(verts[3 * (int64_t)idx[k] + 2]);
    }
    return ok;
}

constexpr int KEEP_T = 256;      // threads per workgroup

// (static: each file that includes this has its own copy, as it must without relocatable device code)
static __global__ void __launch_bounds__(KEEP_T) mesh_keep_kernel(int64_t F, int64_t V, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           uint32_t* __restrict__ keep) {
    const int64_t t = (int64_t)blockIdx.x * KEEP_T + threadIdx.x;
    if (t < F) keep[t] = triangle_kept(t, V, verts, tris) ? 1u : 0u;
}

// keep: the scanned rule-1 flags of the F triangles, *kept their sum (the caller sizes its sort by it); an empty ScanBuf and 0 for a mesh
// without a vertex or a triangle.  One launch, the scan, one read with its wait.
inline int mesh_keep(const char* what, surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                     ScanBuf* keep, uint32_t* kept, hipStream_t st) {
    *keep = ScanBuf(); *kept = 0;
    if (F <= 0 || V <= 0) return 0;
    *keep = take_scan(alloc, user, F);
    if (!keep->flags) return api_fail(SURFEL_E_ALLOC, what);
    hipLaunchKernelGGL(mesh_keep_kernel, dim3(blocks_for(F, KEEP_T)), dim3(KEEP_T), 0, st, F, V, verts, tris, keep->flags);
    keep->scan(st);
    if (int rc = read_words(what, keep->total, kept, 1, st)) return rc;
    return launched("mesh_keep_kernel");
}

}  // namespace surfel
