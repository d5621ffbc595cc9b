/*
 * surfel_simplify.h — C ABI of the mesh simplification by quadric vertex clustering (SIMPLIFY.md), part of libsurfel_hip.so (gfx950
 * only).  Same conventions as surfel_mesh.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t
 * as void*, scratch through the caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Output arrays are sized by the caller from the input's counts; the library reports how much of them it filled.
 *
 * The grid of every entry: `bounds` (HOST, 6 floats: the component-wise minimum and maximum of the finite vertices, as
 * surfel_simplify_bounds writes them; NULL: the entry computes them itself), `origin` (HOST, 3 floats; NULL: the minimum of `bounds`)
 * and `cell`, the fp32 edge length.  Per axis the cell index of a vertex is floor((v - origin) / cell) in fp32; it must lie in
 * [0, 2^SURFEL_SIMPLIFY_AXIS_BITS) for every finite vertex, otherwise the entry returns SURFEL_E_LIMIT before it writes anything.
 * A vertex with a non-finite coordinate belongs to no cluster; a triangle that names one, or an index outside [0, V), is dropped.
 * Every entry synchronises the stream.
 */
#ifndef SURFEL_SIMPLIFY_H
#define SURFEL_SIMPLIFY_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bits of a cell index per axis: the cell key (z << 42 | y << 21 | x) has 63. */
#define SURFEL_SIMPLIFY_AXIS_BITS 21
/* int64 entries of `counts`: occupied cells, vertices out, triangles out, dropped triangles (rule 1), collapsed triangles (a repeated
 * cluster), duplicate triangles (the same rotated triple as an earlier one). */
#define SURFEL_SIMPLIFY_COUNTS 6
/* Floats of `stage_ms`: keys (bounds, cell keys), sorts (vertex sort, run heads, numbering), sums and solve, remap and dedupe,
 * compaction. */
#define SURFEL_SIMPLIFY_STAGES 5

/*
 * bounds[0..2] <- minimum, bounds[3..5] <- maximum of the vertices whose three coordinates are finite (integer atomics on an
 * order-preserving key: the same bits on every run).  Returns 1, or 0 when no vertex is finite (bounds <- 0).  verts[V, 3].
 */
int surfel_simplify_bounds(surfel_alloc_fn alloc, void* user, int64_t V, const float* verts, float* bounds, void* stream);

/*
 * cluster[V] <- per vertex the number of its cell among the occupied cells in key order, -1 for a vertex with a non-finite coordinate.
 * Returns the number of occupied cells.
 */
int64_t surfel_simplify_clusters(surfel_alloc_fn alloc, void* user, int64_t V, const float* verts, const float* bounds, const float* origin,
                                 float cell, int32_t* cluster, void* stream);

/*
 * What surfel_simplify_mesh would leave at this grid, without the sums, the solve and the outputs: counts[SURFEL_SIMPLIFY_COUNTS] (HOST;
 * the entry "vertices out" stays 0).  Returns the number of triangles out.  tris[F, 3].
 */
int64_t surfel_simplify_count(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                              const float* bounds, const float* origin, float cell, int64_t* counts, void* stream);

/*
 * The simplified mesh (SIMPLIFY.md §Rules): one vertex per occupied cell that a surviving triangle uses, at the clamped minimiser of
 * the cell's plane quadrics regularised towards the mean of its members (lam: the regulariser as a share of the quadric's trace), the
 * members' mean colour; the triangles mapped through the cells, without those that repeat a cell and without later copies of the same
 * rotated triple.  colors[V, 3] and colors_out may both be NULL.  cluster[V] as surfel_simplify_clusters (may be NULL);
 * cluster_vertex[V] (may be NULL): its first counts[0] entries <- the output vertex of every occupied cell, -1 for a cell no surviving
 * triangle uses.  verts_out[V, 3], colors_out[V, 3], tris_out[F, 3]: the first counts[1] / counts[2] rows are written.  counts: HOST.
 * stage_ms: HOST, SURFEL_SIMPLIFY_STAGES floats, may be NULL.  The same bytes on every run.
 */
int surfel_simplify_mesh(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const float* colors, const int32_t* tris,
                         const float* bounds, const float* origin, float cell, double lam, int32_t* cluster, int32_t* cluster_vertex,
                         float* verts_out, float* colors_out, int32_t* tris_out, int64_t* counts, float* stage_ms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_SIMPLIFY_H */
