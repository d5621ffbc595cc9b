/*
 * surfel_smooth.h — C ABI of the mesh smoothing (SMOOTH.md): the vertex adjacency of a triangle mesh as a CSR with the number of
 * triangles on every edge, and Laplacian / Taubin filter steps over it.  Part of libsurfel_hip.so (gfx950 only).  Same conventions as
 * surfel_mesh.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t as void*, scratch through the
 * caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in surfel_last_error().  Output
 * arrays are sized by the caller from the input's counts; the library reports how much of them it filled.
 *
 * Limits: V < 2^31 and 6 F < 2^31; beyond them an entry returns SURFEL_E_LIMIT before it calls the device or the allocator.
 */
#ifndef SURFEL_SMOOTH_H
#define SURFEL_SMOOTH_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int64 entries of `counts`: kept triangles, dropped triangles, directed edges (E2), border edges (undirected, one triangle),
 * non-manifold edges (undirected, more than two triangles), boundary vertices, isolated vertices (degree 0), the largest degree. */
#define SURFEL_SMOOTH_COUNTS 8
/* Bits of `flags`: the vertex has an incident edge of one triangle; one of more than two triangles; no incident edge at all. */
#define SURFEL_SMOOTH_BOUNDARY 1
#define SURFEL_SMOOTH_NONMANIFOLD 2
#define SURFEL_SMOOTH_ISOLATED 4
/* `mode` of surfel_smooth_steps: every neighbour counts; boundary vertices are pinned; a boundary vertex averages its neighbours
 * across border edges only. */
#define SURFEL_SMOOTH_FREE 0
#define SURFEL_SMOOTH_FIXED 1
#define SURFEL_SMOOTH_CURVE 2

/*
 * The adjacency of verts[V, 3] / tris[F, 3] (SMOOTH.md §Rules 1-3).  A triangle that names an index outside [0, V), repeats an index
 * or names a vertex with a non-finite coordinate is dropped; every other one gives its six directed vertex pairs.  offsets[V + 1]: row
 * v of the CSR is [offsets[v], offsets[v + 1]); neighbors[6 F] and multiplicity[6 F]: the first E2 entries are written — the row's
 * neighbours in ascending order and, beside each, the number of kept triangles on that edge; flags[V]: SURFEL_SMOOTH_* bits.
 * counts[SURFEL_SMOOTH_COUNTS]: HOST.  Returns E2.  Synchronises the stream.  The same bytes on every run.
 */
int64_t surfel_smooth_adjacency(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                                int32_t* offsets, int32_t* neighbors, int32_t* multiplicity, uint8_t* flags, int64_t* counts, void* stream);

/*
 * nsteps filter steps over attr_in[V, 3] (SMOOTH.md §Rules 4): step k moves every vertex by factors[k] (HOST, nsteps doubles) towards
 * the mean of its row, summed in fp64 in the row's order; a vertex with an empty row, and under SURFEL_SMOOTH_FIXED a boundary vertex,
 * keeps its bits.  The steps alternate between scratch[V, 3] (may be NULL when nsteps < 2) and attr_out[V, 3], and the last one writes
 * attr_out; attr_in is only read, and nsteps = 0 copies it.  Does not synchronise.
 */
int surfel_smooth_steps(int64_t V, const int32_t* offsets, const int32_t* neighbors, const int32_t* multiplicity, const uint8_t* flags,
                        int mode, int nsteps, const double* factors, const float* attr_in, float* scratch, float* attr_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_SMOOTH_H */
