/*
 * surfel_repair.h — C ABI of the mesh repair (REPAIR.md): cut the triangles on edges of more than two triangles or of two triangles
 * with the same direction, give every fan of a vertex a vertex of its own, find the border loops and close those of at most
 * max_hole_edges edges.  Part of libsurfel_hip.so (gfx950 only).  Same conventions as surfel_smooth.h: plain DEVICE pointers for every
 * array unless a comment says HOST, `stream` = hipStream_t as void*, scratch through the caller's surfel_alloc_fn, return >= 0 or a
 * negative SURFEL_E_* code (surfel_hip.h) with the message in surfel_last_error().
 *
 * Two steps, as the smoothing's adjacency and steps: surfel_repair_analyze runs rules 1-5 and the fill's bookkeeping and reports the
 * counts; the caller sizes the outputs exactly from them; surfel_repair_emit (the repaired mesh) and surfel_repair_loops (the border
 * loops) write them.  The state between the steps is a device workspace the caller owns: the arrays of surfel_repair_plan come from
 * the caller's allocator in surfel_repair_analyze and stay valid for as long as the caller keeps them; nothing is computed twice and
 * the library keeps no state of its own.  The input arrays are never written.
 *
 * Limits: 3 F < 2^31 and V + 3 F < 2^31; beyond them surfel_repair_analyze returns SURFEL_E_LIMIT before it calls the device or the
 * allocator.
 */
#ifndef SURFEL_REPAIR_H
#define SURFEL_REPAIR_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int64 entries of `counts`: kept triangles, dropped triangles (rule 1), cut triangles (rule 3), undirected edges of more than two kept
 * triangles, undirected edges of two kept triangles with the same direction, vertices added by the split (rule 4), border loops, border
 * edges of the split mesh, the longest loop's edges, filled loops, fill triangles, fill vertices (centroids), border edges left after
 * the fill, and the pointer-jumping rounds the loop labelling took. */
#define SURFEL_REPAIR_COUNTS 14
/* float entries of `stage_ms`: the half-edge sort, the cut and the twins, the fans and the split, the loops, the fill's bookkeeping */
#define SURFEL_REPAIR_STAGES 5

/* HOST structure that surfel_repair_analyze fills; its arrays are DEVICE memory from the caller's allocator, one allocation each. */
typedef struct surfel_repair_plan {
    int64_t V, F, max_hole_edges;
    int64_t survivors;          /* F_s: triangles left after rules 1 and 3 */
    int64_t split;              /* S: vertices the split adds, indices V .. V + S - 1 */
    int64_t border;             /* border half-edges of the split mesh */
    int64_t loops;
    int64_t fill_triangles, fill_vertices;
    int32_t* triangles;         /* [F_s, 3]: the survivors in their order, corners rewritten by the split */
    int32_t* triangle_source;   /* [F_s]: the input triangle of each */
    int32_t* split_source;      /* [S]: the vertex each split copy repeats */
    int32_t* half_edge;         /* [border]: the border half-edges 3 m + k of `triangles`, ascending */
    int32_t* loop;              /* [border]: the loop of each, loops numbered by their smallest half-edge */
    int32_t* position;          /* [border]: its distance from the loop's smallest half-edge along the loop */
    int32_t* lengths;           /* [loops] */
    uint32_t* fill_vertex;      /* [border]: the source vertex of the half-edge at fill_offset[loop] + position, filled loops only */
    uint32_t* fill_offset;      /* [loops]: exclusive sums over the filled loops of their edges, */
    uint32_t* triangle_offset;  /*          of their fill triangles, */
    uint32_t* centroid_offset;  /*          and of their centroids */
} surfel_repair_plan;

/*
 * Rules 1-5 of REPAIR.md on verts[V, 3] / tris[F, 3], and the sizes of rule 6 under max_hole_edges >= 0.  plan: HOST, written.
 * counts[SURFEL_REPAIR_COUNTS]: HOST.  stage_ms[SURFEL_REPAIR_STAGES]: HOST or NULL; when given, the stages are timed with events on
 * the stream.  Synchronises the stream.  The same bytes in every array of the plan on every run.
 */
int surfel_repair_analyze(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris,
                          int64_t max_hole_edges, surfel_repair_plan* plan, int64_t* counts, float* stage_ms, void* stream);

/*
 * The repaired mesh of a plan (rules 6 and 7): out_verts[V + S + C, 3] — the input's rows, the split copies, the centroids —,
 * out_colors likewise when colors is given (both NULL otherwise), out_tris[F_s + F_f, 3], vertex_source[V + S + C],
 * triangle_source[F_s + F_f], loop_lengths[loops].  verts and colors are the arrays the plan was made from.  Does not synchronise.
 */
int surfel_repair_emit(const surfel_repair_plan* plan, const float* verts, const float* colors, float* out_verts, float* out_colors,
                       int32_t* out_tris, int32_t* vertex_source, int32_t* triangle_source, int32_t* loop_lengths, void* stream);

/* The border loops of a plan (rule 5): half_edge, loop, position [border] and lengths [loops], copied out.  Does not synchronise. */
int surfel_repair_loops(const surfel_repair_plan* plan, int32_t* half_edge, int32_t* loop, int32_t* position, int32_t* lengths,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_REPAIR_H */
