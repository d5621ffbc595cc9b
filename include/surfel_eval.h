/*
 * surfel_eval.h — C ABI of the DTU-style mesh evaluation (EVAL.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_mesh.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t as
 * void*, scratch through the caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().
 *
 * What each entry replaces in the reference (CPU numpy / scikit-learn / scikit-image there):
 *   surfel_eval_sample_count / _emit   scripts/eval_dtu/eval.py:48-71 (points on every triangle, multiprocessing pool)
 *   surfel_eval_grid_build / _thin     eval.py:86-94 (radius_neighbors + the sequential thinning loop)
 *   surfel_eval_obs_mask               eval.py:98-110 (bounding box and observation mask)
 *   surfel_eval_above_plane            eval.py:126-130
 *   surfel_eval_nearest                eval.py:118-134 (KD-tree kneighbors)
 *   surfel_eval_mean_below             eval.py:122, :134 and scripts/eval_tnt/evaluation.py:173-190 (the counts)
 *   surfel_eval_dilate_masks / _cull_vertices
 *                                      scripts/eval_dtu/evaluate_single_scene.py:57-91
 */
#ifndef SURFEL_EVAL_H
#define SURFEL_EVAL_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest n1, n2 of one triangle (EVAL.md rule 1); a triangle that wants more is a SURFEL_E_LIMIT. */
#define SURFEL_EVAL_MAX_N 4096

/*
 * Uniform grid over a cloud.  The caller sets the first block and zeroes the rest; surfel_eval_grid_build writes the rest.
 * Cell of a point p: c = clamp((int)((p - origin) / cell), 0, dims - 1) per axis in fp32, key = c.x + dims[0] * (c.y + dims[1] * c.z).
 * sorted[i] = (p - origin, bits of the point's rank) of the i-th point in key order (stable: input order inside a cell);
 * order[i] = its index in the input; ranges[2 key] .. ranges[2 key + 1] = [first, last + 1) of the cell's points in `sorted`
 * (0, 0 when empty).
 */
typedef struct surfel_eval_grid {
    float origin[3];
    float cell;
    int dims[3];
    int64_t budget_bytes;         /* ranges + sorted + order + sort buffers may not exceed this: SURFEL_E_LIMIT before allocating */
    /* written by the library */
    int64_t n;
    float* sorted;                /* [n * 4] */
    uint32_t* order;              /* [n] */
    uint32_t* ranges;             /* [2 * dims product] */
} surfel_eval_grid;

/*
 * Rule 1, pass 1.  offsets[F] <- samples of every triangle, then their exclusive scan (so triangle t owns
 * [offsets[t], offsets[t + 1]) and the last one ends at the total); scan_scratch from surfel_alloc_fn.  Synchronises.  Returns the
 * total, or SURFEL_E_LIMIT when a triangle exceeds SURFEL_EVAL_MAX_N, the total exceeds 2^31 - 1 - V, or 12 * (V + total) bytes
 * exceed budget_bytes (nothing but the scan scratch was allocated by then).
 */
int64_t surfel_eval_sample_count(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, double density,
                                 int64_t budget_bytes, uint32_t* offsets, void* stream);
/* Rule 1, pass 2.  points[V + total, 3] <- the V vertices, then every triangle's samples at V + offsets[t]. */
int surfel_eval_sample_emit(int64_t V, int64_t F, const float* verts, const int32_t* tris, double density, const uint32_t* offsets, int64_t total,
                            float* points, void* stream);

/* Sorts n points[n, 3] into g's cells.  rank[n] (NULL: the point's index) is the point's place in the thinning order. */
int surfel_eval_grid_build(surfel_alloc_fn alloc, void* user, surfel_eval_grid* g, int64_t n, const float* points, const uint32_t* rank,
                           void* stream);
/*
 * Rule 3 on a built grid whose cell edge is at least density * (1 + 2^-10).  keep[n] (uint8, input order) <- 1 for the kept points.
 * rounds_out (HOST, may be NULL) <- launches it took.  Synchronises.
 */
int surfel_eval_thin(surfel_alloc_fn alloc, void* user, const surfel_eval_grid* g, float density, uint8_t* keep, int* rounds_out, void* stream);

/*
 * Rule 4.  bb (HOST, 6 floats: BB[0], BB[1]); obs_mask uint8 [dims[0], dims[1], dims[2]].  inbound[n], in_obs[n] (uint8) <- the two
 * tests (in_obs implies inbound).
 */
int surfel_eval_obs_mask(int64_t n, const float* points, const float* bb, float patch, double res, const uint8_t* obs_mask, const int* dims,
                         uint8_t* inbound, uint8_t* in_obs, void* stream);
/* above[n] (uint8) <- plane . (p, 1) > 0 in fp64; plane: HOST, 4 doubles. */
int surfel_eval_above_plane(int64_t n, const float* points, const double* plane, uint8_t* above, void* stream);

/*
 * Rule 5.  dist[nq] <- distance from queries[nq, 3] to the nearest point of g's cloud, +inf when it is not below max_dist (or the
 * cloud is empty); index[nq] (may be NULL) <- that point's index in the cloud's input order, -1 for none.  max_dist may be +inf.
 */
int surfel_eval_nearest(surfel_alloc_fn alloc, void* user, const surfel_eval_grid* g, int64_t nq, const float* queries, float max_dist,
                        float* dist, int32_t* index, void* stream);
/* out (2 doubles) <- sum and count of the distances below `bound`, in fp64 in a fixed order (the same bits on every run). */
int surfel_eval_mean_below(surfel_alloc_fn alloc, void* user, int64_t n, const float* dist, float bound, double* out, void* stream);

/* Rule 7.  out[V, H, W] (uint8 0 / 1) <- masks[V, H, W] != 0 dilated by the disk dx^2 + dy^2 <= r^2, 0 <= r <= 254. */
int surfel_eval_dilate_masks(surfel_alloc_fn alloc, void* user, int V, int H, int W, const uint8_t* masks, int r, uint8_t* out, void* stream);
/* Rule 7.  proj[nviews, 12]: rows 0..2 of K . w2c per view (fp32, row-major 3x4).  keep[n] (uint8) <- the vertex survives every view. */
int surfel_eval_cull_vertices(int64_t n, const float* verts, int nviews, const float* proj, int H, int W, const uint8_t* dilated, uint8_t* keep,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_EVAL_H */
