/*
 * surfel_eval_tnt.h — C ABI of the Tanks-and-Temples-style mesh evaluation (TNT.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_eval.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t as
 * void*, scratch through the caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  The neighbour search of the ICP loop and of the scoring is surfel_eval_grid_build / surfel_eval_nearest
 * (surfel_eval.h); nothing here repeats it.
 *
 * What each entry replaces in the reference (CPU numpy / Open3D / trimesh there; line numbers of scripts/eval_tnt/):
 *   surfel_tnt_mesh_cloud          run.py:94-108 (every vertex, then the centroid of every triangle)
 *   surfel_tnt_transform           registration.py:119, evaluation.py:76 (PointCloud.transform) and the moved source of every ICP
 *                                  iteration (registration.py:152-160, :191-199)
 *   surfel_tnt_crop                run.py:153, registration.py:120, evaluation.py:78,89 (SelectionPolygonVolume.crop_point_cloud)
 *   surfel_tnt_voxel_down_sample   registration.py:123, evaluation.py:83,93 (PointCloud.voxel_down_sample)
 *   surfel_tnt_corr_sums           registration.py:152-160, :191-199 (the correspondence sums behind registration_icp's fitness,
 *                                  inlier_rmse and TransformationEstimationPointToPoint(True))
 *   surfel_tnt_histogram           evaluation.py:183-196 (the two counts below the threshold and numpy.histogram)
 */
#ifndef SURFEL_EVAL_TNT_H
#define SURFEL_EVAL_TNT_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most vertices of a crop polygon and most edges of a histogram (both are staged in LDS); more is a SURFEL_E_LIMIT. */
#define SURFEL_TNT_MAX_POLYGON 1024
#define SURFEL_TNT_MAX_EDGES 2048
/* Bits of a voxel's cell index per axis (TNT.md rule 3); a cloud that needs more is a SURFEL_E_LIMIT. */
#define SURFEL_TNT_VOXEL_AXIS_BITS 21
/* Doubles surfel_tnt_corr_sums writes: count, sum x (3), sum y (3), sum y x^T (9, row-major: y's component first), sum |x|^2, sum d^2. */
#define SURFEL_TNT_CORR_SUMS 18

/*
 * Rule 1.  points[V + F, 3] <- the V vertices, then the centroid of every triangle in triangle order: ((a + b) + c) / 3 in fp64,
 * stored as fp32.  A triangle with an index outside [0, V) gives NaN.
 */
int surfel_tnt_mesh_cloud(int64_t V, int64_t F, const float* verts, const int32_t* tris, float* points, void* stream);

/*
 * out[n, 3] <- fp32(T . (p, 1)) for every point of points[n, 3]; T: HOST, 16 doubles, row-major 4 x 4 whose last row is (0, 0, 0, 1).
 * Per row ((T0 x + T1 y) + T2 z) + T3 in fp64.  out may be points.
 */
int surfel_tnt_transform(int64_t n, const float* points, const double* T, float* out, void* stream);

/*
 * Rule 2.  mask[n] (uint8) <- the point lies inside the volume: axis_min <= p.w <= axis_max and inside the polygon by the crossing
 * rule, all in fp64.  axis: 0 X, 1 Y, 2 Z, the orthogonal axis w; polygon[nv, 2] (fp64): the (u, v) of every vertex, (u, v) = (Y, Z),
 * (X, Z), (X, Y) for w = X, Y, Z.  nv > SURFEL_TNT_MAX_POLYGON: SURFEL_E_LIMIT.
 */
int surfel_tnt_crop(int64_t n, const float* points, int axis, double axis_min, double axis_max, int nv, const double* polygon, uint8_t* mask,
                    void* stream);

/*
 * Rule 3.  Cell of a point: floor((p - origin) / voxel) per axis in fp64 (origin: HOST, 3 doubles; the caller passes the cloud's minimum
 * corner - voxel / 2).  out[m, 3] <- the mean of every occupied cell's points (summed in fp64 in input order, divided, stored as fp32)
 * in ascending (z, y, x) cell order; counts[m] (may be NULL) <- the cell's points; cells[m, 3] (int32, may be NULL) <- its index.  out,
 * counts and cells have room for n rows.  Synchronises.  Returns m, or SURFEL_E_LIMIT when an axis needs more than
 * SURFEL_TNT_VOXEL_AXIS_BITS bits (or a coordinate is not finite or lies below the origin), n exceeds 2^30 - 2, or the keys, the sort
 * buffers and the scan exceed budget_bytes (nothing was allocated by then).
 */
int64_t surfel_tnt_voxel_down_sample(surfel_alloc_fn alloc, void* user, int64_t n, const float* points, double voxel, const double* origin,
                                     int64_t budget_bytes, float* out, uint32_t* counts, int32_t* cells, void* stream);

/*
 * Rule 5.  sums[SURFEL_TNT_CORR_SUMS] (fp64) <- over the i with index[i] >= 0, x = source[i], y = target[index[i]], d = x - y, all in fp64:
 * the count, sum x, sum y, sum y x^T, sum |x|^2, sum |d|^2 — accumulated in a fixed order (the same bits on every run).
 * A pair whose index is not below nt is skipped.
 */
int surfel_tnt_corr_sums(surfel_alloc_fn alloc, void* user, int64_t n, const float* source, const int32_t* index, int64_t nt, const float* target,
                         double* sums, void* stream);

/*
 * Rule 8.  hist[nedges] (uint32) <- numpy.histogram(dist, edges) in its first nedges - 1 words (bin i: edges[i] <= d < edges[i + 1], the
 * last bin also takes d == edges[nedges - 1]; larger values, +inf and NaN are dropped), and the number of d < bound (fp64) in the last
 * word.  edges[nedges] (fp64) ascending, 2 <= nedges <= SURFEL_TNT_MAX_EDGES; n <= 2^31 - 1.
 */
int surfel_tnt_histogram(int64_t n, const float* dist, int nedges, const double* edges, double bound, uint32_t* hist, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_EVAL_TNT_H */
