/*
 * surfel_cull.h — C ABI of the view culling of a mesh (CULL.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_eval_tnt.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t as
 * void*, scratch through the caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().
 *
 * What each entry replaces in the reference (line numbers of scripts/eval_tnt/cull_mesh.py):
 *   surfel_cull_mesh_depth     :17-66 (extract_depth_from_mesh: pyrender / OpenGL depth images of the mesh, DEPTH_ONLY | SKIP_CULL_FACES)
 *   surfel_cull_visibility     :96-182 (Mesher.point_masks: in how many views a vertex lies in the frustum and not behind the depth image)
 *
 * Cameras are OpenCV (x right, y down, z forward): w2c[nviews, 12] holds rows 0..2 of every world-to-camera matrix, row-major;
 * intrinsics[n_intrinsics, 4] holds (fx, fy, cx, cy) per view (n_intrinsics == nviews) or once for all (n_intrinsics == 1).
 */
#ifndef SURFEL_CULL_H
#define SURFEL_CULL_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A triangle whose clamped bounding box holds at most this many pixels is rasterised by the lane that set it up; a larger one is queued
 * for the workgroup rasteriser (CULL.md §Work distribution). */
#define SURFEL_CULL_SMALL_PIXELS 32
/* Most views of one call (they share a launch as the grid's second dimension); more is a SURFEL_E_LIMIT. */
#define SURFEL_CULL_MAX_VIEWS 65535
/* Floats surfel_cull_mesh_depth writes to stage_ms: the small-class launches (set-up, small triangles, queue append), the large-class
 * launches, the rest (initialisation and resolve). */
#define SURFEL_CULL_STAGES 3

/*
 * depth[nviews, H, W] <- per pixel (x, y) the smallest camera-space z with znear <= z <= zfar over all triangles hit by the ray
 * d = ((x - cx) / fx, (y - cy) / fy, 1), both faces counting; 0 where nothing is hit.  With camera-space vertices v0, v1, v2:
 * n0 = v1 x v2, n1 = v2 x v0, n2 = v0 x v1, det = v0 . n0; the ray hits iff det != 0, every ni . d is zero or has the sign of det and
 * ((n0 + n1) + n2) . d / det > 0; then z = det / (((n0 + n1) + n2) . d).  All in fp32.  A triangle with an index outside [0, V), a
 * non-finite coordinate or det == 0 is skipped.  The same bits on every run (an integer minimum over positive fp32 bit patterns).
 * verts[V, 3], tris[F, 3]; znear > 0.  small_pixels: the class threshold, < 0 for SURFEL_CULL_SMALL_PIXELS (a test argument: the image does
 * not depend on it).  Scratch: 4 B x nviews x min(F, 2^18) for the queues.  stage_ms: HOST, may be NULL; when given, the call times its
 * launches with events, synchronises and returns the number of (view, triangle) pairs that went through the large class.  Otherwise
 * returns 0 and does not synchronise.
 */
int64_t surfel_cull_mesh_depth(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, int nviews,
                               const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, float znear, float zfar,
                               int small_pixels, float* depth, float* stage_ms, void* stream);

/*
 * counts[N] (int32) += the number of views in which the point is in the frustum and in front of the depth image, as Mesher.point_masks
 * counts them (CULL.md §Visibility gives the fp32 operations and their order).  points[N, 3]; depth[nviews, H, W]; H, W >= 2.  A view in
 * which the point has z <= 0 or a non-finite projection does not count and reads nothing.
 */
int surfel_cull_visibility(int64_t N, const float* points, int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W,
                           const float* depth, float eps, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_CULL_H */
