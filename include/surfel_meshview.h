/*
 * surfel_meshview.h — C ABI of the mesh viewer (MESHVIEW.md), part of libsurfel_hip.so (gfx950 only): a visibility buffer of a triangle
 * mesh for a batch of views, angle-free vertex normals in fixed point, and the pass that shades a visibility buffer into 8-bit frames.
 * Same conventions as surfel_cull.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t as void*,
 * scratch through the caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Cameras as in surfel_cull.h: w2c[nviews, 12] (rows 0..2 of the OpenCV world-to-camera matrices, row-major),
 * intrinsics[n_intrinsics, 4] = (fx, fy, cx, cy) per view or once for all.
 *
 * The reference has no mesh renderer (its scripts/eval_tnt/cull_mesh.py renders depth only, through pyrender); nothing here replaces a
 * line of it.
 */
#ifndef SURFEL_MESHVIEW_H
#define SURFEL_MESHVIEW_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_cull.h"
#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The key of a pixel no triangle hit: (fp32 +inf bits) << 32 | 0xffffffff. */
#define SURFEL_MESHVIEW_EMPTY 0x7f800000ffffffffull
/* surfel_meshview_shade's `mode`. */
#define SURFEL_MESHVIEW_SHADED 0
#define SURFEL_MESHVIEW_NORMAL 1
#define SURFEL_MESHVIEW_COLOR 2
/* The largest supersampling factor of surfel_meshview_shade. */
#define SURFEL_MESHVIEW_MAX_SSAA 4
/* The fixed-point scale of a unit face normal's component in surfel_meshview_vertex_normals' sums: 2^20. */
#define SURFEL_MESHVIEW_NORMAL_SCALE 1048576

/*
 * key[nviews, H, W] <- per pixel (fp32 bits of z) << 32 | triangle index of the nearest hit under the cameras, sample rule, hit rule and
 * skip rules of surfel_cull_mesh_depth (CULL.md §Depth rules 1-6; the same set-up, pixel test, size classes, queue and chunking), or
 * SURFEL_MESHVIEW_EMPTY.  A 64-bit integer minimum: the nearest depth wins and, among triangles that reach the same depth bits, the
 * lowest index; the same bits on every run.  The depth half equals surfel_cull_mesh_depth's image bit for bit (0 there is +inf here).
 * F < 2^32 - 1 (more: SURFEL_E_LIMIT; the other limits are surfel_cull_mesh_depth's).  small_pixels, stage_ms (HOST, may be NULL;
 * SURFEL_CULL_STAGES floats), scratch and the return value as in surfel_cull_mesh_depth.
 */
int64_t surfel_meshview_visibility(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, int nviews,
                                   const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, float znear, float zfar,
                                   int small_pixels, uint64_t* key, float* stage_ms, void* stream);

/*
 * normals[V, 3] <- the normalised sum of the unit face normals of the triangles around every vertex, (0, 0, 0) where the sum is zero.
 * Per triangle fn = (p1 - p0) x (p2 - p0) in fp32, u = fn / sqrt(fn . fn), q = (int64) rintf(u * 2^20) is added to acc[V, 3] (int64,
 * zeroed by the call) at its three vertices with 64-bit integer atomics: acc holds the same bits on every run.  A triangle with an
 * index outside [0, V), a non-finite fn or length, or length zero adds nothing.  Then normals[v] = (float) acc[v] / sqrt of its squared
 * length (MESHVIEW.md §Vertex normals gives the order).  verts[V, 3], tris[F, 3].
 */
int surfel_meshview_vertex_normals(int64_t V, int64_t F, const float* verts, const int32_t* tris, int64_t* acc, float* normals, void* stream);

/*
 * out[nviews, H, W, 3] (uint8) <- the frames of a visibility buffer key[nviews, ssaa H, ssaa W] that surfel_meshview_visibility wrote
 * for the same mesh, w2c and intrinsics (the intrinsics of the ssaa H x ssaa W sample grid).  One thread per output pixel; the ssaa x ssaa
 * float samples of a pixel are summed in row-major order, background samples included, multiplied by 1 / (ssaa ssaa) and quantised as
 * surfel_vis_quantize does (scale 1, bias 0).  A sample whose key is empty, or names a triangle the depth rule would skip, has the
 * colour (bg_r, bg_g, bg_b).  mode: SURFEL_MESHVIEW_SHADED (albedo (0.3 + 0.7 max(0, n . -d / |d|))), _NORMAL (world-space normal
 * 0.5 + 0.5), _COLOR (interpolated vertex colours).  colors[V, 3] may be NULL: grey 0.8.  normals[V, 3] (world space, from
 * surfel_meshview_vertex_normals) may be NULL: flat shading.  MESHVIEW.md §Shading writes out every operation and its order.
 */
int surfel_meshview_shade(int64_t V, int64_t F, const float* verts, const int32_t* tris, const float* colors, const float* normals, int nviews,
                          const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, int ssaa, const uint64_t* key, int mode,
                          float bg_r, float bg_g, float bg_b, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_MESHVIEW_H */
