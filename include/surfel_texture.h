/*
 * surfel_texture.h — C ABI of the mesh texturing (TEXTURE.md), part of libsurfel_hip.so (gfx950 only): a triangle atlas (one right
 * isosceles patch per triangle), the kernel that bakes a batch of views into it, the pass that resolves the accumulator into 8-bit
 * texels, and the pass that shades a visibility buffer with the atlas.
 * Same conventions as surfel_cull.h: plain DEVICE pointers for every array unless a comment says HOST, `stream` = hipStream_t as void*,
 * scratch through the caller's surfel_alloc_fn, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error(); limits are refused before anything is written.  Cameras as in surfel_cull.h: w2c[nviews, 12],
 * intrinsics[n_intrinsics, 4] = (fx, fy, cx, cy) per view or once for all.
 *
 * Texture coordinates are in TEXELS, texel-centre convention: texel (x, y) of atlas[Ha, Wa] has its centre at u = x, v = y; a bilinear
 * fetch at (u, v) reads the texels x0 = floor(u), x0 + 1, y0 = floor(v), y0 + 1 (surfel_texture.obj_uv turns them into OBJ's vt).
 *
 * The reference has no texturing; nothing here replaces a line of it.
 */
#ifndef SURFEL_TEXTURE_H
#define SURFEL_TEXTURE_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_cull.h"
#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Patch classes: class c has legs of n = 2^(c + SURFEL_TEXTURE_MIN_LOG2) texels, c = 0 .. SURFEL_TEXTURE_CLASSES - 1 (n = 4 .. 128). */
#define SURFEL_TEXTURE_CLASSES 6
#define SURFEL_TEXTURE_MIN_LOG2 2
/* A cell (two patches) of legs n is a square of n + SURFEL_TEXTURE_PAD texels. */
#define SURFEL_TEXTURE_PAD 4
/* The largest atlas width and height. */
#define SURFEL_TEXTURE_MAX_SIDE 16384
/* Ints per class in the band table: y0 (the band's first texel row), cells per row, first (the band's first slot in `order`), count
 * (its triangles).  table[SURFEL_TEXTURE_CLASSES, SURFEL_TEXTURE_BAND_INTS] (HOST, int32), row c for class c. */
#define SURFEL_TEXTURE_BAND_INTS 4
/* surfel_texture_bake's and _resolve's `blend`. */
#define SURFEL_TEXTURE_AVERAGE 0
#define SURFEL_TEXTURE_BEST 1
#define SURFEL_TEXTURE_MAX_POWER 8

/*
 * cls[F] (int32) <- the class of every triangle, -1 for a triangle that gets no patch: an index outside [0, V), a non-finite
 * coordinate, or a face normal (p1 - p0) x (p2 - p0) whose fp32 length is zero or not finite.  With L the fp32 length of the longest
 * edge, the class is the smallest c with (float) 2^(c + 2) >= L * density, clamped to 0 .. 5 (integer powers compared with the fp32
 * product; a NaN product gives class 0).  counts[SURFEL_TEXTURE_CLASSES] (HOST, int64) <- the triangles per class; the call
 * synchronises.  Scratch: 32 bytes.  density > 0 and finite.
 */
int surfel_texture_classify(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, float density,
                            int32_t* cls, int64_t* counts, void* stream);

/*
 * The atlas of the classes cls[F] and their counts[6] (HOST) as surfel_texture_classify returned them, Wa texels wide.  Bands of cells
 * are stacked largest class first; a band of class c has floor(Wa / (n + 4)) cells per row; a triangle's rank within its class is its
 * rank in triangle order (a stable exclusive scan), rank r sits in cell r / 2 as its lower (r even) or upper (r odd) half, cells in
 * row-major order.  table[6, 4] (HOST, int32) <- the band table; order[F] (uint32) <- order[first_c + rank] = triangle, the slots
 * behind the last patch are not written; uv[F, 3, 2] (fp32) <- the texel coordinates of every corner, 0 for a triangle without a
 * patch.  Returns the atlas height Ha (>= 1).  SURFEL_E_LIMIT, before anything is written: Wa or Ha above SURFEL_TEXTURE_MAX_SIDE, Wa
 * smaller than the cell of the largest class in use, F above 2^28.  Does not synchronise.  Scratch: 4 B x (6 F + 6 F / 4096 + 2).
 * TEXTURE.md §Layout gives the corner coordinates and the ownership rule.
 */
int64_t surfel_texture_layout(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, const int32_t* cls,
                              const int64_t* counts, int Wa, int32_t* table, uint32_t* order, float* uv, void* stream);

/*
 * acc[Ha, Wa, 4] (fp32: r, g, b, w; the caller's, zeroed before the first batch, carried across batches) <- acc combined with the
 * nviews views of this batch, in view order, one thread per owned texel, no atomics: the same bits on every run and for every
 * batching.  Per texel the point p of its (clamped) barycentrics, per view rules 1-5 of CULL.md §Visibility on p with depth[nviews, H, W]
 * (surfel_cull_mesh_depth's images of the same mesh and cameras) and eps, the cosine c between the face normal and the ray (two-sided),
 * skipped unless c >= cos_min, the weight w = c^power / (z z) (power = 1 .. SURFEL_TEXTURE_MAX_POWER by repeated multiplication) and
 * the bilinear sample of images[nviews, 3, H, W] (fp32, planar).  blend AVERAGE: rgb += w colour, w_sum += w.  BEST: (colour, w)
 * replace the kept ones when w is strictly larger.  table[6, 4] (HOST) and order from surfel_texture_layout.  H, W >= 2.
 * TEXTURE.md §Baking writes out every operation and its order.
 */
int surfel_texture_bake(int64_t V, int64_t F, const float* verts, const int32_t* tris, const int32_t* table, const uint32_t* order, int Wa, int Ha,
                        int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, const float* depth, const float* images,
                        float eps, float cos_min, int power, int blend, float* acc, void* stream);

/*
 * atlas[Ha, Wa, 3] (uint8) <- per texel: seen (acc's w > 0): rgb / w (AVERAGE) or rgb (BEST); owned but unseen: the barycentric
 * interpolation of colors[V, 3] at the texel's point, grey 0.8 when colors is NULL; unowned: (bg_r, bg_g, bg_b); quantised as
 * surfel_vis_quantize does (scale 1, bias 0).  stats[2] (int64, zeroed by the call) <- the number of owned and of seen texels.
 */
int surfel_texture_resolve(int64_t V, int64_t F, const float* verts, const int32_t* tris, const float* colors, const int32_t* table,
                           const uint32_t* order, int Wa, int Ha, const float* acc, int blend, float bg_r, float bg_g, float bg_b, uint8_t* atlas,
                           int64_t* stats, void* stream);

/*
 * out[nviews, H, W, 3] (uint8) <- the frames of a visibility buffer key[nviews, ssaa H, ssaa W] as surfel_meshview_shade's COLOR mode
 * makes them (MESHVIEW.md §Shading steps 1-4 and 9: set-up, barycentrics, supersampling, background), with the colour of a sample taken
 * from atlas[Ha, Wa, 3] (uint8) by a bilinear fetch at the interpolated uv[F, 3, 2] (TEXTURE.md §Textured shading).
 */
int surfel_texture_shade(int64_t V, int64_t F, const float* verts, const int32_t* tris, const float* uv, const uint8_t* atlas, int Wa, int Ha,
                         int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, int ssaa, const uint64_t* key,
                         float bg_r, float bg_g, float bg_b, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_TEXTURE_H */
