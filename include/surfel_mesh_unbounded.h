/*
 * surfel_mesh_unbounded.h — C ABI of the unbounded mesh extraction (MESH.md §Unbounded), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_mesh.h: plain DEVICE pointers for every array, `stream` = hipStream_t as void*, return >= 0 or a
 * negative SURFEL_E_* code (surfel_hip.h) with the message in surfel_last_error().  The lattice and the slab scratch come from the
 * caller's surfel_alloc_fn; output arrays are sized by the caller from the counts the library returns.
 *
 * What each entry replaces in the reference (utils/mesh_utils.py, utils/mcube_utils.py; torch, scikit-image and trimesh there):
 *   surfel_unbounded_bytes / _init  the sample grids of marching_cubes_with_contraction (mcube_utils.py:31-57)
 *   surfel_unbounded_fuse           compute_unbounded_tsdf over the contracted lattice (mesh_utils.py:215-250)
 *   surfel_unbounded_count / _extract
 *                                   measure.marching_cubes per crop, merge_vertices, inv_contraction and clipping
 *                                   (mcube_utils.py:59-91)
 *   surfel_unbounded_color          compute_unbounded_tsdf(..., return_rgb=True) on the mesh vertices (mesh_utils.py:274-276)
 */
#ifndef SURFEL_MESH_UNBOUNDED_H
#define SURFEL_MESH_UNBOUNDED_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One view, 64 B, in a DEVICE array.  proj holds three columns of the row-vector full_proj_transform P (4x4): a world point p
 * projects to x = proj[0..2] . p + proj[3], y = proj[4..6] . p + proj[7], w = proj[8..10] . p + proj[11] (P[:, 0], P[:, 1],
 * P[:, 3]).  The view's surf_depth [H, W] starts at depth[offset] and its render [3, H, W] at rgb[3 * offset] in the packed arrays.
 */
typedef struct surfel_unbounded_view {
    float proj[12];
    int32_t H, W;
    int64_t offset;
} surfel_unbounded_view;

/*
 * Lattice state.  The caller sets the first block and zeroes the rest; the library writes the rest.  Sample (x, y, z) of the
 * M^3 lattice sits at contracted s = -R + (x, y, z) * 2R / (M - 1), i.e. world center + radius * uncontract(s), and its tsdf at
 * tsdf[x + M (y + M z)].  Extraction walks z-slabs of `slab` cube planes; each slab's scratch holds 12 B per sample of slab + 1
 * planes.
 */
typedef struct surfel_unbounded_volume {
    int M;                        /* samples per axis, 2 .. 2048 */
    int slab;                     /* cube planes per extraction slab; 0 = the library's default (about 2^26 samples per slab) */
    float R;                      /* lattice half-width in contracted space (< 2) */
    float center[3];              /* normalisation: s = contract((p - center) / radius) */
    float radius;
    float voxel_size;             /* 2 radius / N: sdf_trunc = 5 voxel_size, divided by 2 - min(|s|, 1.9) where |s| > 1 */
    int64_t budget_bytes;         /* lattice + slab scratch (+ outputs after counting) may not exceed this: SURFEL_E_LIMIT */
    /* written by the library */
    float* tsdf;                  /* [M^3] */
    uint32_t* info;               /* slab scratch [(slab + 1) M^2]: cube case | vertex-edge mask << 8 */
    uint32_t* vbase;              /* slab scratch [(slab + 1) M^2]: first vertex of every sample, relative to the slab */
    uint32_t* tbase;              /* slab scratch [(slab + 1) M^2]: first triangle of every cube, relative to the slab */
    uint32_t* scan_scratch;       /* scan scratch of one slab */
    int64_t* slab_base;           /* [2 * nslabs + 2] first vertex and first triangle of every slab, then the totals */
    int64_t nslabs;
    int64_t nverts, ntris;        /* after surfel_unbounded_count */
} surfel_unbounded_volume;

/* Bytes of the lattice plus the slab scratch, what surfel_unbounded_init allocates (-1 and an error on bad fields).  The outputs
 * add 24 B per vertex (position and colour) and 12 B per triangle. */
int64_t surfel_unbounded_bytes(const surfel_unbounded_volume* vol);

/* Checks M, R, the slab and the budget (SURFEL_E_LIMIT, nothing allocated), then allocates the lattice and the slab scratch. */
int surfel_unbounded_init(surfel_unbounded_volume* vol, surfel_alloc_fn alloc, void* user, void* stream);

/*
 * Fuses every view into every lattice sample (MESH.md §Unbounded): tsdf = (-1 + sum of clamp(sdf / sdf_trunc, -1, 1)) / (1 + n)
 * over the n views that count.  views[nviews] and depth on the device; count[M^3] (NULL = not written) receives n.
 */
int surfel_unbounded_fuse(surfel_unbounded_volume* vol, int nviews, const surfel_unbounded_view* views, const float* depth, uint16_t* count,
                          void* stream);

/* Extraction sweep 1: per-slab vertex and triangle counts and their bases; synchronises and sets nverts / ntris.  SURFEL_E_LIMIT
 * when V or F would pass 2^31 - 1 or lattice + scratch + outputs exceed budget_bytes. */
int surfel_unbounded_count(surfel_unbounded_volume* vol, void* stream);

/* Extraction sweep 2: verts[nverts, 3] (world, clipped to [-32, 32]), tris[ntris, 3]. */
int surfel_unbounded_extract(const surfel_unbounded_volume* vol, float* verts, int32_t* tris, void* stream);

/*
 * Vertex colours: colors[V, 3] = sum of bilinear rgb / (1 + n) over the n views where the world vertex projects inside, w > 0 and
 * depth - w > -sdf_trunc.  rgb packed as the views say ([3, H, W] per view at 3 * offset).
 */
int surfel_unbounded_color(int64_t V, const float* verts, int nviews, const surfel_unbounded_view* views, const float* depth, const float* rgb,
                           float sdf_trunc, float* colors, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_MESH_UNBOUNDED_H */
