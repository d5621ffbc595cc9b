/*
 * surfel_mesh.h — C ABI of the bounded TSDF mesh extraction (MESH.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_train.h: plain DEVICE pointers for every array, `stream` = hipStream_t as void*, return >= 0 or a
 * negative SURFEL_E_* code (surfel_hip.h) with the message in surfel_last_error().  The volume's buffers come from the caller's
 * surfel_alloc_fn; output arrays are sized by the caller from the counts the library returns.
 *
 * What each entry replaces in the reference (CPU Open3D there):
 *   surfel_mesh_prepare_view   utils/mesh_utils.py:160-170 (depth_trunc, background mask, colour as uint8)
 *   surfel_tsdf_init / _mark / _allocate / _integrate
 *                              utils/mesh_utils.py:150-172 (o3d.pipelines.integration.ScalableTSDFVolume, volume.integrate)
 *   surfel_tsdf_count / _extract
 *                              utils/mesh_utils.py:174 (volume.extract_triangle_mesh)
 *   surfel_mesh_clusters       utils/mesh_utils.py:30-31 (cluster_connected_triangles)
 *   surfel_mesh_filter         utils/mesh_utils.py:33-38 (remove_triangles_by_mask, remove_unreferenced_vertices,
 *                              remove_degenerate_triangles)
 */
#ifndef SURFEL_MESH_H
#define SURFEL_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Voxels per block edge: block b holds voxels 16 b .. 16 b + 15 on every axis. */
#define SURFEL_TSDF_BLOCK 16

/*
 * A view's camera, 16 floats on the device: [0..11] extrinsic (world -> camera, row-major 3x4 = world_view_transform.T[:3]),
 * [12..15] fx, fy, cx, cy (pixel units, cx = (W-1)/2, cy = (H-1)/2).
 *
 * Volume state.  The caller sets the first block (dense block table and budget) and zeroes the rest; the library writes the rest.
 * Table: block (origin + (x, y, z)) sits at entry x + dims[0] * (y + dims[1] * z), value = pool slot or -1.  Pool: slot s holds
 * SURFEL_TSDF_BLOCK^3 voxels, voxel (x, y, z) of the block at index x + 16 y + 256 z, as tsdf_rgb[4 (4096 s + i) ..] = (tsdf, r, g, b)
 * and weight[4096 s + i] (20 B per voxel); slots are in table order.
 */
typedef struct surfel_tsdf_volume {
    int origin[3];
    int dims[3];
    float voxel_size;
    float sdf_trunc;
    int64_t budget_bytes;         /* table + pool + extraction buffers may not exceed this: SURFEL_E_LIMIT before allocating */
    /* written by the library */
    int32_t* table;               /* [dims product] */
    uint32_t* scratch;            /* scan scratch of the table */
    int64_t nblocks;              /* allocated blocks (after surfel_tsdf_allocate) */
    int32_t* keys;                /* [nblocks] table index of every slot */
    uint32_t* stamp;              /* [nblocks] last view that listed the slot */
    uint32_t* list;               /* [1 + nblocks] touched-slot count, slots of the current view */
    float* tsdf_rgb;              /* [nblocks * 4096 * 4] */
    float* weight;                /* [nblocks * 4096] */
    uint32_t* info;               /* [nblocks * 4096] extraction: cube case | valid << 8 | vertex-edge mask << 9 */
    uint32_t* vbase;              /* [nblocks * 4096] first vertex of every voxel */
    uint32_t* tbase;              /* [nblocks * 4096] first triangle of every voxel's cube */
    uint32_t* pool_scratch;       /* scan scratch of the pool */
    int64_t views;                /* views integrated so far */
    int64_t nverts, ntris;        /* after surfel_tsdf_count */
} surfel_tsdf_volume;

/* Bytes of the dense table (table + its scan scratch) and of one allocated block (pool + extraction buffers + bookkeeping). */
int64_t surfel_tsdf_table_bytes(const surfel_tsdf_volume* vol);
int64_t surfel_tsdf_block_bytes(void);

/*
 * One view's fusion inputs from render(): depth_out[H,W] = surf_depth, or 0 where it is not <= depth_trunc (larger, or NaN) or where
 * mask[H,W] (gt_alpha_mask, NULL = none) is < 0.5; rgba_out[H,W] = (uint8)(clamp(rgb[3,H,W], 0, 1) * 255) packed r | g << 8 | b << 16.
 * For surfel_tsdf_mark and surfel_tsdf_integrate a depth is valid when it is > 0: zero, negative and NaN depths are holes.
 */
int surfel_mesh_prepare_view(int H, int W, const float* surf_depth, const float* rgb, const float* mask, float depth_trunc, float* depth_out,
                             uint32_t* rgba_out, void* stream);

/* Checks the table against budget_bytes (SURFEL_E_LIMIT, nothing allocated), allocates it through `alloc` and clears it. */
int surfel_tsdf_init(surfel_tsdf_volume* vol, surfel_alloc_fn alloc, void* user, void* stream);
/* Allocation pass of one view: marks every block within +-sdf_trunc of a valid pixel's back-projected point. */
int surfel_tsdf_mark(surfel_tsdf_volume* vol, int H, int W, const float* depth, const float* cam, void* stream);
/* After every view was marked: counts the blocks (synchronises), checks table + pool against budget_bytes (SURFEL_E_LIMIT, nothing
 * allocated), allocates and zeroes the pool, assigns slots in table order.  Returns nblocks. */
int64_t surfel_tsdf_allocate(surfel_tsdf_volume* vol, surfel_alloc_fn alloc, void* user, void* stream);
/* Fuses one view (MESH.md §Integration) into the blocks it touches: a duplicate-free touched list, then one workgroup per block. */
int surfel_tsdf_integrate(surfel_tsdf_volume* vol, int H, int W, const float* depth, const uint32_t* rgba, const float* cam, void* stream);
/* Extraction pass 1: cube cases, per-voxel vertex and triangle counts, their scans; synchronises and sets nverts / ntris. */
int surfel_tsdf_count(surfel_tsdf_volume* vol, void* stream);
/* Extraction pass 2: verts[nverts, 3] (world), colors[nverts, 3] (0..1), tris[ntris, 3]. */
int surfel_tsdf_extract(const surfel_tsdf_volume* vol, float* verts, float* colors, int32_t* tris, void* stream);

/*
 * Edge-connected triangle clusters: label[F] = smallest triangle id of the triangle's cluster, size[F] = triangles in the cluster
 * whose label is that id (0 for every other id).  Two triangles are connected when they share an unordered pair of vertex ids,
 * both in [0, V); an edge with an id outside [0, V) links nothing (it sorts behind every valid edge under the key V) and leaves the
 * other edges of its triangle as they are.  Scratch through `alloc`.
 */
int surfel_mesh_clusters(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const int32_t* tris, int32_t* label, int32_t* size,
                         void* stream);
/*
 * Drops the triangles whose cluster has fewer than `threshold` triangles, then the vertices no kept triangle uses (order kept),
 * then the triangles that repeat an index.  Outputs sized V / F by the caller; counts_out (HOST, 2 int64) = (V', F').  Synchronises.
 */
int surfel_mesh_filter(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const float* colors, const int32_t* tris,
                       const int32_t* label, const int32_t* size, int threshold, float* verts_out, float* colors_out, int32_t* tris_out,
                       int64_t* counts_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_MESH_H */
