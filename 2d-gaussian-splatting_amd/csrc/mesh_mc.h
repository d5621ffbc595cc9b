// mesh_mc.h — the marching-cubes triangle writer shared by the bounded and the unbounded extraction (MESH.md).
#pragma once
#include "mesh_mc_table.h"

namespace surfel {

// the triangles of a cube of case cs into tris_out[3 * MC_NTRI[cs]].  vertex_of(e) is the id of the vertex on cube edge
// e = {x, y, z of the edge's lower corner, axis}: the voxel at that corner owns the edge, and the vertex is the owner's base plus the
// number of its vertex edges below `axis` (popcount of its mask bits below it).  The caller knows how to find the owner.
template <class F>
__device__ __forceinline__ void mc_write_triangles(uint32_t cs, int32_t* tris_out, F vertex_of) {
    const uint32_t nt = MC_NTRI[cs];
    for (uint32_t t = 0; t < nt; t++)
        for (int j = 0; j < 3; j++) tris_out[3 * t + j] = (int32_t)vertex_of(MC_EDGE[MC_TRIS[cs][3 * t + j]]);
}

}  // namespace surfel
