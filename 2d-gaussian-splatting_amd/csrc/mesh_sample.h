// mesh_sample.h — what the passes that shade a visibility buffer share (mesh_view.hip: shaded / normal / colour frames, MESHVIEW.md;
// mesh_texture.hip: textured frames, TEXTURE.md): steps 1 to 4 of MESHVIEW.md §Shading for one sample.  Both files are compiled with
// -ffp-contract=off (build.py): fp32 in the written order, as tests/meshview_oracle.py and tests/texture_oracle.py restate it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_raster.h"

namespace surfel {

struct MeshSample {
    int64_t i0, i1, i2;                                        // the triangle's vertices
    float n0x, n0y, n0z, n1x, n1y, n1z, n2x, n2y, n2z;         // step 2: n0 = v1 x v2, n1 = v2 x v0, n2 = v0 x v1 in camera space
    float dx, dy;                                              // step 3: the ray
    float l0, l1, l2;                                          // step 4: the clamped, normalised weights
};

// x, y: the sample's integer coordinates in the sample grid whose intrinsics the camera holds.  false: the sample shows the background
// (an empty key, or one that names a triangle the depth rule would skip).
__device__ inline bool mesh_sample(uint64_t key, float x, float y, const CullCam& c, int64_t V, int64_t F, const float* __restrict__ verts,
                                   const int32_t* __restrict__ tris, MeshSample& s) {
    const uint32_t t = (uint32_t)key;
    if ((uint32_t)(key >> 32) >= CULL_INF || (int64_t)t >= F) return false;
    const int64_t i0 = tris[3 * (int64_t)t], i1 = tris[3 * (int64_t)t + 1], i2 = tris[3 * (int64_t)t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    s.i0 = i0; s.i1 = i1; s.i2 = i2;
    const float px0 = verts[3 * i0], py0 = verts[3 * i0 + 1], pz0 = verts[3 * i0 + 2];
    const float px1 = verts[3 * i1], py1 = verts[3 * i1 + 1], pz1 = verts[3 * i1 + 2];
    const float px2 = verts[3 * i2], py2 = verts[3 * i2 + 1], pz2 = verts[3 * i2 + 2];
    const float* m = c.m;
    // 1: camera space (CULL.md rule 1)
    const float X0 = ((m[0] * px0 + m[1] * py0) + m[2] * pz0) + m[3], Y0 = ((m[4] * px0 + m[5] * py0) + m[6] * pz0) + m[7],
                Z0 = ((m[8] * px0 + m[9] * py0) + m[10] * pz0) + m[11];
    const float X1 = ((m[0] * px1 + m[1] * py1) + m[2] * pz1) + m[3], Y1 = ((m[4] * px1 + m[5] * py1) + m[6] * pz1) + m[7],
                Z1 = ((m[8] * px1 + m[9] * py1) + m[10] * pz1) + m[11];
    const float X2 = ((m[0] * px2 + m[1] * py2) + m[2] * pz2) + m[3], Y2 = ((m[4] * px2 + m[5] * py2) + m[6] * pz2) + m[7],
                Z2 = ((m[8] * px2 + m[9] * py2) + m[10] * pz2) + m[11];
    // 2: n0 = v1 x v2, n1 = v2 x v0, n2 = v0 x v1, det, its sign
    s.n0x = Y1 * Z2 - Z1 * Y2; s.n0y = Z1 * X2 - X1 * Z2; s.n0z = X1 * Y2 - Y1 * X2;
    s.n1x = Y2 * Z0 - Z2 * Y0; s.n1y = Z2 * X0 - X2 * Z0; s.n1z = X2 * Y0 - Y2 * X0;
    s.n2x = Y0 * Z1 - Z0 * Y1; s.n2y = Z0 * X1 - X0 * Z1; s.n2z = X0 * Y1 - Y0 * X1;
    const float det = (X0 * s.n0x + Y0 * s.n0y) + Z0 * s.n0z;
    const float sg = det < 0.0f ? -1.0f : 1.0f;
    // 3: the ray and the edge values in the plain form
    s.dx = (x - c.cx) / c.fx; s.dy = (y - c.cy) / c.fy;
    const float e0 = sg * ((s.n0x * s.dx + s.n0y * s.dy) + s.n0z), e1 = sg * ((s.n1x * s.dx + s.n1y * s.dy) + s.n1z),
                e2 = sg * ((s.n2x * s.dx + s.n2y * s.dy) + s.n2z);
    // 4: clamped weights
    const float w0 = e0 > 0.0f ? e0 : 0.0f, w1 = e1 > 0.0f ? e1 : 0.0f, w2 = e2 > 0.0f ? e2 : 0.0f;
    const float ws = (w0 + w1) + w2;
    const float third = 1.0f / 3.0f;
    const bool some = ws > 0.0f;
    s.l0 = some ? w0 / ws : third; s.l1 = some ? w1 / ws : third; s.l2 = some ? w2 / ws : third;
    return true;
}

}  // namespace surfel
