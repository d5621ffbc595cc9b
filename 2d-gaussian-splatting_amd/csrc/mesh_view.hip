// mesh_view.hip — the mesh viewer (include/surfel_meshview.h, MESHVIEW.md): the visibility buffer (the rasteriser of mesh_raster.h with a
// 64-bit key per pixel), vertex normals as fixed-point sums of unit face normals, and the pass that shades a visibility buffer into
// 8-bit frames.  Compiled with -ffp-contract=off (build.py): the normal and shading kernels round as their restatement in
// tests/meshview_oracle.py — fp32 throughout, correctly rounded / and sqrt, no fused multiply-add outside the shared rasteriser.
// wave64; no LDS, no MFMA; the shading kernel has no atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_meshview.h"
#include "mesh_raster.h"
#include "mesh_sample.h"
#include "side_util.h"
#include "vis_pixels.h"

namespace surfel {

constexpr uint64_t MV_EMPTY = SURFEL_MESHVIEW_EMPTY;

__global__ void __launch_bounds__(CT) meshview_clear_kernel(int64_t n, uint64_t* key) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i < n) key[i] = MV_EMPTY;
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CT) meshview_face_normals_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                                   unsigned long long* acc) {
    const int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (t >= F) return;
    const int64_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return;
    const float ax = verts[3 * i1] - verts[3 * i0], ay = verts[3 * i1 + 1] - verts[3 * i0 + 1], az = verts[3 * i1 + 2] - verts[3 * i0 + 2];
    const float bx = verts[3 * i2] - verts[3 * i0], by = verts[3 * i2 + 1] - verts[3 * i0 + 1], bz = verts[3 * i2 + 2] - verts[3 * i0 + 2];
    const float fx = ay * bz - az * by, fy = az * bx - ax * bz, fz = ax * by - ay * bx;
    const float len = sqrtf((fx * fx + fy * fy) + fz * fz);
    if (!(isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(len)) || !(len > 0.0f)) return;
    const float s = (float)SURFEL_MESHVIEW_NORMAL_SCALE;
    // two's complement: adding the unsigned image of a negative int64 is the signed addition
    const unsigned long long qx = (unsigned long long)(long long)rintf((fx / len) * s), qy = (unsigned long long)(long long)rintf((fy / len) * s),
                             qz = (unsigned long long)(long long)rintf((fz / len) * s);
    const int64_t idx[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        atomicAdd(acc + 3 * idx[k], qx);
        atomicAdd(acc + 3 * idx[k] + 1, qy);
        atomicAdd(acc + 3 * idx[k] + 2, qz);
    }
}

__global__ void __launch_bounds__(CT) meshview_vertex_normals_kernel(int64_t V, const int64_t* __restrict__ acc, float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (v >= V) return;
    const float x = (float)acc[3 * v], y = (float)acc[3 * v + 1], z = (float)acc[3 * v + 2];
    const float len = sqrtf((x * x + y * y) + z * z);
    const bool ok = len > 0.0f;
    normals[3 * v] = ok ? x / len : 0.0f;
    normals[3 * v + 1] = ok ? y / len : 0.0f;
    normals[3 * v + 2] = ok ? z / len : 0.0f;
}

// ---- shading ----------------------------------------------------------------------------------------------------------------------------
struct MvColor { float r, g, b; };

// One sample of the visibility buffer (MESHVIEW.md §Shading, the numbered steps; steps 1 to 4 are mesh_sample.h's).  x, y: the sample's
// integer coordinates in the sample grid whose intrinsics the camera holds.
__device__ inline MvColor meshview_sample(uint64_t key, float x, float y, const CullCam& c, int64_t V, int64_t F, const float* __restrict__ verts,
                                          const int32_t* __restrict__ tris, const float* __restrict__ colors, const float* __restrict__ normals, int mode,
                                          MvColor bg) {
    MeshSample sm;
    if (!mesh_sample(key, x, y, c, V, F, verts, tris, sm)) return bg;      // steps 1 to 4 (mesh_sample.h)
    const int64_t i0 = sm.i0, i1 = sm.i1, i2 = sm.i2;
    const float* m = c.m;
    const float n0x = sm.n0x, n0y = sm.n0y, n0z = sm.n0z, n1x = sm.n1x, n1y = sm.n1y, n1z = sm.n1z, n2x = sm.n2x, n2y = sm.n2y, n2z = sm.n2z;
    const float dx = sm.dx, dy = sm.dy, l0 = sm.l0, l1 = sm.l1, l2 = sm.l2;
    // 5: the face normal in camera space, against the ray
    float fx = (n0x + n1x) + n2x, fy = (n0y + n1y) + n2y, fz = (n0z + n1z) + n2z;
    const float flen = sqrtf((fx * fx + fy * fy) + fz * fz);
    const bool fok = flen > 0.0f && isfinite(flen);
    fx = fok ? fx / flen : 0.0f; fy = fok ? fy / flen : 0.0f; fz = fok ? fz / flen : 0.0f;
    if ((fx * dx + fy * dy) + fz > 0.0f) { fx = -fx; fy = -fy; fz = -fz; }
    float cx_ = fx, cy_ = fy, cz_ = fz;                                                   // the normal in camera space
    float wx = (m[0] * fx + m[4] * fy) + m[8] * fz, wy = (m[1] * fx + m[5] * fy) + m[9] * fz, wz = (m[2] * fx + m[6] * fy) + m[10] * fz;      // in world space
    // 6: the smooth normal
    if (normals) {
        const float sx = (l0 * normals[3 * i0] + l1 * normals[3 * i1]) + l2 * normals[3 * i2];
        const float sy = (l0 * normals[3 * i0 + 1] + l1 * normals[3 * i1 + 1]) + l2 * normals[3 * i2 + 1];
        const float sz = (l0 * normals[3 * i0 + 2] + l1 * normals[3 * i1 + 2]) + l2 * normals[3 * i2 + 2];
        const float slen = sqrtf((sx * sx + sy * sy) + sz * sz);
        if (slen > 0.0f && isfinite(slen)) {
            wx = sx / slen; wy = sy / slen; wz = sz / slen;
            cx_ = (m[0] * wx + m[1] * wy) + m[2] * wz; cy_ = (m[4] * wx + m[5] * wy) + m[6] * wz; cz_ = (m[8] * wx + m[9] * wy) + m[10] * wz;
            if ((cx_ * dx + cy_ * dy) + cz_ > 0.0f) { wx = -wx; wy = -wy; wz = -wz; cx_ = -cx_; cy_ = -cy_; cz_ = -cz_; }
        }
    }
    MvColor o;
    if (mode == SURFEL_MESHVIEW_NORMAL) {
        o.r = wx * 0.5f + 0.5f; o.g = wy * 0.5f + 0.5f; o.b = wz * 0.5f + 0.5f;
        return o;
    }
    // 7: the albedo
    if (colors) {
        o.r = (l0 * colors[3 * i0] + l1 * colors[3 * i1]) + l2 * colors[3 * i2];
        o.g = (l0 * colors[3 * i0 + 1] + l1 * colors[3 * i1 + 1]) + l2 * colors[3 * i2 + 1];
        o.b = (l0 * colors[3 * i0 + 2] + l1 * colors[3 * i1 + 2]) + l2 * colors[3 * i2 + 2];
    } else {
        o.r = o.g = o.b = 0.8f;
    }
    if (mode == SURFEL_MESHVIEW_COLOR) return o;
    // 8: a headlight
    const float dlen = sqrtf((dx * dx + dy * dy) + 1.0f);
    const float ndl = -((cx_ * dx + cy_ * dy) + cz_) / dlen;
    const float f = 0.3f + 0.7f * (ndl > 0.0f ? ndl : 0.0f);
    o.r = o.r * f; o.g = o.g * f; o.b = o.b * f;
    return o;
}

// one thread per output pixel of every view
__global__ void __launch_bounds__(CT) meshview_shade_kernel(int64_t V, int64_t F, const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                            const float* __restrict__ colors, const float* __restrict__ normals, int nviews,
                                                            const float* __restrict__ w2c, const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                            int ssaa, const uint64_t* __restrict__ key, int mode, float bg_r, float bg_g, float bg_b,
                                                            uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    const int64_t hw = (int64_t)H * W;
    if (i >= hw * nviews) return;
    const int view = (int)(i / hw);
    const int y = (int)((i - view * hw) / W), x = (int)((i - view * hw) - (int64_t)y * W);
    const CullCam cam = cull_cam(w2c, intrinsics, n_intrinsics, view);
    const int64_t sW = (int64_t)W * ssaa;
    const uint64_t* img = key + view * hw * ssaa * ssaa;
    const MvColor bg = {bg_r, bg_g, bg_b};
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (int ky = 0; ky < ssaa; ky++)
        for (int kx = 0; kx < ssaa; kx++) {
            const int sx = x * ssaa + kx, sy = y * ssaa + ky;
            const MvColor c = meshview_sample(img[sy * sW + sx], (float)sx, (float)sy, cam, V, F, verts, tris, colors, normals, mode, bg);
            r = r + c.r; g = g + c.g; b = b + c.b;
        }
    const float inv = 1.0f / (float)(ssaa * ssaa);
    out[3 * i] = (uint8_t)quant8(r * inv, 1.0f, 0.0f);
    out[3 * i + 1] = (uint8_t)quant8(g * inv, 1.0f, 0.0f);
    out[3 * i + 2] = (uint8_t)quant8(b * inv, 1.0f, 0.0f);
}

extern "C" {

int64_t surfel_meshview_visibility(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, int nviews,
                                   const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, float znear, float zfar,
                                   int small_pixels, uint64_t* key, float* stage_ms, void* stream) {
    if (!alloc || V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !tris) || cull_bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 1 || W < 1 ||
        !(znear > 0.0f) || !(zfar >= znear) || !(zfar < INFINITY) || (nviews > 0 && !key))
        return api_fail(SURFEL_E_INVALID, "meshview_visibility: bad arguments");
    // (the rasteriser's own limit on F is the smaller one; the key's is stated for a rasteriser that lifts it)
    if (F >= (int64_t)0xffffffff) return api_fail(SURFEL_E_LIMIT, "meshview_visibility: 2^32 - 1 triangles or more do not fit the key");
    if (V > CULL_MAX_ELEMS || F > CULL_MAX_ELEMS || (int64_t)H * W > CULL_MAX_ELEMS)
        return api_fail(SURFEL_E_LIMIT, "meshview_visibility: more than 2^31 - 1 vertices, triangles or pixels");
    if (nviews > SURFEL_CULL_MAX_VIEWS) return api_fail(SURFEL_E_LIMIT, "meshview_visibility: more than SURFEL_CULL_MAX_VIEWS views in one call");
    if (stage_ms) for (int k = 0; k < SURFEL_CULL_STAGES; k++) stage_ms[k] = 0.0f;
    if (nviews == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t pixels = (int64_t)nviews * H * W;
    if ((pixels + CT - 1) / CT > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "meshview_visibility: more than 2^39 pixels in one call");
    auto init = [&](uint64_t* img) {
        hipLaunchKernelGGL(meshview_clear_kernel, dim3(blocks_for(pixels, CT)), dim3(CT), 0, st, pixels, img);
        return launched("meshview_clear_kernel");
    };
    auto resolve = [](uint64_t*) { return 0; };      // (an empty key stays as it is: the shading pass and unpack() read it)
    return cull_rasterise<uint64_t>("meshview_visibility", alloc, user, V, F, verts, tris, nviews, w2c, intrinsics, n_intrinsics, H, W, znear, zfar,
                                    small_pixels, key, stage_ms, st, init, resolve);
}

int surfel_meshview_vertex_normals(int64_t V, int64_t F, const float* verts, const int32_t* tris, int64_t* acc, float* normals, void* stream) {
    if (V < 0 || F < 0 || (V > 0 && (!verts || !acc || !normals)) || (F > 0 && !tris))
        return api_fail(SURFEL_E_INVALID, "meshview_vertex_normals: bad arguments");
    if (V > CULL_MAX_ELEMS || F > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "meshview_vertex_normals: more than 2^31 - 1 vertices or triangles");
    if (V == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(acc, 0, (size_t)V * 3 * sizeof(int64_t), st) != hipSuccess)
        return api_fail(SURFEL_E_HIP, "meshview_vertex_normals: memset", hipGetLastError());
    if (F > 0) {
        hipLaunchKernelGGL(meshview_face_normals_kernel, dim3(blocks_for(F, CT)), dim3(CT), 0, st, V, F, verts, tris,
                           reinterpret_cast<unsigned long long*>(acc));
        if (int rc = launched("meshview_face_normals_kernel")) return rc;
    }
    hipLaunchKernelGGL(meshview_vertex_normals_kernel, dim3(blocks_for(V, CT)), dim3(CT), 0, st, V, acc, normals);
    return launched("meshview_vertex_normals_kernel");
}

int surfel_meshview_shade(int64_t V, int64_t F, const float* verts, const int32_t* tris, const float* colors, const float* normals, int nviews,
                          const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, int ssaa, const uint64_t* key, int mode,
                          float bg_r, float bg_g, float bg_b, uint8_t* out, void* stream) {
    if (V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !tris) || cull_bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 1 || W < 1 || ssaa < 1 ||
        ssaa > SURFEL_MESHVIEW_MAX_SSAA || (nviews > 0 && (!key || !out)) || mode < SURFEL_MESHVIEW_SHADED || mode > SURFEL_MESHVIEW_COLOR)
        return api_fail(SURFEL_E_INVALID, "meshview_shade: bad arguments");
    if (V > CULL_MAX_ELEMS || F > CULL_MAX_ELEMS || (int64_t)H * W * ssaa * ssaa > CULL_MAX_ELEMS)
        return api_fail(SURFEL_E_LIMIT, "meshview_shade: more than 2^31 - 1 vertices, triangles or samples of a view");
    if (nviews > SURFEL_CULL_MAX_VIEWS) return api_fail(SURFEL_E_LIMIT, "meshview_shade: more than SURFEL_CULL_MAX_VIEWS views in one call");
    if (nviews == 0) return 0;
    const int64_t n = (int64_t)nviews * H * W;
    if ((n + CT - 1) / CT > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "meshview_shade: more than 2^39 output pixels in one call");
    hipLaunchKernelGGL(meshview_shade_kernel, dim3(blocks_for(n, CT)), dim3(CT), 0, static_cast<hipStream_t>(stream), V, F, verts, tris, colors, normals,
                       nviews, w2c, intrinsics, n_intrinsics, H, W, ssaa, key, mode, bg_r, bg_g, bg_b, out);
    return launched("meshview_shade_kernel");
}

}  // extern "C"

}  // namespace surfel
