// mesh_cull.hip — view culling of a mesh: depth images of a triangle mesh for a batch of views (the clip-free homogeneous rasteriser of
// mesh_raster.h with an integer-minimum depth buffer) and the per-vertex view count of the reference's Mesher.point_masks
// (include/surfel_cull.h, CULL.md).
// Compiled with -ffp-contract=off (build.py): the visibility kernel rounds exactly as its restatement in tests/cull_oracle.py; the
// rasteriser spells its fused multiply-adds out (fmaf), so a pixel gets the same bits from either size class.  wave64; no LDS, no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_cull.h"
#include "mesh_raster.h"
#include "side_util.h"

namespace surfel {

__global__ void __launch_bounds__(CT) cull_resolve_kernel(int64_t n, uint32_t* depth) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i < n && depth[i] == CULL_INF) depth[i] = 0u;
}

// ---- the per-vertex view count (Mesher.point_masks) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(CT) cull_visibility_kernel(int64_t N, const float* __restrict__ points, int nviews, const float* __restrict__ w2c,
                                                             const float* __restrict__ intrinsics, int n_intrinsics, int H, int W,
                                                             const float* __restrict__ depth, float eps, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= N) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    const float wm = (float)(W - 1), hm = (float)(H - 1);
    int count = 0;
    for (int view = 0; view < nviews; view++) {
        const float* m = w2c + 12 * (int64_t)view;
        const float* q = intrinsics + 4 * (int64_t)(n_intrinsics == 1 ? 0 : view);
        const float X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3], Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7], Z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        const float zz = Z + 1e-8f;
        const float u = (q[0] * X + q[2] * Z) / zz, v = (q[1] * Y + q[3] * Z) / zz;
        if (!(u >= 0.0f && u <= wm && v >= 0.0f && v <= hm && zz > 0.0f)) continue;      // (false for NaN: nothing non-finite indexes below)
        // grid_sample(padding_mode = 'border', align_corners = True) at the normalised (u, v): the round trip, the clip, four corners
        const float gx = u / wm * 2.0f - 1.0f, gy = v / hm * 2.0f - 1.0f;
        const float ix = fminf(wm, fmaxf(((gx + 1.0f) / 2.0f) * wm, 0.0f)), iy = fminf(hm, fmaxf(((gy + 1.0f) / 2.0f) * hm, 0.0f));
        const float fx0 = floorf(ix), fy0 = floorf(iy), fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
        const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
        const float nw = (fx1 - ix) * (fy1 - iy), ne = (ix - fx0) * (fy1 - iy), sw = (fx1 - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
        const float* img = depth + (int64_t)view * H * W;
        float sample = 0.0f;      // x0, y0 lie inside (clipped); x1, y1 may be W, H, where torch adds nothing
        sample += img[(int64_t)y0 * W + x0] * nw;
        if (x1 < W) sample += img[(int64_t)y0 * W + x1] * ne;
        if (y1 < H) sample += img[(int64_t)y1 * W + x0] * sw;
        if (x1 < W && y1 < H) sample += img[(int64_t)y1 * W + x1] * se;
        const bool front = sample > 0.0f ? zz < sample + eps : true;
        count += front;
    }
    counts[i] += count;
}

namespace {
inline unsigned grid(int64_t n) { return blocks_for(n, CT); }
}  // namespace

extern "C" {

int64_t surfel_cull_mesh_depth(surfel_alloc_fn alloc, void* user, int64_t V, int64_t F, const float* verts, const int32_t* tris, int nviews,
                               const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W, float znear, float zfar,
                               int small_pixels, float* depth, float* stage_ms, void* stream) {
    if (!alloc || V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !tris) || cull_bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 1 || W < 1 ||
        !(znear > 0.0f) || !(zfar >= znear) || !(zfar < INFINITY) || (nviews > 0 && !depth))
        return api_fail(SURFEL_E_INVALID, "cull_mesh_depth: bad arguments");
    if (V > CULL_MAX_ELEMS || F > CULL_MAX_ELEMS || (int64_t)H * W > CULL_MAX_ELEMS)
        return api_fail(SURFEL_E_LIMIT, "cull_mesh_depth: more than 2^31 - 1 vertices, triangles or pixels");
    if (nviews > SURFEL_CULL_MAX_VIEWS) return api_fail(SURFEL_E_LIMIT, "cull_mesh_depth: more than SURFEL_CULL_MAX_VIEWS views in one call");
    if (stage_ms) for (int k = 0; k < SURFEL_CULL_STAGES; k++) stage_ms[k] = 0.0f;
    if (nviews == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t pixels = (int64_t)nviews * H * W;
    auto init = [&](uint32_t* img) {
        if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(img), (int)CULL_INF, (size_t)pixels, st) != hipSuccess)
            return api_fail(SURFEL_E_HIP, "cull_mesh_depth: memset", hipGetLastError());
        return 0;
    };
    auto resolve = [&](uint32_t* img) {
        hipLaunchKernelGGL(cull_resolve_kernel, dim3(grid(pixels)), dim3(CT), 0, st, pixels, img);
        return launched("cull_resolve_kernel");
    };
    return cull_rasterise<uint32_t>("cull_mesh_depth", alloc, user, V, F, verts, tris, nviews, w2c, intrinsics, n_intrinsics, H, W, znear, zfar,
                                    small_pixels, reinterpret_cast<uint32_t*>(depth), stage_ms, st, init, resolve);
}

int surfel_cull_visibility(int64_t N, const float* points, int nviews, const float* w2c, const float* intrinsics, int n_intrinsics, int H, int W,
                           const float* depth, float eps, int32_t* counts, void* stream) {
    if (N < 0 || (N > 0 && (!points || !counts)) || cull_bad_cameras(nviews, w2c, intrinsics, n_intrinsics) || H < 2 || W < 2 || (nviews > 0 && !depth) ||
        !(eps == eps))
        return api_fail(SURFEL_E_INVALID, "cull_visibility: bad arguments");
    if (N > CULL_MAX_ELEMS || (int64_t)H * W > CULL_MAX_ELEMS) return api_fail(SURFEL_E_LIMIT, "cull_visibility: more than 2^31 - 1 points or pixels");
    if (N == 0 || nviews == 0) return 0;
    hipLaunchKernelGGL(cull_visibility_kernel, dim3(grid(N)), dim3(CT), 0, static_cast<hipStream_t>(stream), N, points, nviews, w2c, intrinsics,
                       n_intrinsics, H, W, depth, eps, counts);
    return launched("cull_visibility_kernel");
}

}  // extern "C"

}  // namespace surfel
