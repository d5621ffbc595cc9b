// scene_undistort.hip — the capture loader's undistortion (include/surfel_undistort.h, UNDISTORT.md): a decoded u8 image taken with a
// SIMPLE_RADIAL, RADIAL, OPENCV or FULL_OPENCV camera is resampled into the undistorted pinhole camera, bilinearly, in fp64.
// Compiled without contraction (build.py), so every expression below rounds operation by operation like its numpy restatement
// (tests/undistort_oracle.py) and the bytes come out equal.  No tables, no LDS, no atomics, no scratch: the twelve distortion
// parameters and the pinhole travel in the kernel's arguments.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/surfel_undistort.h"
#include "side_util.h"

namespace surfel {

constexpr int UX = 64;      // output columns per workgroup: one per lane, so a wave's taps follow one (bent) source row ...
constexpr int UY = 4;       // ... times rows, one per wave: the workgroup's source footprint is a patch of about 64 x 4 pixels

struct UndistortParams {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6;      // q, in the header's order
    double fx2, fy2, cx2, cy2;                                  // the undistorted pinhole
};

// One thread per output pixel.  The validity test is the only bounds logic: it is made on the fp64 floor values before any
// conversion to an integer, and every comparison is written so that a NaN (or an infinity) fails it.
template <int C>
__global__ void __launch_bounds__(UX * UY) undistort_kernel(int H, int W, int H2, int W2, UndistortParams p, const uint8_t* __restrict__ src,
                                                            uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * UX + (threadIdx.x & (UX - 1)), y = blockIdx.y * UY + (threadIdx.x / UX);
    if (x >= W2 || y >= H2) return;
    const double u = ((double)x + 0.5 - p.cx2) / p.fx2, v = ((double)y + 0.5 - p.cy2) / p.fy2;
    const double r2 = u * u + v * v, r4 = r2 * r2, r6 = r4 * r2;
    const double rad = (1.0 + p.k1 * r2 + p.k2 * r4 + p.k3 * r6) / (1.0 + p.k4 * r2 + p.k5 * r4 + p.k6 * r6);
    const double uv = u * v;
    const double ud = u * rad + 2.0 * p.p1 * uv + p.p2 * (r2 + 2.0 * u * u);
    const double vd = v * rad + 2.0 * p.p2 * uv + p.p1 * (r2 + 2.0 * v * v);
    const double xs = p.fx * ud + p.cx - 0.5, ys = p.fy * vd + p.cy - 0.5;
    const double x0 = floor(xs), y0 = floor(ys);
    const bool valid = x0 >= 0.0 && x0 + 1.0 <= (double)(W - 1) && y0 >= 0.0 && y0 + 1.0 <= (double)(H - 1);
    uint8_t* o = dst + ((int64_t)y * W2 + x) * C;
    if (!valid) {
#pragma unroll
        for (int c = 0; c < C; c++) o[c] = 0;
        return;
    }
    const double dx = xs - x0, dy = ys - y0;
    const uint8_t* s0 = src + ((int64_t)(int)y0 * W + (int)x0) * C;      // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2
    const uint8_t* s1 = s0 + (int64_t)W * C;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const double top = (1.0 - dx) * (double)s0[c] + dx * (double)s0[C + c];
        const double bot = (1.0 - dx) * (double)s1[c] + dx * (double)s1[C + c];
        const double val = (1.0 - dy) * top + dy * bot;
        o[c] = (uint8_t)(int)floor(val + 0.5);
    }
}

}  // namespace surfel

using namespace surfel;

extern "C" {

int surfel_scene_undistort(int H, int W, int C, int H2, int W2, const double* q, const double* pinhole, const uint8_t* src, uint8_t* dst,
                           void* stream) {
    if (H <= 0 || W <= 0 || H2 <= 0 || W2 <= 0 || (C != 1 && C != 3 && C != 4) || !q || !pinhole || !src || !dst)
        return api_fail(SURFEL_E_INVALID, "scene_undistort: bad arguments");
    if (H > SURFEL_SCENE_MAX_EDGE || W > SURFEL_SCENE_MAX_EDGE || H2 > SURFEL_SCENE_MAX_EDGE || W2 > SURFEL_SCENE_MAX_EDGE)
        return api_fail(SURFEL_E_LIMIT, "scene_undistort: an image edge exceeds SURFEL_SCENE_MAX_EDGE");
    for (int k = 0; k < 12; k++)
        if (!isfinite(q[k])) return api_fail(SURFEL_E_INVALID, "scene_undistort: a distortion parameter is not finite");
    for (int k = 0; k < 4; k++)
        if (!isfinite(pinhole[k])) return api_fail(SURFEL_E_INVALID, "scene_undistort: a pinhole parameter is not finite");
    if (!(q[0] > 0.0) || !(q[1] > 0.0) || !(pinhole[0] > 0.0) || !(pinhole[1] > 0.0))
        return api_fail(SURFEL_E_INVALID, "scene_undistort: a focal length is not positive");
    const UndistortParams p = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], pinhole[0], pinhole[1], pinhole[2], pinhole[3]};
    const dim3 grid(blocks_for(W2, UX), blocks_for(H2, UY));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C == 1) hipLaunchKernelGGL(undistort_kernel<1>, grid, dim3(UX * UY), 0, s, H, W, H2, W2, p, src, dst);
    else if (C == 3) hipLaunchKernelGGL(undistort_kernel<3>, grid, dim3(UX * UY), 0, s, H, W, H2, W2, p, src, dst);
    else hipLaunchKernelGGL(undistort_kernel<4>, grid, dim3(UX * UY), 0, s, H, W, H2, W2, p, src, dst);
    return launched("undistort_kernel");
}

}  // extern "C"
