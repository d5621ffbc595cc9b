/*
 * surfel_undistort.h — C ABI of the capture loader's undistortion (UNDISTORT.md), part of libsurfel_hip.so (gfx950 only).  It belongs
 * to the loader entries of surfel_scene.h and keeps their conventions: plain DEVICE pointers and sizes for the images, `stream` =
 * hipStream_t as void*, no allocation inside the library, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Images are 8-bit, interleaved [H][W][C] with C = 1, 3 or 4 and no row padding.
 *
 * What the entry replaces: COLMAP's image_undistorter, which the reference's convert.py:68-78 shells out to before a capture can be
 * trained on.
 */
#ifndef SURFEL_UNDISTORT_H
#define SURFEL_UNDISTORT_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * dst[H2][W2][C] <- src[H][W][C] seen through the pinhole camera pinhole[4] = (fx2, fy2, cx2, cy2), where src was taken with the
 * distorted camera q[12] = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6).  q and pinhole are HOST arrays, read before the call returns
 * and passed to the launch by value; there are no device tables.  Per output pixel (x, y), in fp64 without contraction:
 *   u = (x + 0.5 - cx2) / fx2, v = (y + 0.5 - cy2) / fy2
 *   r2 = u*u + v*v, r4 = r2*r2, r6 = r4*r2, rad = (1 + k1*r2 + k2*r4 + k3*r6) / (1 + k4*r2 + k5*r4 + k6*r6), uv = u*v
 *   ud = u*rad + 2*p1*uv + p2*(r2 + 2*u*u), vd = v*rad + 2*p2*uv + p1*(r2 + 2*v*v)
 *   xs = fx*ud + cx - 0.5, ys = fy*vd + cy - 0.5, x0 = floor(xs), y0 = floor(ys), dx = xs - x0, dy = ys - y0
 *   valid <=> 0 <= x0 and x0 + 1 <= W - 1 and 0 <= y0 and y0 + 1 <= H - 1      (a NaN compares false: invalid)
 *   per channel: top = (1-dx)*s[y0][x0] + dx*s[y0][x0+1], bot likewise on row y0 + 1, val = (1-dy)*top + dy*bot, out = floor(val + 0.5)
 *   invalid: every channel 0 (for C = 4 the alpha too, so the pixel is masked)
 * Nothing outside src[0 .. H*W*C) is read, whatever q holds.
 * SURFEL_E_LIMIT when an edge exceeds SURFEL_SCENE_MAX_EDGE; SURFEL_E_INVALID for C other than 1, 3, 4, an edge below 1, a parameter
 * that is not finite, or a focal length (q[0], q[1], pinhole[0], pinhole[1]) that is not positive.
 */
int surfel_scene_undistort(int H, int W, int C, int H2, int W2, const double* q, const double* pinhole, const uint8_t* src, uint8_t* dst,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_UNDISTORT_H */
