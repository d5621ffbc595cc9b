/*
 * surfel_view.h — C ABI of the live viewer's image kernels (VIEWER.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_vis.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library (scratch comes from the caller), return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Nothing here waits for the device, and no value visits the host.
 *
 * What they replace in the reference: utils/image_utils.py:23-61 (`gradient_map`, `colormap`, `render_net_image`) and the
 * `(clamp(img, 0, 1) * 255).byte().permute(1, 2, 0)` in front of the socket (train.py:156, view.py:26) for the four render modes
 * that show a scalar map in turbo colours: Alpha, Depth (the map is an input plane) and Edge, Curvature (the map is the gradient
 * magnitude of three planes).  The two remaining modes, RGB and Normal, are surfel_vis_quantize(3, ..., 1, 0) and (3, ..., 0.5, 0.5).
 *
 * Colouring of a map m[H][W], all fp32, one rounding per operation:
 *   lo = min m, hi = max m over the pixels that are not NaN (exact: min and max do not depend on the order of reduction)
 *   t = (m - lo) / (hi - lo);  idx = rintf(t * 255) (half to even);  pixel = TURBO[idx] (csrc/vis_turbo_table.h)
 *   a pixel whose t is NaN takes TURBO[0]: a NaN pixel, a constant map (hi == lo), a map without a finite range (+-inf in it, or
 *   nothing but NaN).  The reference indexes its table with NaN.long() there, which is undefined.
 *
 * Images have no row padding.  u8 outputs may start at any byte address; float inputs and the scratch need 4-byte alignment only.
 * H == 1 and W == 1 are ordinary sizes.
 */
#ifndef SURFEL_VIEW_H
#define SURFEL_VIEW_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of scratch an H x W image needs: the two 32-bit keys of lo and hi (in a 64-byte block) and, for surfel_view_gradient, the map.
 * The scratch needs no initialisation and holds nothing a later call depends on.
 */
#define SURFEL_VIEW_SCRATCH_BYTES(H, W) (64 + 4 * (int64_t)(H) * (int64_t)(W))

/* dst[H][W][3] (u8) <- turbo colours of map[H][W] (Alpha: rend_alpha, Depth: surf_depth).  Launches: key reset, min / max, colouring. */
int surfel_view_scalar(int H, int W, const float* map, uint8_t* dst, void* scratch, int64_t scratch_bytes, void* stream);

/*
 * dst[H][W][3] (u8) <- turbo colours of the gradient magnitude of planes[3][H][W] (Edge: render with scale 1, bias 0; Curvature:
 * rend_normal with scale 0.5, bias 0.5).  Per channel v = p * scale + bias (two roundings), pixels outside the image read as 0 (the
 * zero padding follows the scale and bias), a..i = the 3 x 3 neighbourhood in row-major order:
 *   gx = ((c - a) * 0.25 + (f - d) * 0.5) + (i - g) * 0.25
 *   gy = ((g - a) * 0.25 + (h - b) * 0.5) + (i - c) * 0.25
 *   s = (gx0^2 + gy0^2) + (gx1^2 + gy1^2) + (gx2^2 + gy2^2);  m = sqrtf(s)
 * Launches: key reset; one that computes m from an LDS tile with a one-pixel halo, stores it to the scratch and reduces min / max
 * (per wave, then one atomic min and one atomic max per workgroup on the order-preserving key); colouring.
 */
int surfel_view_gradient(int H, int W, const float* planes, float scale, float bias, uint8_t* dst, void* scratch, int64_t scratch_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_VIEW_H */
