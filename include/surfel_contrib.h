/*
 * surfel_contrib.h — C ABI of the contribution pass (CONTRIB.md), part of libsurfel_hip.so (gfx950 only): per-surfel statistics of
 * the blend weights w = alpha * T a rendered view composited.  Same conventions as surfel_hip.h: plain DEVICE pointers, `stream` =
 * hipStream_t as void*, return >= 0 or a negative SURFEL_E_* code with the message in surfel_last_error().
 *
 * Nothing of the reference is replaced: it prunes by opacity and screen size only (scene/gaussian_model.py).  The statistics are the
 * scores of LightGaussian (sum of blend weights), RadSplat (maximum blend weight) and Mini-Splatting (pixels dominated).
 */
#ifndef SURFEL_CONTRIB_H
#define SURFEL_CONTRIB_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sum_q counts blend weights in units of 2^-SURFEL_CONTRIB_FRAC_BITS: sum of w = sum_q / 2^24 */
#define SURFEL_CONTRIB_FRAC_BITS 24

/*
 * Runs after surfel_rasterize_forward, on that forward's three buffers (R = its return value), the way the backward does.  The frame
 * must be EXACTLY counted (rendered with SURFEL_OPT_EXACT_BINNING): a capacity-binned or lazily counted frame is SURFEL_E_INVALID.
 * The tile lists are walked again with the forward's pair test, transmittance recurrence and termination rule (T (1 - alpha) < 1e-4
 * ends the pixel; the terminating surfel is not composited), so the composited (pixel, surfel) pairs are the forward's.  For every
 * composited pair, with w = alpha * T (fp32, the forward's bits):
 *     sum_q[id]    += rint(w * 2^24)             hits[id] += 1             max_bits[id] = max(max_bits[id], bits of w)
 *     dominant[id] += 1 for the pixel's heaviest composited surfel (a tie goes to the nearer one, the first in list order)
 *     views[id]    += 1 once per view_tag if the surfel composited OR terminated a pixel of this view (stamp[id] = last tag seen)
 * The six arrays hold P elements each, are zeroed by the caller once and accumulated across calls; view_tag >= 1 and rises from call
 * to call for one set of arrays.  dominant_id[height, width] (or NULL) receives this view's heaviest surfel per pixel, -1 = none.
 * Integer accumulators only: the same bytes on every run and for every order of views.  P == 0 or R == 0 returns 0 and touches nothing.
 * The call waits for the stream once (it reads the frame's counting mode back).  debug: reserved, pass 0.
 */
int surfel_rasterize_contribution(int P, int64_t R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                                  const void* image_buffer, uint32_t view_tag, uint64_t* sum_q, uint64_t* hits, uint32_t* max_bits,
                                  uint32_t* dominant, uint32_t* views, uint32_t* stamp, int32_t* dominant_id, int debug, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_CONTRIB_H */
