/*
 * surfel_select.h — C ABI of the label pass (SELECT.md), part of libsurfel_hip.so (gfx950 only): per-surfel, per-label sums of the
 * blend weights w = alpha * T a rendered view composited, the weight of every pair routed by a per-pixel label image.  Same conventions
 * as surfel_hip.h: plain DEVICE pointers, `stream` = hipStream_t as void*, return >= 0 or a negative SURFEL_E_* code with the message
 * in surfel_last_error().
 *
 * Nothing of the reference is replaced: it has no segmentation.  The sums are the votes of FlashSplat ("2D to 3D Gaussian splatting
 * segmentation solved optimally"): under linear blending the optimal label of a surfel is the arg-max of its votes over the labels.
 */
#ifndef SURFEL_SELECT_H
#define SURFEL_SELECT_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* votes count blend weights in units of 2^-SURFEL_SELECT_FRAC_BITS (the contribution pass's unit): sum of w = votes / 2^24 */
#define SURFEL_SELECT_FRAC_BITS 24
#define SURFEL_SELECT_MAX_LABELS 32
/* by convention the label of a pixel that says nothing (any label >= num_labels is ignored) */
#define SURFEL_SELECT_UNLABELLED 255

/*
 * Runs after surfel_rasterize_forward, on that forward's three buffers (R = its return value), the way surfel_rasterize_contribution
 * does.  The frame must be EXACTLY counted (rendered with SURFEL_OPT_EXACT_BINNING): a capacity-binned or lazily counted frame is
 * SURFEL_E_INVALID.  The tile lists are walked again with the forward's pair test, transmittance recurrence and termination rule
 * (T (1 - alpha) < 1e-4 ends the pixel; the terminating surfel is not composited), so the composited (pixel, surfel) pairs are the
 * forward's.  For every composited pair at a pixel with labels[y, x] = k < num_labels, with w = alpha * T (fp32, the forward's bits):
 *     votes[id * num_labels + k] += rint(w * 2^24)
 * A pixel with labels[y, x] >= num_labels votes for nothing.  labels holds height * width bytes (no padding is read).  votes holds
 * P * num_labels elements, row-major, is zeroed by the caller once and accumulated across calls.  Integer accumulators only: the same
 * bytes on every run and for every order of views.  With no pixel ignored, the sum of a row of votes is the contribution pass's sum_q.
 * P == 0 or R == 0 returns 0 and touches nothing.  num_labels outside 1 .. 32, or a NULL labels or votes, is SURFEL_E_INVALID.
 * The call waits for the stream once (it reads the frame's counting mode back).  debug: reserved, pass 0.
 */
int surfel_rasterize_label_votes(int P, int64_t R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                                 const void* image_buffer, const uint8_t* labels, int num_labels, uint64_t* votes, int debug,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_SELECT_H */
