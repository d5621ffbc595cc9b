/*
 * surfel_scene.h — C ABI of the capture loader's image path (SCENE.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_train.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library, return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in surfel_last_error().  Integer arithmetic
 * throughout the resampling; the only floating-point results are v / 255 (IEEE division) and the fp64 composite.
 *
 * What each entry replaces in the reference (Pillow / numpy / torch on the host there):
 *   surfel_scene_resample_table   Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BICUBIC filter (what
 *                                 utils/general_utils.py:22 `pil_image.resize(resolution)` runs with), one axis
 *   surfel_scene_resample_h       its horizontal pass on 8-bit channels
 *   surfel_scene_resample_v       its vertical pass, on the 8-bit result of the horizontal one
 *   surfel_scene_to_float         utils/general_utils.py:23-27 (`/ 255.0`, HWC -> CHW) and utils/camera_utils.py:41-44 (the alpha split)
 *   surfel_scene_composite        scene/dataset_readers.py:204-210 (RGBA over a black or white background)
 *
 * Images are 8-bit, interleaved [H][W][C] with C = 1, 3 or 4 and no row padding.  The float output is planar: planes[min(C, 3)][H][W],
 * plus mask[1][H][W] from the fourth channel when C = 4.
 */
#ifndef SURFEL_SCENE_H
#define SURFEL_SCENE_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fixed-point position of the resampling weights (Pillow's PRECISION_BITS for 8-bit channels). */
#define SURFEL_SCENE_PRECISION_BITS 22
/* Largest number of taps per output sample: ksize = 2 * ceil(2 * max(in / out, 1)) + 1, so 193 admits every reduction up to 48 x. */
#define SURFEL_SCENE_MAX_KSIZE 193
/* Largest image edge, source or result. */
#define SURFEL_SCENE_MAX_EDGE 32768

/*
 * Host function, touches no device.  Returns ksize, the taps per output sample of resampling one axis from in_size to out_size samples.
 * With bounds and coeffs non-NULL it also fills bounds[out_size][2] = (first source sample, taps used) and coeffs[ksize][out_size]
 * (weights times 2^22, rounded half away from zero; the taps behind `taps used` are 0; tap-major, so that lanes which own consecutive
 * output samples read consecutive ints).  capacity = ints available behind coeffs.
 * SURFEL_E_LIMIT when ksize exceeds SURFEL_SCENE_MAX_KSIZE or an edge SURFEL_SCENE_MAX_EDGE; SURFEL_E_INVALID when capacity is short.
 */
int surfel_scene_resample_table(int in_size, int out_size, int* bounds, int* coeffs, int64_t capacity);

/*
 * Horizontal pass src[H][W][C] -> [H][W2][C]: per output sample 2^21 + sum of src * coeff in int32, shifted right by 22 (arithmetic),
 * clipped to 0..255.  bounds / coeffs: the DEVICE copy of surfel_scene_resample_table(W, W2).  The result goes to dst_u8 when that is
 * non-NULL (an intermediate), else as v / 255 to dst_planes (and dst_mask when C = 4).
 */
int surfel_scene_resample_h(int H, int W, int C, int W2, int ksize, const uint8_t* src, const int* bounds, const int* coeffs,
                            uint8_t* dst_u8, float* dst_planes, float* dst_mask, void* stream);

/* Vertical pass src[H][W][C] -> [H2][W][C], the same arithmetic down the columns with the table of (H, H2); outputs as above. */
int surfel_scene_resample_v(int H, int W, int C, int H2, int ksize, const uint8_t* src, const int* bounds, const int* coeffs,
                            uint8_t* dst_u8, float* dst_planes, float* dst_mask, void* stream);

/* dst_planes[min(C, 3)][H][W] (and dst_mask[H][W] when C = 4) <- (float)v / 255.0f, correctly rounded, of src[H][W][C]. */
int surfel_scene_to_float(int H, int W, int C, const uint8_t* src, float* dst_planes, float* dst_mask, void* stream);

/*
 * dst[H][W][3] <- src[H][W][4] over a black (white = 0) or white background, in fp64 without contraction:
 * n = v / 255.0, arr = n_c * n_a + bg * (1 - n_a), out = arr * 255.0 truncated towards zero.
 */
int surfel_scene_composite(int H, int W, int white, const uint8_t* src, uint8_t* dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_SCENE_H */
