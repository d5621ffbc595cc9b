/*
 * surfel_metrics.h — C ABI of the image-quality evaluation (METRICS.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_train.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library (the caller carves the workspace whose size surfel_lpips_workspace_bytes reports), return >= 0 or a negative SURFEL_E_*
 * code (surfel_hip.h) with the message in surfel_last_error().  No float atomics: every sum is a per-workgroup partial, reduced in
 * a fixed order by surfel_reduce_partials (surfel_train.h), so two runs give the same bits.  SSIM is surfel_l1_ssim_forward_w.
 *
 * What each entry replaces in the reference (torch / torchvision there):
 *   surfel_lpips_prepare      lpipsPyTorch/modules/networks.py:41-51 (z-score), for both images of a pair
 *   surfel_lpips_conv3x3      the 13 Conv2d(3x3, padding 1) + ReLU of torchvision's vgg16().features (networks.py:92)
 *   surfel_lpips_pool         its MaxPool2d(2, 2)
 *   surfel_lpips_tap          modules/utils.py:6-8 (normalize_activation) and modules/lpips.py:33-34 ((fx - fy)^2, 1x1 conv, mean)
 *   surfel_sq_err_partials    utils/image_utils.py:20 (the squared error behind psnr)
 *
 * Activations are channels-last and hold BOTH images of a pair: act[2][H][W][C] (image 0 = x, image 1 = y), C a multiple of 4.
 */
#ifndef SURFEL_METRICS_H
#define SURFEL_METRICS_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Partial sums surfel_lpips_tap and surfel_sq_err_partials write (always all of them; unused workgroups write 0). */
#define SURFEL_METRICS_PARTIALS 1024
/* Channels of the prepared image: R, G, B and one zero. */
#define SURFEL_LPIPS_IN_CHANNELS 4
/* Largest image edge. */
#define SURFEL_LPIPS_MAX_EDGE 16384

/*
 * Bytes of the workspace of one H x W pair: two activation buffers of 2 * H * W * 64 floats each (relu1_1 and relu1_2 of both images,
 * the peak; every later layer fits in the same two), each rounded up to 256 bytes, then 6 * SURFEL_METRICS_PARTIALS floats of
 * partial sums.  Touches no device.  SURFEL_E_LIMIT when an edge exceeds SURFEL_LPIPS_MAX_EDGE or the result exceeds budget_bytes.
 */
int64_t surfel_lpips_workspace_bytes(int H, int W, int64_t budget_bytes);

/* out[2][H][W][4] <- ((v - mean_c) / std_c for c = R, G, B; 0) of x[3][H][W] (image 0) and y[3][H][W] (image 1), planar fp32. */
int surfel_lpips_prepare(int H, int W, const float* x, const float* y, float* out, void* stream);

/*
 * out[2][H][W][cout] <- relu(bias + conv3x3(in[2][H][W][cin], zero padding 1)) as an implicit GEMM on the f32-input MFMA
 * (M = pixels, N = cout, K = 9 * cin, summed tap by tap and channel by channel inside a tap).
 * weight[9][cin][cout]: tap (ky * 3 + kx) first, cout contiguous (the transpose of torch's [cout][cin][3][3]).
 * cin: 4 or a multiple of 16; cout: a multiple of 64.  A first layer passes cin = 4 with a zero fourth channel (K = 36).
 */
int surfel_lpips_conv3x3(int H, int W, int cin, int cout, const float* in, const float* weight, const float* bias, float* out, void* stream);

/* out[2][H / 2][W / 2][C] <- the maximum of every 2 x 2 block of in[2][H][W][C]; an odd last row / column is dropped.  C % 4 == 0. */
int surfel_lpips_pool(int H, int W, int C, const float* in, float* out, void* stream);

/*
 * partials[SURFEL_METRICS_PARTIALS] <- per-workgroup sums over pixels of sum_c lin[c] * (fx_c / (|fx| + 1e-10) - fy_c / (|fy| + 1e-10))^2,
 * fx = feat[0][y][x][:], fy = feat[1][y][x][:], |f| = sqrt(sum_c f_c^2).  C: 64, 128, 256 or 512.  The layer's term is their sum
 * (fixed order) divided by H * W.
 */
int surfel_lpips_tap(int H, int W, int C, const float* feat, const float* lin, float* partials, void* stream);

/* partials[SURFEL_METRICS_PARTIALS] <- per-workgroup sums of (a[i] - b[i])^2 over i < n. */
int surfel_sq_err_partials(int64_t n, const float* a, const float* b, float* partials, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_METRICS_H */
