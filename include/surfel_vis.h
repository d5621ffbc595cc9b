/*
 * surfel_vis.h — C ABI of the frame kernels of the trajectory renderer (RENDER.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_scene.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library (the one entry that needs scratch takes it from the caller), return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with
 * the message in surfel_last_error().  Nothing here waits for the device.
 *
 * What each entry replaces in the reference (numpy / matplotlib on the host there, after a device-to-host copy of fp32 frames):
 *   surfel_vis_quantize      utils/render_utils.py:270-275 `save_img_u8` (and the `* 0.5 + 0.5` in front of it for normal maps,
 *                            utils/mesh_utils.py:294), fused with the CHW -> HWC permute
 *   surfel_vis_order_stats   the selection inside np.percentile(depth, [p, 100 - p]) of create_videos (render_utils.py:219)
 *   surfel_vis_depth_turbo   the depth frame of create_videos (render_utils.py:261-266): log, normalise, turbo colormap, 8 bits
 *
 * Images have no row padding.  u8 outputs may start at any byte address; float inputs need their natural 4-byte alignment only.
 */
#ifndef SURFEL_VIS_H
#define SURFEL_VIS_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest number of order statistics one surfel_vis_order_stats call selects. */
#define SURFEL_VIS_MAX_RANKS 8
/* Bytes of scratch surfel_vis_order_stats needs (8 histograms of 256 counters and the selection state); 4-byte aligned. */
#define SURFEL_VIS_ORDER_SCRATCH_BYTES 8448

/*
 * dst[H][W][C] (u8, interleaved) <- planes[C][H][W] (fp32, planar), C = 1 or 3.  Per value, in fp32 with separate roundings:
 * y = v * scale + bias; NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX; clip to [0, 1]; times 255; truncated towards zero.
 */
int surfel_vis_quantize(int C, int H, int W, const float* planes, float scale, float bias, uint8_t* dst, void* stream);

/*
 * out[j] (device, j < m) <- the ranks[j]-th smallest (0-based) of x[n] in numpy's sort order: -inf < ... < -0 = +0 < ... < +inf < NaN
 * (-0 and +0 compare equal; which of the two a tie returns is unspecified; every NaN comes back as the canonical quiet NaN).
 * ranks: HOST array, ascending (repeats allowed), each in [0, n); 1 <= m <= SURFEL_VIS_MAX_RANKS; 1 <= n < 2^32.
 * Exact selection: four passes over x, each a 256-bin histogram of one byte of the order-preserving 32-bit key restricted to the
 * elements that share the bytes already decided (LDS counters, merged with integer atomics), each followed by a one-workgroup kernel
 * that picks the bin on the device.  No sort, no host round trip, no floating-point arithmetic: bit-identical from run to run.
 * scratch: SURFEL_VIS_ORDER_SCRATCH_BYTES device bytes; it needs no initialisation and holds nothing afterwards.
 */
int surfel_vis_order_stats(int64_t n, const float* x, int m, const int64_t* ranks, float* out, void* scratch, int64_t scratch_bytes,
                           void* stream);

/*
 * dst[H][W][3] (u8) <- turbo colours of depth[H][W]: x = logf(depth) in fp32; t = ((double)x - min(lo, hi)) / |hi - lo| in fp64,
 * clipped to [0, 1]; a NaN t gives (0, 0, 0); otherwise TURBO[min((int)(t * 256), 255)] (csrc/vis_turbo_table.h).
 */
int surfel_vis_depth_turbo(int H, int W, const float* depth, double lo, double hi, uint8_t* dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_VIS_H */
