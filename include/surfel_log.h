/*
 * surfel_log.h — C ABI of the training log (LOG.md), part of libsurfel_hip.so (gfx950 only): what the reference's
 * prepare_output_and_logger / training_report (train.py:115-119, 184-248) hand to TensorBoard, without the package and without a
 * host wait in the step.  Three groups:
 *   - the step ring (device):  surfel_log_append, one small launch per step that turns the step's six loss scalars into one record;
 *   - the panels (device):     surfel_log_panel, a map -> interleaved 8-bit pixels as TensorBoard's image summary quantises them;
 *   - the event framing (HOST, no device touched): surfel_log_crc32c, surfel_log_frame, surfel_log_steps_capacity,
 *     surfel_log_encode_steps.  They take HOST pointers and no stream.
 * Conventions of the library (surfel_hip.h): plain DEVICE pointers plus sizes, `stream` = hipStream_t as void*, no allocation inside,
 * return >= 0 or a negative SURFEL_E_* code with the message in surfel_last_error().
 */
#ifndef SURFEL_LOG_H
#define SURFEL_LOG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the step ring ---------------------------------------------------------------------------------------------------------------
 * state (SURFEL_LOG_STATE_BYTES, 8-byte aligned, zeroed by the caller before the first append):
 *   double ema_dist, double ema_normal, int64 count, int64 reserved
 * record (SURFEL_LOG_RECORD_BYTES, little endian, the ring is 4-byte aligned):
 *   int32 iteration | int32 points | float reg_loss | float total_loss | float ema_dist | float ema_normal | float raw_total | uint32 seq
 * with, from scalars6 = [Ll1, ssim, normal_err, dist, photometric, total] (fp32, on the device):
 *   reg_loss = [0] (train.py:119 passes Ll1), total_loss = [4] (it passes `loss`, the photometric term, not total_loss), raw_total = [5]
 *   dist_loss = fp32(lambda_dist * [3]), normal_loss = fp32(lambda_normal * [2])              one fp32 rounding each, denormals kept
 *   ema_x <- fp64(fp64(0.4 * x_loss) + fp64(0.6 * ema_x))                                     two products and a sum, NOT fused
 *   record.ema_x = fp32(ema_x), seq = count mod 2^32; the record goes to slot count mod capacity; count <- count + 1
 */
#define SURFEL_LOG_STATE_BYTES 32
#define SURFEL_LOG_RECORD_BYTES 32

/* One launch of one wave on `stream`; reads scalars6 on the device (valid behind the step's backward), waits for nothing.
 * SURFEL_E_INVALID: a null or misaligned pointer, capacity < 1. */
int surfel_log_append(void* state, void* ring, int capacity, int iteration, int points, const float* scalars6, float lambda_normal,
                      float lambda_dist, void* stream);

/* ---- the panels --------------------------------------------------------------------------------------------------------------------
 * dst[H][W][3] (any byte alignment) <- planes (fp32, 4-byte aligned, [C][H][W] without padding; C = 3 for RGB and NORMAL, 1 otherwise).
 * q(y) = 0 for y NaN or y <= 0, 255 for y >= 255, else y truncated: numpy's (x * 255).clip(0, 255).astype(uint8) of torch's
 * summary.image with NaN -> 0 stated.  Every operation is fp32 and rounds once (no contraction); the divisions are correctly rounded.
 *   RGB        dst[..c] = q(x_c * 255)
 *   GRAY       dst[..c] = q(x * 255) for c = 0, 1, 2                                         (rend_alpha)
 *   NORMAL     dst[..c] = q((x_c * 0.5 + 0.5) * 255)                                        (rend_normal, surf_normal)
 *   TURBO_MAX  m = max over the pixels that are not NaN; t = x / m; dst = TURBO[k(t)]        (surf_depth / surf_depth.max())
 *              m NaN (no such pixel), infinite or <= 0: every pixel is TURBO[0]
 *   JET_MINMAX lo, hi = min, max over the pixels that are not NaN; t = (x - lo) / (hi - lo); dst = JET[k(t)]       (imshow(rend_dist))
 *              no such pixel, lo or hi infinite, or hi == lo: every pixel is JET[0] (matplotlib's Normalize maps a constant image to 0)
 *   k(t) = 0 for t NaN or t * 256 < 1, 255 for t * 256 >= 255, else t * 256 truncated: matplotlib's min(int(t * 256), 255), with its
 *   under-range colour (entry 0) and over-range colour (entry 255)
 * TURBO is the table of the depth frames (RENDER.md), JET the table scripts/gen_jet_table.py derives from matplotlib the same way:
 * the colormap's 256 entries times 255, truncated.  The extrema are merged with integer atomics on an order-preserving key: the bytes
 * do not depend on the order in which workgroups finish.
 * scratch: SURFEL_LOG_PANEL_SCRATCH_BYTES, 4-byte aligned (the two keys).  RGB, GRAY and NORMAL are one launch, the others three.
 * SURFEL_E_INVALID: unknown mode, an edge below 1, a null or misaligned pointer, too little scratch; SURFEL_E_LIMIT: an edge above 65536.
 */
#define SURFEL_LOG_PANEL_RGB 0
#define SURFEL_LOG_PANEL_GRAY 1
#define SURFEL_LOG_PANEL_NORMAL 2
#define SURFEL_LOG_PANEL_TURBO_MAX 3
#define SURFEL_LOG_PANEL_JET_MINMAX 4
#define SURFEL_LOG_PANEL_SCRATCH_BYTES 64

int surfel_log_panel(int mode, int H, int W, const float* planes, uint8_t* dst, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- the event framing (host) -----------------------------------------------------------------------------------------------------
 * A TensorBoard event file is a sequence of TFRecords:  u64 length | u32 mask(crc32c(length bytes)) | payload | u32 mask(crc32c(payload)),
 * little endian, mask(c) = ((c >> 15 | c << 17) + 0xa282ead8) mod 2^32.  A payload is a serialised Event (LOG.md lists the field numbers).
 */

/* CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of data[0 .. n); 0 for n = 0 */
uint32_t surfel_log_crc32c(const void* data, int64_t n);

/* out[0 .. n + 16) <- the TFRecord of payload[0 .. n); returns n + 16, or SURFEL_E_INVALID (null pointer, n < 0).  out must not overlap payload. */
int64_t surfel_log_frame(const void* payload, int64_t n, void* out);

/* an upper bound of what surfel_log_encode_steps writes for n records */
int64_t surfel_log_steps_capacity(int64_t n);

/*
 * records[n] (SURFEL_LOG_RECORD_BYTES each, HOST memory) -> n TFRecords in out, one Event per record:
 *   Event { wall_time (1, double) = wall_time, step (2, varint) = iteration [omitted when 0, as proto3 does],
 *           summary (5) { value (1) { tag (1), simple_value (2, float) } x 6 } }
 * with the reference's tags in the order it writes them: train_loss_patches/dist_loss = ema_dist, train_loss_patches/normal_loss =
 * ema_normal, train_loss_patches/reg_loss, train_loss_patches/total_loss, iter_time = iter_time_ms, total_points = (float)points.
 * Returns the bytes written; SURFEL_E_INVALID for a null pointer, n < 0 or a negative iteration; SURFEL_E_LIMIT when out_capacity is
 * too small (nothing useful is in out then).
 */
int64_t surfel_log_encode_steps(const void* records, int64_t n, float iter_time_ms, double wall_time, void* out, int64_t out_capacity);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_LOG_H */
