/*
 * surfel_jpeg.h — C ABI of the baseline JPEG encoder behind the trajectory videos (VIDEO.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_vis.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library (the scratch comes from the caller), return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Nothing here waits for the device.
 *
 * One call turns one interleaved 8-bit RGB frame into one complete JFIF file: baseline sequential DCT, 4:2:0, the Annex K tables of
 * ITU-T T.81, one restart interval per MCU row.  VIDEO.md states every rule, operation by operation; tests/video_oracle.py restates
 * them in numpy and the file is equal to that restatement byte for byte.
 */
#ifndef SURFEL_JPEG_H
#define SURFEL_JPEG_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes in front of the entropy-coded data: SOI, APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS. */
#define SURFEL_JPEG_HEADER_BYTES 629
/* Largest image edge (SOF0 holds 16-bit sizes). */
#define SURFEL_JPEG_MAX_EDGE 65535

/*
 * Upper bound of the file size of an H x W frame at any quality, header included.  With R = ceil(H / 16) MCU rows of M = ceil(W / 16)
 * MCUs of 6 blocks:
 *   a block holds 64 coefficients, and none costs more than 26 bits: the longest AC code has 16 bits and carries 10 magnitude bits
 *   (the DC code has at most 9 + 11; a ZRL code, 11 bits, stands for 16 zero coefficients that cost nothing else; the EOB, 4 bits,
 *   stands for at least one): 64 * 26 bits = 208 bytes per block, 1248 per MCU;
 *   every byte may be 0xFF and then takes a stuffed zero behind it: times 2;
 *   a row ends with less than one byte of padding (stuffed: 2 bytes) and a 2-byte RSTm marker (the last row with EOI instead).
 * capacity = SURFEL_JPEG_HEADER_BYTES + R * (M * 2496 + 4).  A bad size returns SURFEL_E_INVALID / SURFEL_E_LIMIT.
 */
int64_t surfel_jpeg_capacity(int H, int W);

/*
 * Bytes of scratch surfel_jpeg_encode needs for an H x W frame (host arithmetic only; a multiple of 16): the quantised coefficients
 * (128 B per block), one unstuffed bit buffer of M * 1248 bytes per MCU row, one 32-bit length / offset per block and 16 bytes of
 * totals per row.
 */
int64_t surfel_jpeg_scratch_bytes(int H, int W);

/*
 * dst[0 .. *size) <- the JFIF file of rgb[H][W][3] (u8, interleaved, no row padding) at `quality` (1 .. 100; VIDEO.md).
 * rgb and dst may start at any byte address; size: one 8-byte aligned DEVICE word that receives the file's length; scratch: 8-byte
 * aligned, needs no initialisation and holds nothing afterwards.  capacity < surfel_jpeg_capacity(H, W) or scratch_bytes <
 * surfel_jpeg_scratch_bytes(H, W) is SURFEL_E_INVALID, decided on the host before any launch.  No byte of dst at or beyond *size is
 * written.  The bytes depend on the arguments only: the same on every run.
 */
int surfel_jpeg_encode(int H, int W, const uint8_t* rgb, int quality, uint8_t* dst, int64_t capacity, int64_t* size, void* scratch,
                       int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_JPEG_H */
