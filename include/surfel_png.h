/*
 * surfel_png.h — C ABI of the PNG encoder behind the per-frame exports (PNG.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_jpeg.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library (the scratch comes from the caller), return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Nothing here waits for the device.
 *
 * One call turns one interleaved 8-bit gray (C = 1, colour type 0) or RGB (C = 3, colour type 2) frame into one complete PNG file:
 * signature, IHDR, one IDAT chunk, IEND; bit depth 8, no interlace.  The scanlines take the adaptive filter with the smallest sum
 * of absolute residuals; the filtered stream is cut into stripes of whole rows, each compressed on its own into one dynamic-Huffman
 * deflate block whose only matches have distance 1.  PNG.md states every rule, operation by operation; tests/png_oracle.py restates
 * them in numpy and the file is equal to that restatement byte for byte.
 */
#ifndef SURFEL_PNG_H
#define SURFEL_PNG_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes in front of the deflate data: signature 8, IHDR chunk 25, IDAT length and type 8, zlib header 2. */
#define SURFEL_PNG_FRONT_BYTES 43
/* A stripe is the smallest number of whole filtered rows (1 + W * C bytes each) that reaches this many bytes; the last is shorter. */
#define SURFEL_PNG_STRIPE_BYTES 32768
/* Limits that keep every 32-bit offset and bit count inside the library in range: a filtered row (1 + W * C) holds at most 2^20
 * bytes and the filtered stream H * (1 + W * C) at most 2^30.  A frame beyond either is SURFEL_E_LIMIT. */
#define SURFEL_PNG_MAX_ROW (1 << 20)
#define SURFEL_PNG_MAX_STREAM (1 << 30)
/* Bits of a stripe beyond its literals and matches: the block header (3 + 5 + 5 + 4, 19 * 3 code-length-code lengths, 287 code
 * lengths of at most 7 bits: a repeat symbol with its extra bits costs at most 14 and stands for at least 3), the end-of-block (15),
 * and behind every stripe but the last the empty stored block (3 bits, at most 7 of padding, 32 of LEN / NLEN): 2083 + 15 + 42. */
#define SURFEL_PNG_STRIPE_EXTRA_BITS 2140

/*
 * Upper bound of the file size of an H x W x C frame.  With stripes of L_s filtered bytes (L_s = rows of the stripe * (1 + W * C)):
 *   no byte costs more than 15 bits as a literal (the literal/length code is limited to 15 bits);
 *   a match covers at least 3 bytes and costs at most 15 (length code) + 5 (extra bits) + 1 (distance code) = 21 bits, 7 per byte;
 *   so a stripe holds at most 15 * L_s + SURFEL_PNG_STRIPE_EXTRA_BITS bits, rounded up to whole 32-bit words: cap(L_s) bytes;
 *   the fixed parts: SURFEL_PNG_FRONT_BYTES in front, Adler-32 (4), the IDAT CRC (4) and IEND (12) behind.
 * capacity = 43 + sum over the stripes of cap(L_s) + 20, cap(L) = ((15 * L + 2140 + 31) / 32) * 4.
 * A bad size returns SURFEL_E_INVALID / SURFEL_E_LIMIT.
 */
int64_t surfel_png_capacity(int H, int W, int C);

/*
 * Bytes of scratch surfel_png_encode needs for an H x W x C frame (host arithmetic only; a multiple of 16): the filtered stream
 * (1 byte per byte), one 16-bit token per byte, 8 bytes of Adler partial sums per row, per stripe a 288-word histogram, a 288-word
 * code table and 32 bytes of totals, and the stripes' zeroed bit buffers (cap(L_s) bytes each).
 */
int64_t surfel_png_scratch_bytes(int H, int W, int C);

/*
 * dst[0 .. *size) <- the PNG file of pix[H][W][C] (u8, interleaved, no row padding), C = 1 or 3.
 * pix and dst may start at any byte address; size: one 8-byte aligned DEVICE word that receives the file's length; scratch: 8-byte
 * aligned, needs no initialisation and holds nothing afterwards.  capacity < surfel_png_capacity(H, W, C) or scratch_bytes <
 * surfel_png_scratch_bytes(H, W, C) is SURFEL_E_INVALID, decided on the host before any launch.  No byte of dst at or beyond *size is
 * written.  The bytes depend on the arguments only: the same on every run.
 */
int surfel_png_encode(int H, int W, int C, const uint8_t* pix, uint8_t* dst, int64_t capacity, int64_t* size, void* scratch,
                      int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_PNG_H */
