/*
 * surfel_jpegdec.h — C ABI of the baseline JPEG decoder behind capture loading (JPEGDEC.md), part of libsurfel_hip.so (gfx950 only).
 * Same conventions as surfel_png.h: plain DEVICE pointers and sizes, `stream` = hipStream_t as void*, no allocation inside the
 * library (the scratch comes from the caller), return >= 0 or a negative SURFEL_E_* code (surfel_hip.h) with the message in
 * surfel_last_error().  Nothing here waits for the device: what the decoder finds out about the stream (converged, not converged,
 * damaged) lands in a device status word.
 *
 * The host walks the file's segments and fills the descriptor (surfel_jpegdec.parse in Python); the whole file is uploaded once; the
 * device unstuffs the entropy-coded segment, decodes it with a self-synchronising parallel Huffman decoder, sums the DC differences,
 * and runs libjpeg's ISLOW inverse DCT, its fancy upsampling and its YCbCr -> RGB conversion.  JPEGDEC.md states every rule, operation
 * by operation; tests/jpegdec_oracle.py restates them in numpy, and the pixels are bit for bit those of libjpeg-turbo 3.1 (Pillow).
 * Integer arithmetic only, and no read-modify-write on pixels or coefficients: the bytes are the same on every run.
 */
#ifndef SURFEL_JPEGDEC_H
#define SURFEL_JPEGDEC_H

#include <stddef.h>
#include <stdint.h>

#include "surfel_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits: an edge of at most 32768 pixels, an entropy-coded segment below 2^28 bytes (every bit position fits 32 bits), subsequences
 * of 32 .. 65536 bits and at most 64 synchronisation rounds.  Beyond them: SURFEL_E_LIMIT. */
#define SURFEL_JPEGDEC_MAX_EDGE 32768
#define SURFEL_JPEGDEC_MAX_ECS (1 << 28)
#define SURFEL_JPEGDEC_MAX_ROUNDS 64

/* status[0] */
#define SURFEL_JPEGDEC_OK 0
#define SURFEL_JPEGDEC_NOT_CONVERGED 1     /* no round within max_rounds left every stored state as it was */
#define SURFEL_JPEGDEC_DAMAGED 2           /* the restart markers or the decoded blocks are not the counts the frame header implies, an
                                            * interval ends inside a block, or no EOI marker follows the data */

/* stages of surfel_jpegdec_decode (bits of `stages`); SURFEL_JPEGDEC_ALL runs the decoder.  A call with a later stage alone continues
 * in the scratch an earlier call with the same arguments left (scripts/jpegdec_bench.py times the stages this way). */
#define SURFEL_JPEGDEC_CLEAN 1             /* unstuffing, restart markers, end of data; the subsequences; the code tables */
#define SURFEL_JPEGDEC_HUFFMAN 2           /* the synchronisation rounds */
#define SURFEL_JPEGDEC_WRITE 4             /* block counts, their scan, the coefficients */
#define SURFEL_JPEGDEC_DC 8                /* DC sums */
#define SURFEL_JPEGDEC_IDCT 16             /* dequantisation and inverse DCT into the component planes */
#define SURFEL_JPEGDEC_COLOUR 32           /* upsampling, colour conversion, the status word */
#define SURFEL_JPEGDEC_ALL 63

/*
 * What the host's parser found (a HOST structure, passed by pointer and copied by the call).  Baseline / extended sequential Huffman
 * (SOF0, SOF1), 8 bits, one interleaved scan; ncomp 1 (hs = vs = 1) or 3 (component ids 1, 2, 3; luma sampling hs x vs = 1x1, 2x1 or
 * 2x2; chroma 1x1).  Tables 0, 1 are the DC tables 0, 1 and tables 2, 3 the AC tables 0, 1, each as DHT carries it (BITS, HUFFVAL).
 * The entropy-coded segment runs from behind the SOS header to the end of the file; the device finds its end.
 */
typedef struct surfel_jpegdec_desc {
    int32_t width, height;
    int32_t ncomp;
    int32_t hs, vs;
    int32_t restart_interval;              /* MCUs per restart interval; 0: none */
    int64_t ecs_offset, ecs_bytes;
    uint8_t tq[4], td[4], ta[4];           /* per component: quantisation table, DC table (0, 1), AC table (0, 1) */
    uint16_t qt[4][64];                    /* natural (row-major) order */
    uint8_t bits[4][16];
    uint8_t huffval[4][256];
} surfel_jpegdec_desc;

/* Bytes of scratch surfel_jpegdec_decode needs (host arithmetic only; a multiple of 16), or SURFEL_E_INVALID / SURFEL_E_LIMIT. */
int64_t surfel_jpegdec_scratch_bytes(const surfel_jpegdec_desc* desc, int subseq_bits);

/*
 * out[height][width][ncomp] (u8, interleaved: gray or RGB) <- the pixels of file[0 .. file_bytes), the file `desc` describes.
 * file and out may start at any byte address; scratch: 16-byte aligned, at least surfel_jpegdec_scratch_bytes(desc, subseq_bits),
 * needs no initialisation; status: four 4-byte aligned DEVICE words: {SURFEL_JPEGDEC_OK / _NOT_CONVERGED / _DAMAGED, rounds used,
 * subsequences, blocks counted}, written by the last stage.  `out` holds the file's pixels only when status[0] is SURFEL_JPEGDEC_OK.
 * max_rounds rounds are launched with no host wait in between; "rounds used" is the first round that changed no stored state.  Every
 * index the stream yields is clamped to the counts the descriptor implies, so a wrong or truncated stream is a status, never an
 * access outside file, scratch or out.  The bytes depend on the arguments only: the same on every run.
 */
int surfel_jpegdec_decode(const surfel_jpegdec_desc* desc, const uint8_t* file, int64_t file_bytes, uint8_t* out, void* scratch,
                          int64_t scratch_bytes, int subseq_bits, int max_rounds, int stages, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SURFEL_JPEGDEC_H */
