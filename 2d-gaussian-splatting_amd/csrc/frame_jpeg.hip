// frame_jpeg.hip — the baseline JPEG encoder behind the trajectory videos (include/surfel_jpeg.h, VIDEO.md): one interleaved 8-bit RGB
// frame in, one complete JFIF file out, with no host round trip in between.
// Compiled without contraction (build.py): every fp32 product and sum below rounds on its own, in the order VIDEO.md states, so the
// numpy restatement (tests/video_oracle.py) reproduces the file byte for byte.
//
// Stages (one stream, eight launches):
//   transform   one workgroup per MCU: 16 x 16 pixels staged in LDS, colour conversion, 2 x 2 chroma mean, the two 8-point DCT passes
//               (one wave per 8 x 8 block), quantisation; int16 coefficients in zig-zag order
//   block bits  one wave per block, one coefficient per lane: the Huffman code + magnitude bits of every lane, their total
//   row scan    one workgroup per MCU row: the blocks' bit offsets inside the row (a restart interval), the row's 1-bits of padding
//   emit        one wave per block again: the lanes' bits OR-ed into a wave-private LDS window, the window into the row's zeroed
//               big-endian dwords
//   count       one workgroup per MCU row: the 0xFF bytes of the row
//   finish      one workgroup: the rows' offsets behind the header, the header, EOI and the size word
//   stuff       one workgroup per MCU row: the row's bytes with the stuffed zeros and its RSTm marker, scattered into the file
// Integer OR is the only read-modify-write on memory, so the bytes are the same on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../include/surfel_jpeg.h"
#include "block_ops.h"
#include "carve.h"
#include "jpeg_tables.h"
#include "side_util.h"

namespace surfel {

constexpr int JT = 256;                  // threads per workgroup of every stage but the transform
constexpr int JT_MCU = 384;              // transform: six waves, one per block of the MCU
constexpr int BLOCK_BYTES = 208;         // 64 coefficients x 26 bits (surfel_jpeg.h)
constexpr int MCU_BYTES = 6 * BLOCK_BYTES;

struct JpegQuant {      // the scaled tables in zig-zag order, as the DQT segments carry them
    uint8_t q[2][64];
};
struct JpegHeader {
    uint8_t b[640];
};
static_assert(SURFEL_JPEG_HEADER_BYTES <= sizeof(JpegHeader), "header");
struct RowInfo {        // per MCU row
    uint32_t bits;      // entropy-coded bits before padding
    uint32_t nff;       // 0xFF bytes among the padded bytes
    int64_t off;        // first byte of the row behind the header
};
static_assert(sizeof(RowInfo) == 16, "scratch layout");

// ---- transform -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JT_MCU) jpeg_transform_kernel(int H, int W, int mcus, const uint8_t* __restrict__ rgb, JpegQuant qt,
                                                                int16_t* __restrict__ coef) {
    __shared__ uint8_t s_raw[16][48];
    __shared__ float s_a[64];                 // B[u][x] = cos((2x + 1) u pi / 16)
    __shared__ float s_c[2][16][16];          // Cb, Cr at full resolution
    __shared__ float s_blk[6][64];            // level-shifted samples: Y00 Y01 Y10 Y11 Cb Cr, [y][x]
    __shared__ float s_t[6][64];              // after the row pass, [y][u]
    __shared__ int16_t s_q[6][64];            // quantised, zig-zag order
    const int t = threadIdx.x;
    const int mcu = blockIdx.x, my = mcu / mcus, mx = mcu - my * mcus;
    // 16 rows of 48 bytes; rows and columns behind the image repeat the last one
    for (int i = t; i < 768; i += JT_MCU) {
        const int r = i / 48, c = i - r * 48, px = c / 3, ch = c - px * 3;
        const int sy = min(my * 16 + r, H - 1), sx = min(mx * 16 + px, W - 1);
        s_raw[r][c] = rgb[((int64_t)sy * W + sx) * 3 + ch];
    }
    if (t < 64) s_a[t] = __uint_as_float(JPEG_DCT_COS_BITS[t]);
    __syncthreads();
    if (t < 256) {
        const int r = t >> 4, x = t & 15;
        const float R = (float)s_raw[r][x * 3], G = (float)s_raw[r][x * 3 + 1], B = (float)s_raw[r][x * 3 + 2];
        const float Y = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(0.299f, R), __fmul_rn(0.587f, G)), __fmul_rn(0.114f, B)), 128.0f);
        s_blk[(r >> 3) * 2 + (x >> 3)][(r & 7) * 8 + (x & 7)] = Y;
        s_c[0][r][x] = __fadd_rn(__fadd_rn(__fmul_rn(-0.168736f, R), __fmul_rn(-0.331264f, G)), __fmul_rn(0.5f, B));
        s_c[1][r][x] = __fadd_rn(__fadd_rn(__fmul_rn(0.5f, R), __fmul_rn(-0.418688f, G)), __fmul_rn(-0.081312f, B));
    }
    __syncthreads();
    if (t < 128) {
        const int c = t >> 6, k = t & 63, y = (k >> 3) * 2, x = (k & 7) * 2;
        s_blk[4 + c][k] = __fmul_rn(__fadd_rn(__fadd_rn(s_c[c][y][x], s_c[c][y][x + 1]), __fadd_rn(s_c[c][y + 1][x], s_c[c][y + 1][x + 1])), 0.25f);
    }
    __syncthreads();
    const int b = t >> 6, lane = t & 63, hi = lane >> 3, lo = lane & 7;
    {      // rows: T[y][u] = sum over x of B[u][x] * s[y][x], x ascending (y = hi, u = lo)
        float acc = __fmul_rn(s_a[lo * 8], s_blk[b][hi * 8]);
#pragma unroll
        for (int x = 1; x < 8; x++) acc = __fadd_rn(acc, __fmul_rn(s_a[lo * 8 + x], s_blk[b][hi * 8 + x]));
        s_t[b][lane] = acc;
    }
    __syncthreads();
    {      // columns: G[v][u] = sum over y of B[v][y] * T[y][u], y ascending (v = hi, u = lo); F = G * K[v][u]
        float acc = __fmul_rn(s_a[hi * 8], s_t[b][lo]);
#pragma unroll
        for (int y = 1; y < 8; y++) acc = __fadd_rn(acc, __fmul_rn(s_a[hi * 8 + y], s_t[b][y * 8 + lo]));
        const int z = JPEG_ZZ_OF_NATURAL[lane];
        float q = rintf(__fdiv_rn(__fmul_rn(acc, __uint_as_float(JPEG_DCT_SCALE_BITS[lane])), (float)qt.q[b < 4 ? 0 : 1][z]));      // round half to even
        q = fminf(fmaxf(q, -1023.0f), 1023.0f);
        s_q[b][z] = (int16_t)(int)q;
    }
    __syncthreads();
    coef[((int64_t)mcu * 6 + b) * 64 + lane] = s_q[b][lane];
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int category(int v) {      // number of bits of |v|
    const int a = v < 0 ? -v : v;
    return a ? 32 - __clz(a) : 0;
}

// The bits lane `lane` contributes to block `blk` (right-aligned in `bits`, `len` of them, at most 59), all 64 lanes of the wave together.
// lane 0: the DC difference against the previous block of the same component in this MCU row (0 at the row's start).  A non-zero AC
// lane: one ZRL per 16 zeros of its run, the run / size code, the magnitude bits.  The lane behind the last non-zero coefficient: EOB.
__device__ __forceinline__ void lane_code(const int16_t* __restrict__ coef, int64_t blk, int mcus, int lane, uint64_t* bits, int* len) {
    const int64_t mcu = blk / 6;
    const int b = (int)(blk - mcu * 6), tb = b < 4 ? 0 : 1;
    const bool first = mcu % mcus == 0;
    int v = coef[blk * 64 + lane];
    if (lane == 0) {
        int prev = 0;
        if (b >= 1 && b <= 3) prev = coef[(blk - 1) * 64];
        else if (!first) prev = coef[(blk - (b == 0 ? 3 : 6)) * 64];
        v -= prev;
    }
    const unsigned long long mask = __ballot(v != 0) & ~1ull;      // the non-zero AC coefficients
    const int last = mask ? 63 - __clzll(mask) : 0;
    const int cat = category(v);
    const uint32_t mag = (uint32_t)(v + (v >> 31)) & ((1u << cat) - 1u);
    uint64_t out = 0;
    int n = 0;
    if (lane == 0) {
        out = (uint64_t)JPEG_DC_CODE[tb][cat] << cat | mag;
        n = JPEG_DC_LEN[tb][cat] + cat;
    } else if (v != 0) {
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        const int run = lane - (below ? 63 - __clzll(below) : 0) - 1;
        const int zl = JPEG_AC_LEN[tb][0xF0];
        const uint64_t zc = JPEG_AC_CODE[tb][0xF0];
        for (int k = run >> 4; k > 0; k--) {      // at most 3
            out = out << zl | zc;
            n += zl;
        }
        const int sym = (run & 15) << 4 | cat;
        const int cl = JPEG_AC_LEN[tb][sym];
        out = (out << cl | JPEG_AC_CODE[tb][sym]) << cat | mag;
        n += cl + cat;
    } else if (last < 63 && lane == last + 1) {
        out = JPEG_AC_CODE[tb][0];
        n = JPEG_AC_LEN[tb][0];
    }
    *bits = out;
    *len = n;
}

__global__ void __launch_bounds__(JT) jpeg_block_bits_kernel(int64_t nblocks, int mcus, const int16_t* __restrict__ coef, uint32_t* __restrict__ blockbits) {
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * (JT / 64) + (threadIdx.x >> 6);
    if (blk >= nblocks) return;      // (a whole wave)
    uint64_t bits;
    int len;
    lane_code(coef, blk, mcus, lane, &bits, &len);
    const uint32_t total = wave_incl_sum((uint32_t)len);
    if (lane == 63) blockbits[blk] = total;
}

// blockbits[row's blocks] <- their exclusive scan; the row's total; the 1-bits that pad the row to a byte go into its (zeroed) buffer
__global__ void __launch_bounds__(JT) jpeg_row_scan_kernel(int mcus, uint32_t* __restrict__ blockbits, RowInfo* __restrict__ rows, uint32_t* __restrict__ rowbuf,
                                                           int64_t row_words) {
    __shared__ uint32_t s_w[JT / 64];
    const int n = mcus * 6;
    uint32_t* bb = blockbits + (int64_t)blockIdx.x * n;
    uint32_t carry = 0;
    for (int i0 = 0; i0 < n; i0 += JT) {
        const int i = i0 + threadIdx.x;
        const uint32_t v = i < n ? bb[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_sum<JT>(v, s_w, &total);
        if (i < n) bb[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        rows[blockIdx.x].bits = carry;
        const uint32_t used = carry & 7u;
        if (used) {
            const uint32_t pad = 8u - used, s = carry & 31u;
            atomicOr(&rowbuf[(int64_t)blockIdx.x * row_words + (carry >> 5)], ((1u << pad) - 1u) << (32u - s - pad));
        }
    }
}

__global__ void __launch_bounds__(JT) jpeg_emit_kernel(int64_t nblocks, int mcus, const int16_t* __restrict__ coef, const uint32_t* __restrict__ blockoff,
                                                       uint32_t* __restrict__ rowbuf, int64_t row_words) {
    // a block's bits start at most 31 bits into its first dword and are at most 1664: dwords 0 .. 52 of the window
    __shared__ uint32_t s_win[JT / 64][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t blk = (int64_t)blockIdx.x * (JT / 64) + wv;
    const bool live = blk < nblocks;
    s_win[wv][lane] = 0u;
    __syncthreads();
    uint32_t start = 0;
    if (live) {
        uint64_t bits;
        int len;
        lane_code(coef, blk, mcus, lane, &bits, &len);
        start = blockoff[blk];
        const uint32_t incl = wave_incl_sum((uint32_t)len);      // (all 64 lanes)
        if (len > 0) {
            const uint32_t o = (start & 31u) + incl - (uint32_t)len;
            const uint64_t x = bits << (64 - len);      // left-aligned
            const uint32_t s = o & 31u, w = o >> 5;
            const uint64_t y = x >> s;
            const uint32_t w0 = (uint32_t)(y >> 32), w1 = (uint32_t)y, w2 = s ? (uint32_t)((x << (64u - s)) >> 32) : 0u;
            if (w0) atomicOr(&s_win[wv][w], w0);
            if (w1) atomicOr(&s_win[wv][w + 1], w1);      // (a non-zero w1 / w2 means the bits reach that dword: inside the window)
            if (w2) atomicOr(&s_win[wv][w + 2], w2);
        }
    }
    __syncthreads();
    if (live) {
        const uint32_t word = s_win[wv][lane];
        const int64_t row = blk / ((int64_t)mcus * 6);
        if (word) atomicOr(&rowbuf[row * row_words + (start >> 5) + lane], word);      // (the first and last dword are shared with the neighbours)
    }
}

// ---- byte stuffing and compaction ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t count_ff(uint32_t word, int64_t first_byte, int64_t nbytes) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) c += (first_byte + j < nbytes && ((word >> (24 - 8 * j)) & 255u) == 255u) ? 1u : 0u;
    return c;
}

__global__ void __launch_bounds__(JT) jpeg_count_kernel(RowInfo* __restrict__ rows, const uint32_t* __restrict__ rowbuf, int64_t row_words) {
    __shared__ uint32_t s_w[JT / 64];
    const uint32_t* src = rowbuf + (int64_t)blockIdx.x * row_words;
    const int64_t nbytes = ((int64_t)rows[blockIdx.x].bits + 7) >> 3, nwords = (nbytes + 3) >> 2;
    uint32_t c = 0;
    for (int64_t i = threadIdx.x; i < nwords; i += JT) c += count_ff(src[i], i * 4, nbytes);
    uint32_t total;
    block_excl_sum<JT>(c, s_w, &total);
    if (threadIdx.x == 0) rows[blockIdx.x].nff = total;
}

__global__ void __launch_bounds__(JT) jpeg_finish_kernel(int nrows, RowInfo* __restrict__ rows, JpegHeader hdr, uint8_t* __restrict__ dst, int64_t* __restrict__ size) {
    __shared__ uint32_t s_w[JT / 64];
    int64_t carry = 0;
    for (int r0 = 0; r0 < nrows; r0 += JT) {      // (a row holds at most 4096 * 2496 + 4 bytes and a round 256 rows: 32 bits suffice)
        const int r = r0 + threadIdx.x;
        uint32_t v = 0;
        if (r < nrows) v = ((rows[r].bits + 7u) >> 3) + rows[r].nff + (r < nrows - 1 ? 2u : 0u);
        uint32_t total;
        const uint32_t ex = block_excl_sum<JT>(v, s_w, &total);
        if (r < nrows) rows[r].off = carry + ex;
        carry += total;
    }
    for (int i = threadIdx.x; i < SURFEL_JPEG_HEADER_BYTES; i += JT) dst[i] = hdr.b[i];
    if (threadIdx.x == 0) {
        dst[SURFEL_JPEG_HEADER_BYTES + carry] = 0xFF;      // EOI
        dst[SURFEL_JPEG_HEADER_BYTES + carry + 1] = 0xD9;
        *size = SURFEL_JPEG_HEADER_BYTES + carry + 2;
    }
}

__global__ void __launch_bounds__(JT) jpeg_stuff_kernel(int nrows, const RowInfo* __restrict__ rows, const uint32_t* __restrict__ rowbuf, int64_t row_words,
                                                        uint8_t* __restrict__ data) {
    __shared__ uint32_t s_w[JT / 64];
    const int r = blockIdx.x;
    const uint32_t* src = rowbuf + (int64_t)r * row_words;
    const int64_t nbytes = ((int64_t)rows[r].bits + 7) >> 3, nwords = (nbytes + 3) >> 2;
    uint8_t* out = data + rows[r].off;
    int64_t carry = 0;      // stuffed zeros in front of this round
    for (int64_t i0 = 0; i0 < nwords; i0 += JT) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t word = i < nwords ? src[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_sum<JT>(i < nwords ? count_ff(word, i * 4, nbytes) : 0u, s_w, &total);
        int64_t p = i * 4 + carry + ex;
        if (i < nwords) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (i * 4 + j < nbytes) {
                    const uint8_t byte = (uint8_t)(word >> (24 - 8 * j));
                    out[p++] = byte;
                    if (byte == 0xFF) out[p++] = 0x00;
                }
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0 && r < nrows - 1) {
        out[nbytes + carry] = 0xFF;
        out[nbytes + carry + 1] = (uint8_t)(0xD0 + (r & 7));
    }
}

namespace {

struct JpegGeometry {
    int64_t rows, mcus, nblocks, row_bytes, rowbuf_bytes;
};

inline JpegGeometry jpeg_geometry(int H, int W) {
    JpegGeometry g;
    g.rows = (H + 15) / 16;
    g.mcus = (W + 15) / 16;
    g.nblocks = g.rows * g.mcus * 6;
    g.row_bytes = g.mcus * MCU_BYTES;                 // a multiple of 16
    g.rowbuf_bytes = g.rows * g.row_bytes;
    return g;
}

struct JpegScratch {      // the scratch, described once: base == nullptr measures, the caller's pointer hands out the arrays
    int16_t* coef; uint32_t *rowbuf, *blockbits; RowInfo* rows;
    int64_t total;
    static JpegScratch carve(void* base, const JpegGeometry& g) {
        Carver c(base, 16); JpegScratch p;
        p.coef = c.take<int16_t>((size_t)g.nblocks * 64);
        p.rowbuf = c.take<uint32_t>((size_t)g.rowbuf_bytes / 4);
        p.blockbits = c.take<uint32_t>((size_t)g.nblocks);
        p.rows = c.take<RowInfo>((size_t)g.rows);
        p.total = (int64_t)c.size();
        return p;
    }
};

inline int jpeg_size_check(const char* who, int H, int W) {
    char msg[96];
    if (H <= 0 || W <= 0) {
        snprintf(msg, sizeof msg, "%s: bad arguments (H and W must be positive)", who);
        return api_fail(SURFEL_E_INVALID, msg);
    }
    if (H > SURFEL_JPEG_MAX_EDGE || W > SURFEL_JPEG_MAX_EDGE) {
        snprintf(msg, sizeof msg, "%s: an image edge exceeds 65535", who);
        return api_fail(SURFEL_E_LIMIT, msg);
    }
    return 0;
}

// libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline: clipped to 1 .. 255)
inline void jpeg_scaled_tables(int quality, JpegQuant* qt) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) {
            const int v = (JPEG_QBASE_ZZ[t][k] * s + 50) / 100;
            qt->q[t][k] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

inline int jpeg_header(int H, int W, int mcus, const JpegQuant& qt, JpegHeader* hdr) {
    uint8_t* p = hdr->b;
    auto put = [&p](std::initializer_list<int> bytes) {
        for (int v : bytes) *p++ = (uint8_t)v;
    };
    put({0xFF, 0xD8});                                                                                  // SOI
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});                         // APP0: JFIF 1.01, no units, 1:1
    for (int t = 0; t < 2; t++) {                                                                       // DQT 0, DQT 1
        put({0xFF, 0xDB, 0, 67, t});
        memcpy(p, qt.q[t], 64);
        p += 64;
    }
    put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});   // SOF0
    memcpy(p, JPEG_DHT_SEGMENTS, JPEG_DHT_BYTES);                                                       // DHT DC0 AC0 DC1 AC1
    p += JPEG_DHT_BYTES;
    put({0xFF, 0xDD, 0, 4, mcus >> 8, mcus & 255});                                                     // DRI: one MCU row
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});                                   // SOS
    return (int)(p - hdr->b);
}

}  // namespace
}  // namespace surfel

using namespace surfel;

extern "C" {

int64_t surfel_jpeg_capacity(int H, int W) {
    if (const int rc = jpeg_size_check("jpeg_capacity", H, W)) return rc;
    const JpegGeometry g = jpeg_geometry(H, W);
    return SURFEL_JPEG_HEADER_BYTES + g.rows * (g.mcus * 2 * MCU_BYTES + 4);
}

int64_t surfel_jpeg_scratch_bytes(int H, int W) {
    if (const int rc = jpeg_size_check("jpeg_scratch_bytes", H, W)) return rc;
    return JpegScratch::carve(nullptr, jpeg_geometry(H, W)).total;
}

int surfel_jpeg_encode(int H, int W, const uint8_t* rgb, int quality, uint8_t* dst, int64_t capacity, int64_t* size, void* scratch,
                       int64_t scratch_bytes, void* stream) {
    if (const int rc = jpeg_size_check("jpeg_encode", H, W)) return rc;
    if (quality < 1 || quality > 100) return api_fail(SURFEL_E_INVALID, "jpeg_encode: bad arguments (quality must be in 1 .. 100)");
    if (!rgb || !dst || !size || !scratch || (reinterpret_cast<uintptr_t>(size) & 7) || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return api_fail(SURFEL_E_INVALID, "jpeg_encode: bad arguments (a NULL pointer, or size / scratch not 8-byte aligned)");
    const JpegGeometry g = jpeg_geometry(H, W);
    if (capacity < surfel_jpeg_capacity(H, W)) return api_fail(SURFEL_E_INVALID, "jpeg_encode: capacity is below surfel_jpeg_capacity(H, W)");
    const JpegScratch p = JpegScratch::carve(scratch, g);
    if (scratch_bytes < p.total) return api_fail(SURFEL_E_INVALID, "jpeg_encode: scratch holds fewer than surfel_jpeg_scratch_bytes(H, W)");
    JpegQuant qt;
    JpegHeader hdr = {};
    jpeg_scaled_tables(quality, &qt);
    if (jpeg_header(H, W, (int)g.mcus, qt, &hdr) != SURFEL_JPEG_HEADER_BYTES) return api_fail(SURFEL_E_INVALID, "jpeg_encode: header size");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t row_words = g.row_bytes / 4;
    const unsigned wave_blocks = (unsigned)((g.nblocks + JT / 64 - 1) / (JT / 64));
    const hipError_t e = hipMemsetAsync(p.rowbuf, 0, (size_t)g.rowbuf_bytes, s);
    if (e != hipSuccess) return api_fail(SURFEL_E_HIP, "jpeg_encode: hipMemsetAsync", e);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)(g.rows * g.mcus)), dim3(JT_MCU), 0, s, H, W, (int)g.mcus, rgb, qt, p.coef);
    hipLaunchKernelGGL(jpeg_block_bits_kernel, dim3(wave_blocks), dim3(JT), 0, s, g.nblocks, (int)g.mcus, p.coef, p.blockbits);
    hipLaunchKernelGGL(jpeg_row_scan_kernel, dim3((unsigned)g.rows), dim3(JT), 0, s, (int)g.mcus, p.blockbits, p.rows, p.rowbuf, row_words);
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(wave_blocks), dim3(JT), 0, s, g.nblocks, (int)g.mcus, p.coef, p.blockbits, p.rowbuf, row_words);
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)g.rows), dim3(JT), 0, s, p.rows, p.rowbuf, row_words);
    hipLaunchKernelGGL(jpeg_finish_kernel, dim3(1), dim3(JT), 0, s, (int)g.rows, p.rows, hdr, dst, size);
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)g.rows), dim3(JT), 0, s, (int)g.rows, p.rows, p.rowbuf, row_words, dst + SURFEL_JPEG_HEADER_BYTES);
    return launched("jpeg_encode kernels");
}

}  // extern "C"
