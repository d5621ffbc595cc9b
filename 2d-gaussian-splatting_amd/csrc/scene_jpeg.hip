// scene_jpeg.hip — the baseline JPEG decoder behind capture loading (include/surfel_jpegdec.h, JPEGDEC.md): the uploaded file in, the
// interleaved 8-bit gray or RGB pixels out, with no host round trip in between.  All arithmetic is integer; tests/jpegdec_oracle.py
// restates every rule in numpy and the pixels come out bit for bit (they are libjpeg-turbo's).
//
// Stages (one stream):
//   clean     per byte of the entropy-coded segment: kept, stuffed zero or marker; the shared scan compacts the kept bytes and numbers
//             the restart markers; every restart interval is cut into subsequences of subseq_bits bits; the code tables
//   huffman   max_rounds launches, one lane per subsequence: round 0 decodes every subsequence from (its first bit, slot 0, index 0),
//             round r from the state its predecessor stored in round r - 1; a lane whose input did not change copies its state.  The
//             states are double-buffered, so a round reads only what the previous launch wrote.  A round that changes nothing is the
//             fixed point; the rounds behind it return at once.
//   write     a copy of the blocks every subsequence starts, scanned; one more decode pass writes the coefficients (DC as its difference)
//             and checks that every interval ends behind a whole MCU
//   dc        the DC differences in component order, scanned; a block's DC is its inclusive sum minus the sum at its interval's start
//   idct      jpeg_idct_islow, 8 blocks per wave: lane = (block, column), LDS, lane = (block, row)
//   colour    libjpeg's fancy upsampling and its YCbCr -> RGB conversion, one lane per pixel; the status word
// The only atomic is an integer minimum over byte positions (the end of the data).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "../../include/surfel_jpegdec.h"
#include "block_ops.h"
#include "carve.h"
#include "side_util.h"

namespace surfel {
namespace {

constexpr int JT = 256;                  // threads per workgroup
constexpr int LOOK_BITS = 9;             // first-level lookup: codes of at most 9 bits
// control words (u32)
constexpr int C_END = 0;                 // first byte of the marker that ends the data (the segment's length when there is none)
constexpr int C_CLEAN = 1;               // clean bytes
constexpr int C_RST = 2;                 // restart markers in front of the end
constexpr int C_BAD = 3;                 // their count is not the descriptor's
constexpr int C_NS = 4;                  // subsequences
constexpr int C_ANCHOR = 5;              // an interval does not start at its block, or does not end behind a whole block
constexpr int C_CHANGED = 16;            // [max_rounds]: an unanchored lane decoded in round r
constexpr int CTRL_WORDS = C_CHANGED + SURFEL_JPEGDEC_MAX_ROUNDS;

__device__ const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTables {      // tables 0, 1: DC; 2, 3: AC
    uint16_t look[4][1 << LOOK_BITS];      // length << 8 | symbol of the code that starts these 9 bits; 0: longer than 9 bits
    int32_t maxcode[4][17];                // largest code of a length, -1 when it has none
    int32_t valoff[4][17];                 // index of a length's first value minus its first code
    uint8_t vals[4][256];
    uint8_t zigzag[64];
};
static_assert(sizeof(HuffTables) % 16 == 0, "scratch layout");

struct HuffSpec {
    uint8_t bits[4][16];
    uint8_t huffval[4][256];
};
struct QuantTables {
    uint16_t q[4][64];
};

struct JpegGeom {
    int W, H, ncomp, hs, vs, ny;         // ny = hs * vs luma blocks per MCU
    int ri;                              // MCUs per restart interval (all of them when the file has none)
    int mcux, mcuy, nmcu, bpm, nblocks, nint;
    int sb, max_rounds;
    uint32_t n;                          // bytes of the entropy-coded segment
    uint32_t ns_max;                     // subsequences at most: n * 8 / sb + nint
    uint8_t tq[4], td[4], ta[4];
    int plane_w[3], plane_h[3], dc_base[3];
    int64_t plane_off[3];
};

inline int64_t clean_bytes(const JpegGeom& g) { return (int64_t)align_up((size_t)g.n + 16, 16); }      // zeroed before every decode

struct JpegDecScratch {      // the scratch, described once: base == nullptr measures, the caller's pointer hands out the arrays
    uint32_t* ctrl; HuffTables* tabs; uint32_t *keep, *rst, *scan; uint8_t* clean; uint32_t *istart, *nsub; uint4* subs;
    uint2* state[2]; uint2* lastin; uint32_t *nblk, *first; int16_t* coef; uint32_t* dc; uint8_t* planes;
    int64_t total;
    static JpegDecScratch carve(void* base, const JpegGeom& g) {
        Carver c(base, 16); JpegDecScratch p;
        const size_t n1 = (size_t)g.n + 1, ns = g.ns_max, ns1 = ns + 1, nb1 = (size_t)g.nblocks + 1, e1 = (size_t)g.nint + 1;
        const size_t a = n1 > ns1 ? n1 : ns1, b = nb1 > e1 ? nb1 : e1, longest = a > b ? a : b;      // the scans share one scratch
        p.ctrl = c.take<uint32_t>(CTRL_WORDS);
        p.tabs = c.take<HuffTables>(1);
        p.keep = c.take<uint32_t>(n1);
        p.rst = c.take<uint32_t>(n1);
        p.scan = c.take<uint32_t>((size_t)scan_scratch_u32((int64_t)longest));
        p.clean = c.take<uint8_t>((size_t)clean_bytes(g));
        p.istart = c.take<uint32_t>(e1);
        p.nsub = c.take<uint32_t>(e1);
        p.subs = c.take<uint4>(ns);
        p.state[0] = c.take<uint2>(ns);
        p.state[1] = c.take<uint2>(ns);
        p.lastin = c.take<uint2>(ns);
        p.nblk = c.take<uint32_t>(ns1);
        p.first = c.take<uint32_t>(ns1);
        p.coef = c.take<int16_t>(64 * (size_t)g.nblocks);
        p.dc = c.take<uint32_t>(nb1);
        p.planes = c.take<uint8_t>((size_t)(g.plane_off[g.ncomp - 1] + (int64_t)g.plane_w[g.ncomp - 1] * g.plane_h[g.ncomp - 1]));
        p.total = (int64_t)c.size();
        return p;
    }
};

// ------------------------------------------------------------------------------------------------ 1. the clean stream
__global__ void __launch_bounds__(JT) jpegdec_init_kernel(JpegGeom g, uint32_t* __restrict__ ctrl) {
    for (int k = threadIdx.x; k < CTRL_WORDS; k += JT) ctrl[k] = k == C_END ? g.n : 0u;
}

// what byte i of the segment is: bit 0 kept, bit 1 first byte of a restart marker, bit 2 first byte of any other marker
__device__ __forceinline__ uint32_t byte_class(const uint8_t* __restrict__ b, uint32_t i, uint32_t n) {
    const uint32_t v = b[i], nxt = i + 1 < n ? b[i + 1] : 0u, prv = i > 0 ? b[i - 1] : 0u;
    const bool marker = v == 0xFFu && nxt != 0u;
    const bool rst = marker && nxt >= 0xD0u && nxt <= 0xD7u;
    return (!marker && prv != 0xFFu ? 1u : 0u) | (rst ? 2u : 0u) | (marker && !rst ? 4u : 0u);
}

__global__ void __launch_bounds__(JT) jpegdec_classify_kernel(JpegGeom g, const uint8_t* __restrict__ b, uint32_t* __restrict__ keep,
                                                              uint32_t* __restrict__ rst, uint32_t* __restrict__ ctrl) {
    const uint32_t i = blockIdx.x * JT + threadIdx.x;
    if (i > g.n) return;
    const uint32_t c = i < g.n ? byte_class(b, i, g.n) : 0u;
    keep[i] = c & 1u;
    rst[i] = (c >> 1) & 1u;
    if (c & 4u) atomicMin(&ctrl[C_END], i);
}

// keep, rst: scanned.  The kept bytes in front of the end, packed; istart[j]: the first clean byte of restart interval j
__global__ void __launch_bounds__(JT) jpegdec_compact_kernel(JpegGeom g, const uint8_t* __restrict__ b, const uint32_t* __restrict__ keep,
                                                             const uint32_t* __restrict__ rst, uint8_t* __restrict__ clean,
                                                             uint32_t* __restrict__ istart, uint32_t* __restrict__ ctrl) {
    const uint32_t i = blockIdx.x * JT + threadIdx.x;
    const uint32_t end = min(ctrl[C_END], g.n);
    if (i == 0) {
        ctrl[C_CLEAN] = keep[end];
        ctrl[C_RST] = rst[end];
        ctrl[C_BAD] = rst[end] != (uint32_t)(g.nint - 1);
        istart[0] = 0;
        istart[g.nint] = keep[end];
    }
    if (i >= end) return;
    const uint32_t c = byte_class(b, i, g.n);
    if (c & 1u) clean[keep[i]] = b[i];                                     // (keep[i] < n: one slot per kept byte)
    if ((c & 2u) && rst[i] + 1 < (uint32_t)g.nint) istart[rst[i] + 1] = keep[i];
}

__global__ void __launch_bounds__(JT) jpegdec_nsub_kernel(JpegGeom g, const uint32_t* __restrict__ istart, uint32_t* __restrict__ nsub,
                                                          const uint32_t* __restrict__ ctrl) {
    const int j = blockIdx.x * JT + threadIdx.x;
    if (j > g.nint) return;
    uint32_t count = 0;
    if (j < g.nint && !ctrl[C_BAD]) {      // (the marker count is right: every istart is written, and they ascend)
        const uint32_t bits = 8u * (istart[j + 1] - istart[j]);
        count = max(1u, (bits + (uint32_t)g.sb - 1) / (uint32_t)g.sb);
    }
    nsub[j] = count;
}

// nsub: scanned.  subs[s] = (first bit, end bit, the interval's end bit, interval + 1 for the interval's first subsequence, else 0)
__global__ void __launch_bounds__(JT) jpegdec_subs_kernel(JpegGeom g, const uint32_t* __restrict__ istart, const uint32_t* __restrict__ nsub,
                                                          uint4* __restrict__ subs, uint32_t* __restrict__ ctrl) {
    const uint32_t s = blockIdx.x * JT + threadIdx.x;
    const uint32_t ns = min(nsub[g.nint], g.ns_max);
    if (s == 0) ctrl[C_NS] = ns;
    if (s >= ns) return;
    int lo = 0, hi = g.nint - 1;           // the last interval whose first subsequence is at or before s
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (nsub[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const uint32_t k = s - nsub[lo], first = 8u * istart[lo], last = 8u * istart[lo + 1];
    const uint32_t start = min(first + k * (uint32_t)g.sb, last);
    subs[s] = make_uint4(start, min(start + (uint32_t)g.sb, last), last, k == 0 ? (uint32_t)lo + 1u : 0u);
}

// ------------------------------------------------------------------------------------------------ 2. Huffman
__global__ void __launch_bounds__(64) jpegdec_tables_kernel(HuffSpec spec, HuffTables* __restrict__ T) {
    const int t = threadIdx.x;
    if (t < 64) T->zigzag[t] = ZIGZAG[t];
    if (t >= 4) return;
    for (int e = 0; e < (1 << LOOK_BITS); e++) T->look[t][e] = 0;
    for (int k = 0; k < 256; k++) T->vals[t][k] = spec.huffval[t][k];
    int code = 0, k = 0;
    T->maxcode[t][0] = -1, T->valoff[t][0] = 0;
    for (int l = 1; l <= 16; l++) {
        T->valoff[t][l] = k - code;
        const int count = spec.bits[t][l - 1];
        for (int c = 0; c < count && k < 256; c++, code++, k++)
            if (l <= LOOK_BITS && code < (1 << l))
                for (int e = code << (LOOK_BITS - l); e < (code + 1) << (LOOK_BITS - l); e++) T->look[t][e] = (uint16_t)(l << 8 | spec.huffval[t][k]);
        T->maxcode[t][l] = count ? code - 1 : -1;
        code <<= 1;
    }
}

__device__ __forceinline__ void load_tables(HuffTables* s_T, const HuffTables* __restrict__ T) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(T);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_T);
    for (unsigned k = threadIdx.x; k < sizeof(HuffTables) / 4; k += JT) dst[k] = src[k];
    __syncthreads();
}

// big-endian word k of the clean stream (zero behind its end: the buffer is zeroed and 16 bytes longer)
__device__ __forceinline__ uint32_t be_word(const uint32_t* __restrict__ words, uint32_t k) { return __builtin_bswap32(words[k]); }

// Decodes every symbol that starts in [pos, end) and ends at or before `hard`; returns the blocks started.  WRITE: the coefficients go to
// coef[block][64] (natural order, DC as its difference), `cur` being the block the incoming state continues; blocks outside
// [0, nblocks) are dropped.
template <bool WRITE>
__device__ __forceinline__ uint32_t decode_run(const JpegGeom& g, const HuffTables& T, const uint32_t* __restrict__ words, uint32_t& pos,
                                               uint32_t& slot, uint32_t& zz, uint32_t end, uint32_t hard, int16_t* __restrict__ coef, int cur) {
    uint32_t started = 0;
    if (pos >= end) return 0;
    // the window: words w, w + 1 hold the 32 bits at `pos`; w + 2 is loaded one step ahead, off the symbol-to-symbol chain.  A symbol
    // is at most 31 bits, so the window moves by at most one word per symbol; pos <= hard <= 8 * clean bytes bounds w + 2.
    uint32_t w = pos >> 5;
    uint32_t w0 = be_word(words, w), w1 = be_word(words, w + 1), w2 = be_word(words, w + 2);
    while (pos < end) {
        const uint32_t comp = slot < (uint32_t)g.ny ? 0u : 1u + slot - (uint32_t)g.ny;
        const uint32_t tab = zz == 0 ? g.td[comp] & 1u : 2u + (g.ta[comp] & 1u);
        const uint32_t c32 = (uint32_t)((((uint64_t)w0 << 32 | w1) << (pos & 31u)) >> 32), c16 = c32 >> 16;
        const uint32_t e = T.look[tab][c16 >> (16 - LOOK_BITS)];
        uint32_t len = e >> 8, sym = e & 255u;
        if (e == 0) {
            len = 16, sym = 0;
            for (int l = LOOK_BITS + 1; l <= 16; l++) {
                const int code = (int)(c16 >> (16 - l));
                if (code <= T.maxcode[tab][l]) {
                    len = l, sym = T.vals[tab][(T.valoff[tab][l] + code) & 255];
                    break;
                }
            }
        }
        const uint32_t s = sym & 15u, npos = pos + len + s;
        if (npos > hard) break;
        int v = 0;
        if (s) {
            v = (int)((c32 >> (32 - len - s)) & ((1u << s) - 1u));
            if (v < (1 << (s - 1))) v -= (1 << s) - 1;
        }
        if (zz == 0) {
            started++, cur++;
            if (WRITE && cur >= 0 && cur < g.nblocks) coef[(int64_t)cur * 64] = (int16_t)v;
            zz = 1;
        } else if (s == 0) {
            zz = (sym >> 4) == 15u ? zz + 16 : 64;
        } else {
            zz += sym >> 4;
            if (WRITE && zz < 64 && cur >= 0 && cur < g.nblocks) coef[(int64_t)cur * 64 + T.zigzag[zz]] = (int16_t)v;
            zz++;
        }
        if (zz >= 64) {
            zz = 0;
            slot = slot + 1 < (uint32_t)g.bpm ? slot + 1 : 0;
        }
        pos = npos;
        if ((pos >> 5) != w) {
            w++;
            w0 = w1, w1 = w2, w2 = be_word(words, w + 2);
        }
    }
    return started;
}

// a state: x = bit position, y = slot << 6 | zig-zag index
__global__ void __launch_bounds__(JT) jpegdec_huffman_kernel(JpegGeom g, int round, const uint32_t* __restrict__ words, const uint4* __restrict__ subs,
                                                             const HuffTables* __restrict__ T, const uint2* __restrict__ prev, uint2* __restrict__ cur,
                                                             uint2* __restrict__ lastin, uint32_t* __restrict__ nblk, uint32_t* __restrict__ ctrl) {
    __shared__ HuffTables s_T;
    if (round > 0 && ctrl[C_CHANGED + round - 1] == 0) return;      // the fixed point is behind us: both state buffers hold it
    load_tables(&s_T, T);
    const uint32_t s = blockIdx.x * JT + threadIdx.x;
    if (s >= ctrl[C_NS]) return;
    const uint4 sub = subs[s];
    const bool anchored = sub.w != 0;
    uint2 in = make_uint2(sub.x, 0u);
    if (round > 0) {
        if (!anchored) in = prev[s - 1];                            // (subsequence 0 is anchored)
        const uint2 last = lastin[s];
        if (anchored || (in.x == last.x && in.y == last.y)) {
            cur[s] = prev[s];
            return;
        }
    }
    lastin[s] = in;
    uint32_t pos = in.x, slot = in.y >> 6, zz = in.y & 63u;
    nblk[s] = decode_run<false>(g, s_T, words, pos, slot, zz, sub.y, sub.z, nullptr, 0);
    cur[s] = make_uint2(pos, slot << 6 | zz);
    if (!anchored) ctrl[C_CHANGED + round] = 1u;
}

// ------------------------------------------------------------------------------------------------ 3. write
// nblk: the scanned copy of the counts (nblk[s] = the first block subsequence s starts)
__global__ void __launch_bounds__(JT) jpegdec_write_kernel(JpegGeom g, const uint32_t* __restrict__ words, const uint4* __restrict__ subs,
                                                           const HuffTables* __restrict__ T, const uint2* __restrict__ state,
                                                           const uint32_t* __restrict__ nblk, int16_t* __restrict__ coef, uint32_t* __restrict__ ctrl) {
    __shared__ HuffTables s_T;
    load_tables(&s_T, T);
    const uint32_t s = blockIdx.x * JT + threadIdx.x;
    if (s >= ctrl[C_NS]) return;
    const uint4 sub = subs[s];
    uint2 in = make_uint2(sub.x, 0u);
    if (sub.w != 0) {
        if ((int64_t)nblk[s] != (int64_t)(sub.w - 1) * g.ri * g.bpm) ctrl[C_ANCHOR] = 1u;
    } else {
        in = state[s - 1];
    }
    uint32_t pos = in.x, slot = in.y >> 6, zz = in.y & 63u;
    const int64_t first = (int64_t)nblk[s] - 1;
    decode_run<true>(g, s_T, words, pos, slot, zz, sub.y, sub.z, coef, first > g.nblocks ? g.nblocks : (int)first);
    // the interval's last subsequence leaves between two MCUs, or the stream ends inside a block
    if (sub.y == sub.z && (slot | zz) != 0) ctrl[C_ANCHOR] = 1u;
}

// ------------------------------------------------------------------------------------------------ 4. DC
struct BlockPlace {
    int comp, bx, by;      // component, block column and row in its plane
    int dc, dc_seg;        // index of the block's DC in component order, and of the first one of its restart interval
};

__device__ __forceinline__ BlockPlace place(const JpegGeom& g, int b) {
    BlockPlace p;
    const int mcu = b / g.bpm, slot = b - mcu * g.bpm, mx = mcu % g.mcux, my = mcu / g.mcux, m0 = mcu / g.ri * g.ri;
    if (slot < g.ny) {
        p.comp = 0, p.bx = mx * g.hs + slot % g.hs, p.by = my * g.vs + slot / g.hs;
        p.dc = mcu * g.ny + slot, p.dc_seg = m0 * g.ny;
    } else {
        p.comp = 1 + slot - g.ny, p.bx = mx, p.by = my;
        p.dc = g.dc_base[p.comp] + mcu, p.dc_seg = g.dc_base[p.comp] + m0;
    }
    return p;
}

__global__ void __launch_bounds__(JT) jpegdec_dc_kernel(JpegGeom g, const int16_t* __restrict__ coef, uint32_t* __restrict__ dc) {
    const int b = blockIdx.x * JT + threadIdx.x;
    if (b > g.nblocks) return;
    if (b == g.nblocks) dc[b] = 0;
    else dc[place(g, b).dc] = (uint32_t)(int)coef[(int64_t)b * 64];
}

// ------------------------------------------------------------------------------------------------ 5. dequantisation and IDCT
// one pass of jpeg_idct_islow over d[0 .. 7] (CONST_BITS 13), descaled by `shift`
__device__ __forceinline__ void idct_pass(int (&d)[8], int shift) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
    z2 = d[0], z3 = d[4];
    int tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7], tmp1 = d[5], tmp2 = d[3], tmp3 = d[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const int half = 1 << (shift - 1);
    d[0] = (tmp10 + tmp3 + half) >> shift, d[7] = (tmp10 - tmp3 + half) >> shift;
    d[1] = (tmp11 + tmp2 + half) >> shift, d[6] = (tmp11 - tmp2 + half) >> shift;
    d[2] = (tmp12 + tmp1 + half) >> shift, d[5] = (tmp12 - tmp1 + half) >> shift;
    d[3] = (tmp13 + tmp0 + half) >> shift, d[4] = (tmp13 - tmp0 + half) >> shift;
}

// dc: scanned.  A wave holds 8 blocks: lane = (block, column) for the column pass, (block, row) for the row pass
__global__ void __launch_bounds__(JT) jpegdec_idct_kernel(JpegGeom g, QuantTables qt, const int16_t* __restrict__ coef, const uint32_t* __restrict__ dc,
                                                          uint8_t* __restrict__ planes) {
    __shared__ uint16_t s_q[4][64];
    __shared__ int s_ws[JT / 8][8][9];      // [block][row][column], a row padded to 9 words
    for (int k = threadIdx.x; k < 256; k += JT) s_q[k >> 6][k & 63] = qt.q[k >> 6][k & 63];
    __syncthreads();
    const int blk = threadIdx.x >> 3, col = threadIdx.x & 7;
    const int b = blockIdx.x * (JT / 8) + blk;
    const bool live = b < g.nblocks;
    BlockPlace p = {};
    if (live) p = place(g, b);
    int d[8];
    if (live) {
        const int16_t* src = coef + (int64_t)b * 64 + col;
        const uint16_t* q = s_q[g.tq[p.comp] & 3];
#pragma unroll
        for (int r = 0; r < 8; r++) d[r] = (int)src[8 * r] * (int)q[8 * r + col];
        if (col == 0) d[0] = ((int)(dc[p.dc] - dc[p.dc_seg]) + (int)src[0]) * (int)q[0];
        idct_pass(d, 13 - 2);
#pragma unroll
        for (int r = 0; r < 8; r++) s_ws[blk][r][col] = d[r];
    }
    __syncthreads();
    if (!live) return;
    const int row = col;
#pragma unroll
    for (int c = 0; c < 8; c++) d[c] = s_ws[blk][row][c];
    idct_pass(d, 13 + 2 + 3);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        lo |= (uint32_t)min(max(d[c] + 128, 0), 255) << (8 * c);
        hi |= (uint32_t)min(max(d[c + 4] + 128, 0), 255) << (8 * c);
    }
    uint8_t* dst = planes + g.plane_off[p.comp] + (int64_t)(p.by * 8 + row) * g.plane_w[p.comp] + p.bx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);      // (planes: 16-byte aligned, widths multiples of 8)
}

// ------------------------------------------------------------------------------------------------ 6. upsampling, colour, status
// the chroma sample of pixel (x, y): libjpeg's fancy h2v1 / h2v2 filters on the cw x ch real samples, replication when cw <= 2
__device__ __forceinline__ int chroma_at(const JpegGeom& g, const uint8_t* __restrict__ p, int pw, int cw, int ch, int x, int y) {
    if (g.hs == 1) return p[(int64_t)y * pw + x];
    const int i = x >> 1;
    if (cw <= 2) return p[(int64_t)(y / g.vs) * pw + i];
    if (g.vs == 1) {
        const uint8_t* r = p + (int64_t)y * pw;
        const int v = r[i];
        if (x & 1) return i == cw - 1 ? v : (3 * v + r[i + 1] + 2) >> 2;
        return i == 0 ? v : (3 * v + r[i - 1] + 1) >> 2;
    }
    const int near = y >> 1, far = (y & 1) ? min(near + 1, ch - 1) : max(near - 1, 0);
    const uint8_t* rn = p + (int64_t)near * pw;
    const uint8_t* rf = p + (int64_t)far * pw;
    const int cs = 3 * rn[i] + rf[i];
    if (x & 1) {
        const int k = min(i + 1, cw - 1);
        return (3 * cs + 3 * rn[k] + rf[k] + 7) >> 4;
    }
    const int k = max(i - 1, 0);
    return (3 * cs + 3 * rn[k] + rf[k] + 8) >> 4;
}

__global__ void __launch_bounds__(JT) jpegdec_colour_kernel(JpegGeom g, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * JT + threadIdx.x;
    if (i >= (int64_t)g.W * g.H) return;
    const int y = (int)(i / g.W), x = (int)(i - (int64_t)y * g.W);
    const int lum = planes[g.plane_off[0] + (int64_t)y * g.plane_w[0] + x];
    if (g.ncomp == 1) {
        out[i] = (uint8_t)lum;
        return;
    }
    const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
    const int cb = chroma_at(g, planes + g.plane_off[1], g.plane_w[1], cw, ch, x, y) - 128;
    const int cr = chroma_at(g, planes + g.plane_off[2], g.plane_w[2], cw, ch, x, y) - 128;
    const int r = lum + ((91881 * cr + 32768) >> 16);
    const int gr = lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int bl = lum + ((116130 * cb + 32768) >> 16);
    out[3 * i] = (uint8_t)min(max(r, 0), 255);
    out[3 * i + 1] = (uint8_t)min(max(gr, 0), 255);
    out[3 * i + 2] = (uint8_t)min(max(bl, 0), 255);
}

// nblk: the scanned copy of the counts, its last word the number of blocks all subsequences start
__global__ void jpegdec_status_kernel(JpegGeom g, const uint32_t* __restrict__ ctrl, const uint32_t* __restrict__ nblk, int32_t* __restrict__ status) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int rounds = -1;
    for (int r = 0; r < g.max_rounds && rounds < 0; r++)
        if (ctrl[C_CHANGED + r] == 0) rounds = r;
    const uint32_t total = nblk[g.ns_max];
    int code = SURFEL_JPEGDEC_OK;
    if (ctrl[C_BAD]) code = SURFEL_JPEGDEC_DAMAGED;
    else if (rounds < 0) code = SURFEL_JPEGDEC_NOT_CONVERGED;
    else if (total != (uint32_t)g.nblocks || ctrl[C_ANCHOR] || ctrl[C_END] >= g.n) code = SURFEL_JPEGDEC_DAMAGED;      // (C_END = n: no EOI)
    status[0] = code;
    status[1] = rounds < 0 ? g.max_rounds : rounds;
    status[2] = (int32_t)ctrl[C_NS];
    status[3] = (int32_t)total;
}

// ------------------------------------------------------------------------------------------------ host
inline int geometry(const char* who, const surfel_jpegdec_desc* d, int subseq_bits, int max_rounds, JpegGeom* out) {
    char msg[200];
    if (!d) return api_fail(SURFEL_E_INVALID, "jpegdec: desc is NULL");
    const bool gray = d->ncomp == 1 && d->hs == 1 && d->vs == 1;
    const bool colour = d->ncomp == 3 && ((d->hs == 1 && d->vs == 1) || (d->hs == 2 && (d->vs == 1 || d->vs == 2)));
    bool ok = d->width > 0 && d->height > 0 && (gray || colour) && d->restart_interval >= 0 && d->ecs_offset >= 0 && d->ecs_bytes >= 0;
    for (int c = 0; ok && c < d->ncomp; c++) ok = d->tq[c] < 4 && d->td[c] < 2 && d->ta[c] < 2;
    if (!ok) {
        snprintf(msg, sizeof msg, "%s: bad descriptor (1 component, or 3 with luma sampling 1x1, 2x1 or 2x2; tables 0 .. 3 / 0 .. 1)", who);
        return api_fail(SURFEL_E_INVALID, msg);
    }
    if (subseq_bits < 32 || subseq_bits > 65536 || max_rounds < 1 || max_rounds > SURFEL_JPEGDEC_MAX_ROUNDS) {
        snprintf(msg, sizeof msg, "%s: bad arguments (subseq_bits 32 .. 65536, max_rounds 1 .. %d)", who, SURFEL_JPEGDEC_MAX_ROUNDS);
        return api_fail(SURFEL_E_INVALID, msg);
    }
    if (d->width > SURFEL_JPEGDEC_MAX_EDGE || d->height > SURFEL_JPEGDEC_MAX_EDGE || d->ecs_bytes >= SURFEL_JPEGDEC_MAX_ECS) {
        snprintf(msg, sizeof msg, "%s: the file exceeds the limits (edges <= %d, entropy-coded segment < 2^28 bytes)", who, SURFEL_JPEGDEC_MAX_EDGE);
        return api_fail(SURFEL_E_LIMIT, msg);
    }
    JpegGeom g = {};
    g.W = d->width, g.H = d->height, g.ncomp = d->ncomp, g.hs = d->hs, g.vs = d->vs, g.ny = d->hs * d->vs;
    g.mcux = (g.W + 8 * g.hs - 1) / (8 * g.hs), g.mcuy = (g.H + 8 * g.vs - 1) / (8 * g.vs);
    g.nmcu = g.mcux * g.mcuy;                              // (at most 4096 * 4096)
    g.bpm = g.ny + (g.ncomp == 3 ? 2 : 0);
    g.nblocks = g.nmcu * g.bpm;                            // (at most 2^24 * 3 luma-sized blocks: below 2^26)
    g.ri = d->restart_interval > 0 && d->restart_interval < g.nmcu ? d->restart_interval : g.nmcu;
    g.nint = (g.nmcu + g.ri - 1) / g.ri;
    g.sb = subseq_bits, g.max_rounds = max_rounds;
    g.n = (uint32_t)d->ecs_bytes;
    g.ns_max = (uint32_t)((8 * d->ecs_bytes) / subseq_bits + g.nint);
    int64_t off = 0;
    for (int c = 0; c < g.ncomp; c++) {
        g.tq[c] = d->tq[c], g.td[c] = d->td[c], g.ta[c] = d->ta[c];
        g.plane_w[c] = g.mcux * 8 * (c == 0 ? g.hs : 1), g.plane_h[c] = g.mcuy * 8 * (c == 0 ? g.vs : 1);
        g.plane_off[c] = off;
        off += (int64_t)align_up((size_t)g.plane_w[c] * g.plane_h[c], 16);
        g.dc_base[c] = c == 0 ? 0 : g.nmcu * g.ny + (c - 1) * g.nmcu;
    }
    *out = g;
    return 0;
}

}  // namespace
}  // namespace surfel

using namespace surfel;

extern "C" {

int64_t surfel_jpegdec_scratch_bytes(const surfel_jpegdec_desc* desc, int subseq_bits) {
    JpegGeom g;
    if (const int rc = geometry("jpegdec_scratch_bytes", desc, subseq_bits, 1, &g)) return rc;
    return JpegDecScratch::carve(nullptr, g).total;
}

int surfel_jpegdec_decode(const surfel_jpegdec_desc* desc, const uint8_t* file, int64_t file_bytes, uint8_t* out, void* scratch,
                          int64_t scratch_bytes, int subseq_bits, int max_rounds, int stages, int32_t* status, void* stream) {
    JpegGeom g;
    if (const int rc = geometry("jpegdec_decode", desc, subseq_bits, max_rounds, &g)) return rc;
    if (!file || !out || !scratch || !status || (reinterpret_cast<uintptr_t>(scratch) & 15) || (reinterpret_cast<uintptr_t>(status) & 3))
        return api_fail(SURFEL_E_INVALID, "jpegdec_decode: bad arguments (a NULL pointer, scratch not 16-byte or status not 4-byte aligned)");
    if (desc->ecs_offset + desc->ecs_bytes > file_bytes) return api_fail(SURFEL_E_INVALID, "jpegdec_decode: the entropy-coded segment ends behind the file");
    const JpegDecScratch p = JpegDecScratch::carve(scratch, g);
    if (scratch_bytes < p.total) return api_fail(SURFEL_E_INVALID, "jpegdec_decode: scratch holds fewer than surfel_jpegdec_scratch_bytes(desc, subseq_bits)");
    const uint8_t* ecs = file + desc->ecs_offset;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n1 = (int64_t)g.n + 1, ns1 = (int64_t)g.ns_max + 1;
    const unsigned lanes = blocks_for(g.ns_max, JT);

    if (stages & SURFEL_JPEGDEC_CLEAN) {
        hipError_t e = hipMemsetAsync(p.clean, 0, (size_t)clean_bytes(g), s);
        if (e == hipSuccess) e = hipMemsetAsync(p.istart, 0, (size_t)(4 * (g.nint + 1)), s);
        if (e != hipSuccess) return api_fail(SURFEL_E_HIP, "jpegdec_decode: hipMemsetAsync", e);
        hipLaunchKernelGGL(jpegdec_init_kernel, dim3(1), dim3(JT), 0, s, g, p.ctrl);
        hipLaunchKernelGGL(jpegdec_classify_kernel, dim3(blocks_for(n1, JT)), dim3(JT), 0, s, g, ecs, p.keep, p.rst, p.ctrl);
        scan_u32(p.keep, n1, p.scan, s);
        scan_u32(p.rst, n1, p.scan, s);
        hipLaunchKernelGGL(jpegdec_compact_kernel, dim3(blocks_for(n1, JT)), dim3(JT), 0, s, g, ecs, p.keep, p.rst, p.clean, p.istart, p.ctrl);
        hipLaunchKernelGGL(jpegdec_nsub_kernel, dim3(blocks_for(g.nint + 1, JT)), dim3(JT), 0, s, g, p.istart, p.nsub, p.ctrl);
        scan_u32(p.nsub, g.nint + 1, p.scan, s);
        hipLaunchKernelGGL(jpegdec_subs_kernel, dim3(lanes), dim3(JT), 0, s, g, p.istart, p.nsub, p.subs, p.ctrl);
        HuffSpec spec;
        memcpy(spec.bits, desc->bits, sizeof spec.bits);
        memcpy(spec.huffval, desc->huffval, sizeof spec.huffval);
        hipLaunchKernelGGL(jpegdec_tables_kernel, dim3(1), dim3(64), 0, s, spec, p.tabs);
    }
    if (stages & SURFEL_JPEGDEC_HUFFMAN) {
        hipError_t e = hipMemsetAsync(p.nblk, 0, (size_t)(4 * ns1), s);
        if (e == hipSuccess) e = hipMemsetAsync(p.ctrl + C_CHANGED, 0, 4 * SURFEL_JPEGDEC_MAX_ROUNDS, s);
        if (e != hipSuccess) return api_fail(SURFEL_E_HIP, "jpegdec_decode: hipMemsetAsync", e);
        for (int r = 0; r < max_rounds; r++)
            hipLaunchKernelGGL(jpegdec_huffman_kernel, dim3(lanes), dim3(JT), 0, s, g, r, reinterpret_cast<const uint32_t*>(p.clean), p.subs, p.tabs,
                               p.state[(r + 1) & 1], p.state[r & 1], p.lastin, p.nblk, p.ctrl);
    }
    if (stages & SURFEL_JPEGDEC_WRITE) {
        hipError_t e = hipMemsetAsync(p.coef, 0, (size_t)(128 * (int64_t)g.nblocks), s);
        if (e == hipSuccess) e = hipMemcpyAsync(p.first, p.nblk, (size_t)(4 * ns1), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return api_fail(SURFEL_E_HIP, "jpegdec_decode: hipMemsetAsync / hipMemcpyAsync", e);
        scan_u32(p.first, ns1, p.scan, s);
        hipLaunchKernelGGL(jpegdec_write_kernel, dim3(lanes), dim3(JT), 0, s, g, reinterpret_cast<const uint32_t*>(p.clean), p.subs, p.tabs,
                           p.state[(max_rounds - 1) & 1], p.first, p.coef, p.ctrl);
    }
    if (stages & SURFEL_JPEGDEC_DC) {
        hipLaunchKernelGGL(jpegdec_dc_kernel, dim3(blocks_for(g.nblocks + 1, JT)), dim3(JT), 0, s, g, p.coef, p.dc);
        scan_u32(p.dc, (int64_t)g.nblocks + 1, p.scan, s);
    }
    if (stages & SURFEL_JPEGDEC_IDCT) {
        QuantTables qt;
        memcpy(qt.q, desc->qt, sizeof qt.q);
        hipLaunchKernelGGL(jpegdec_idct_kernel, dim3(blocks_for(g.nblocks, JT / 8)), dim3(JT), 0, s, g, qt, p.coef, p.dc, p.planes);
    }
    if (stages & SURFEL_JPEGDEC_COLOUR) {
        hipLaunchKernelGGL(jpegdec_colour_kernel, dim3(blocks_for((int64_t)g.W * g.H, JT)), dim3(JT), 0, s, g, p.planes, out);
        hipLaunchKernelGGL(jpegdec_status_kernel, dim3(1), dim3(64), 0, s, g, p.ctrl, p.first, status);
    }
    return launched("jpegdec_decode kernels");
}

}  // extern "C"
