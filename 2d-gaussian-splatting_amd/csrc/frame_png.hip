// frame_png.hip — the PNG encoder behind the per-frame exports (include/surfel_png.h, PNG.md): one interleaved 8-bit gray or RGB frame
// in, one complete PNG file out, with no host round trip in between.  All arithmetic is integer; tests/png_oracle.py restates every
// rule in numpy and the file comes out byte for byte.
//
// Stages (one stream, a memset and seven launches):
//   filter    one workgroup per scanline: the five filters' sums of |residual|, the winner's bytes into the filtered stream, the
//             row's two Adler-32 partial sums
//   tokens    one workgroup per stripe, a tile of 1024 bytes per round: group starts by a max-scan, group ends by a suffix min-scan
//             (the run behind a tile comes from a backward pass over the tiles' leading runs), one 16-bit token per byte, the
//             literal/length histogram in LDS
//   codes     one wave per stripe: the two length-limited prefix codes, the block header into the stripe's zeroed words
//   emit      one workgroup per stripe: the tokens' bit offsets by a scan, their bits OR-ed into an LDS window, the window into the
//             stripe's zeroed words; end-of-block, the stored block behind it
//   layout    one workgroup: the stripes' offsets, the Adler-32
//   compact   one workgroup per stripe: its bytes behind the front, its CRC-32
//   finish    one workgroup: front, IDAT length, Adler-32, the CRC-32 merged from the stripes', IEND, the size word
// Integer OR is the only read-modify-write on memory, so the bytes are the same on every run.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "../../include/surfel_png.h"
#include "block_ops.h"
#include "carve.h"
#include "side_util.h"

namespace surfel {

constexpr int PF = 256;                  // threads per workgroup: filter, layout, compact, finish
constexpr int PT = 1024;                 // threads per workgroup (= bytes per tile): tokens, emit
constexpr int NSYM = 286;                // literal/length symbols
constexpr int NSYM_PAD = 288;
constexpr uint32_t ADLER = 65521u;
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr int MAX_TILES = (SURFEL_PNG_MAX_ROW + SURFEL_PNG_STRIPE_BYTES) / PT + 1;
constexpr uint32_t NO_TOKEN = 0xFFFFu;
constexpr int WIN_WORDS = (31 + PT * 21 + 31) / 32 + 2;

struct StripeInfo {      // per stripe
    uint32_t header_bits;
    uint32_t bytes;      // the stripe's bytes in the file
    int64_t off;         // its first byte behind the front
    uint32_t crc;        // CRC-32 of those bytes
    uint32_t pad[3];
};
static_assert(sizeof(StripeInfo) == 32, "scratch layout");
struct PngMeta {
    int64_t total;       // deflate bytes
    uint32_t adler;
    uint32_t pad;
};
struct PngFront {
    uint8_t b[48];       // SURFEL_PNG_FRONT_BYTES of them; the IDAT length is patched on the device
};
struct PngShape {
    int H, n, C;         // n = W * C bytes of pixels per row
    int row;             // 1 + n
    int rps;             // rows per stripe
    int stripes;
    int64_t cap_full;    // bytes of the bit buffer of a full stripe
};

// ---- filter --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t filtered(int f, int x, int a, int b, int c) {
    const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint32_t)(x - pred) & 255u;
}

__global__ void __launch_bounds__(PF) png_filter_kernel(PngShape sh, const uint8_t* __restrict__ pix, uint8_t* __restrict__ stream,
                                                        uint32_t* __restrict__ rowsum) {
    __shared__ uint64_t s_w[PF / 64];
    __shared__ int s_best;
    const int r = blockIdx.x, t = threadIdx.x, n = sh.n, C = sh.C;
    const uint8_t* cur = pix + (int64_t)r * n;
    const uint8_t* up = cur - n;      // (read only when r > 0)
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int i = t; i < n; i += PF) {
        const int x = cur[i], a = i >= C ? cur[i - C] : 0, b = r > 0 ? up[i] : 0, c = (r > 0 && i >= C) ? up[i - C] : 0;
#pragma unroll
        for (int f = 0; f < 5; f++) {
            const uint32_t v = filtered(f, x, a, b, c);
            cost[f] += v >= 128u ? 256u - v : v;
        }
    }
    uint64_t sum[5];
#pragma unroll
    for (int f = 0; f < 5; f++) sum[f] = block_sum64<PF>(cost[f], s_w);
    if (t == 0) {
        int best = 0;
#pragma unroll
        for (int f = 1; f < 5; f++)
            if (sum[f] < sum[best]) best = f;      // ties: the lowest filter number
        s_best = best;
    }
    __syncthreads();
    const int best = s_best;
    uint8_t* out = stream + (int64_t)r * sh.row;
    uint64_t A = 0, B = 0;
    if (t == 0) {
        out[0] = (uint8_t)best;
        A = (uint64_t)best;
    }
    for (int i = t; i < n; i += PF) {
        const int x = cur[i], a = i >= C ? cur[i - C] : 0, b = r > 0 ? up[i] : 0, c = (r > 0 && i >= C) ? up[i - C] : 0;
        const uint32_t v = filtered(best, x, a, b, c);
        out[1 + i] = (uint8_t)v;
        A += v;
        B += (uint64_t)(i + 1) * v;
    }
    A = block_sum64<PF>(A, s_w);
    B = block_sum64<PF>(B, s_w);
    if (t == 0) {
        rowsum[2 * r] = (uint32_t)(A % ADLER);
        rowsum[2 * r + 1] = (uint32_t)(B % ADLER);
    }
}

// ---- tokens --------------------------------------------------------------------------------------------------------------------------
// a match length 3 .. 258 -> its symbol, the number of extra bits and their value (RFC 1951 3.2.5)
__device__ __forceinline__ void length_symbol(int len, int* sym, int* eb, int* ev) {
    const int l = len - 3;
    if (len == 258) {
        *sym = 285, *eb = 0, *ev = 0;
    } else if (l < 8) {
        *sym = 257 + l, *eb = 0, *ev = 0;
    } else {
        const int e = 29 - __clz(l);      // floor(log2 l) - 2
        *sym = 261 + 4 * e + ((l >> e) & 3);
        *eb = e;
        *ev = l & ((1 << e) - 1);
    }
}

__global__ void __launch_bounds__(PT) png_token_kernel(PngShape sh, const uint8_t* __restrict__ stream, uint16_t* __restrict__ tok,
                                                       uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_w[PT / 64];
    __shared__ uint32_t s_hist[NSYM_PAD];
    __shared__ uint32_t s_ext[MAX_TILES];      // per tile: the bytes behind it that continue its last byte's run
    __shared__ uint32_t s_carry;
    const int t = threadIdx.x, s = blockIdx.x;
    const int rows = min(sh.rps, sh.H - s * sh.rps);
    const int L = rows * sh.row, tiles = (L + PT - 1) / PT;
    const int64_t base = (int64_t)s * sh.rps * sh.row;
    const uint8_t* d = stream + base;
    for (int i = t; i < NSYM_PAD; i += PT) s_hist[i] = 0u;
    // backward over the tiles: lead = the run that starts at a tile's first byte, through the tiles behind it
    uint32_t lead_next = 0;
    int first_next = -1;
    for (int tl = tiles - 1; tl >= 0; tl--) {
        const int i0 = tl * PT, len = min(PT, L - i0), i = i0 + t;
        const int first = d[i0], last = d[i0 + len - 1];
        const uint32_t lr = block_min<PT>((t < len && d[i] != first) ? (uint32_t)t : (uint32_t)len, s_w);
        const uint32_t ext = first_next == last ? lead_next : 0u;
        if (t == 0) s_ext[tl] = ext;
        lead_next = lr == (uint32_t)len ? (uint32_t)len + ext : lr;
        first_next = first;
    }
    __syncthreads();
    // forward: group start, group end, the token
    uint32_t gs_carry = 0;      // the group start of the byte in front of the tile
    for (int tl = 0; tl < tiles; tl++) {
        const int i0 = tl * PT, len = min(PT, L - i0), i = i0 + t;
        const bool live = t < len;
        const int v = live ? d[i] : 0;
        const bool start = live && (i == 0 || d[i - 1] != v);
        const uint32_t sc = block_scan_max<PT>(start ? (uint32_t)i + 1u : 0u, s_w);
        const uint32_t gs = sc ? sc - 1u : gs_carry;
        const bool next_starts = live && t + 1 < len && d[i + 1] != v;
        const uint32_t sm = block_scan_min_suffix<PT>(next_starts ? (uint32_t)i + 1u : 0xFFFFFFFFu, s_w);
        const uint32_t ge = sm != 0xFFFFFFFFu ? sm : (uint32_t)(i0 + len) + s_ext[tl];
        if (live) {
            const uint32_t p = (uint32_t)i - gs, m = ge - gs - 1u;
            uint32_t token = NO_TOKEN;
            if (p == 0u) {
                token = (uint32_t)v;
            } else {
                const uint32_t q = p - 1u, whole = m / 258u * 258u, rem = m - whole;
                if (q < whole) {
                    if (q % 258u == 0u) token = 256u + 258u;
                } else if (rem < 3u) {
                    token = (uint32_t)v;
                } else if (q == whole) {
                    token = 256u + rem;
                }
            }
            tok[base + i] = (uint16_t)token;
            if (token != NO_TOKEN) {
                int sym = (int)token, eb, ev;
                if (token >= 256u) length_symbol((int)token - 256, &sym, &eb, &ev);
                atomicAdd(&s_hist[sym], 1u);
            }
        }
        if (t == len - 1) s_carry = gs;
        __syncthreads();
        gs_carry = s_carry;
    }
    __syncthreads();
    for (int i = t; i < NSYM_PAD; i += PT) hist[(int64_t)s * NSYM_PAD + i] = s_hist[i] + (i == 256 ? 1u : 0u);      // + the end-of-block
}

// ---- codes ---------------------------------------------------------------------------------------------------------------------------
struct CodeWork {
    uint32_t nodew[NSYM_PAD];
    uint32_t bl[16];
    uint32_t next[16];
    uint16_t order[NSYM_PAD], leafpar[NSYM_PAD], nodepar[NSYM_PAD], depth[NSYM_PAD];
};

// One wave.  len[s] / code[s] (bit-reversed over its length) of the n symbols with counts cnt[]: the used symbols in ascending (count,
// symbol) order, Huffman by two queues with a leaf first on a tie, the depth histogram folded to `limit` and repaired until the Kraft
// sum is 1, lengths handed out longest first along the sorted order, canonical codes (PNG.md section 4).
__device__ void build_code(const uint32_t* cnt, int n, int limit, uint8_t* len, uint16_t* code, CodeWork& w) {
    const int lane = threadIdx.x;
    int m = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        const uint32_t c = s < n ? cnt[s] : 0u;
        if (s < n) {
            len[s] = 0;
            code[s] = 0;
        }
        if (c) {
            int rank = 0;
            for (int j = 0; j < n; j++) {
                const uint32_t cj = cnt[j];
                rank += (cj && (cj < c || (cj == c && j < s))) ? 1 : 0;
            }
            w.order[rank] = (uint16_t)s;
        }
        m += __popcll(__ballot(c != 0u));
    }
    __syncthreads();
    if (lane == 0 && m > 0) {
        for (int b = 0; b < 16; b++) w.bl[b] = 0u;
        if (m == 1) {
            w.bl[1] = 1u;
        } else {
            int i = 0, j = 0;
            for (int k = 0; k < m - 1; k++) {
                uint32_t total = 0;
                for (int r = 0; r < 2; r++) {
                    const uint32_t lw = i < m ? cnt[w.order[i]] : 0u;
                    if (i < m && (j >= k || lw <= w.nodew[j])) {
                        total += lw;
                        w.leafpar[i++] = (uint16_t)k;
                    } else {
                        total += w.nodew[j];
                        w.nodepar[j++] = (uint16_t)k;
                    }
                }
                w.nodew[k] = total;
            }
            w.depth[m - 2] = 0;
            for (int k = m - 3; k >= 0; k--) w.depth[k] = (uint16_t)(w.depth[w.nodepar[k]] + 1);
            for (int q = 0; q < m; q++) w.bl[min((int)w.depth[w.leafpar[q]] + 1, limit)]++;
            uint32_t total = 0;
            for (int b = 1; b <= limit; b++) total += w.bl[b] << (limit - b);
            while (total != 1u << limit) {
                w.bl[limit]--;
                for (int b = limit - 1; b > 0; b--)
                    if (w.bl[b]) {
                        w.bl[b]--;
                        w.bl[b + 1] += 2u;
                        break;
                    }
                total--;
            }
        }
        int i = 0;
        for (int b = limit; b > 0; b--)
            for (uint32_t c = 0; c < w.bl[b]; c++) len[w.order[i++]] = (uint8_t)b;
        uint32_t codev = 0;
        w.next[0] = 0u;
        for (int b = 1; b <= limit; b++) {
            codev = (codev + (b > 1 ? w.bl[b - 1] : 0u)) << 1;
            w.next[b] = codev;
        }
        for (int s = 0; s < n; s++) {
            const int l = len[s];
            if (l) code[s] = (uint16_t)(__brev(w.next[l]++) >> (32 - l));
        }
    }
    __syncthreads();
}

struct BitWriter {      // one lane, into zeroed words, LSB first
    uint32_t* buf;
    uint32_t pos;
    __device__ __forceinline__ void put(uint32_t v, int nb) {
        if (nb == 0) return;
        const uint32_t wd = pos >> 5, sft = pos & 31u;
        atomicOr(&buf[wd], v << sft);
        if (sft + (uint32_t)nb > 32u) atomicOr(&buf[wd + 1], v >> (32u - sft));
        pos += (uint32_t)nb;
    }
};

__constant__ uint8_t PNG_IEND[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
__constant__ uint8_t PNG_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__global__ void __launch_bounds__(64) png_codes_kernel(PngShape sh, const uint32_t* __restrict__ hist, uint32_t* __restrict__ tables,
                                                       StripeInfo* __restrict__ info, uint32_t* __restrict__ bitbuf) {
    __shared__ CodeWork w;
    __shared__ uint32_t s_cnt[NSYM_PAD], s_clcnt[32];
    __shared__ uint8_t s_len[NSYM_PAD], s_cllen[32], s_seq[NSYM_PAD], s_rsym[NSYM_PAD], s_rev[NSYM_PAD];
    __shared__ uint16_t s_code[NSYM_PAD], s_clcode[32];
    __shared__ int s_nrle, s_hlit;
    const int lane = threadIdx.x, s = blockIdx.x;
    for (int i = lane; i < NSYM_PAD; i += 64) s_cnt[i] = hist[(int64_t)s * NSYM_PAD + i];
    if (lane < 32) s_clcnt[lane] = 0u;
    __syncthreads();
    build_code(s_cnt, NSYM, 15, s_len, s_code, w);
    // the code-length sequence: HLIT literal/length lengths, then the one distance code's (1 with matches, 0 without)
    bool has_match = false;
    for (int i = 257 + lane; i < NSYM; i += 64) has_match |= s_cnt[i] != 0u;
    has_match = __ballot(has_match) != 0ull;
    if (lane == 0) {
        int hlit = NSYM;
        while (s_len[hlit - 1] == 0) hlit--;      // (>= 257: the end-of-block is always used)
        s_hlit = hlit;
        const int nseq = hlit + 1;
        for (int i = 0; i < hlit; i++) s_seq[i] = s_len[i];
        s_seq[hlit] = has_match ? 1 : 0;
        int nr = 0;
        for (int i = 0; i < nseq;) {      // greedy from the left (PNG.md section 4)
            const int v = s_seq[i];
            int run = 1;
            while (i + run < nseq && s_seq[i + run] == v) run++;
            int c = 1, sym = v, ev = 0;
            if (v == 0 && run >= 3) {
                c = min(run, 138);
                sym = c >= 11 ? 18 : 17;
                ev = c >= 11 ? c - 11 : c - 3;
            } else if (v != 0 && i > 0 && s_seq[i - 1] == v && run >= 3) {
                c = min(run, 6);
                sym = 16;
                ev = c - 3;
            }
            s_rsym[nr] = (uint8_t)sym;
            s_rev[nr] = (uint8_t)ev;
            s_clcnt[sym]++;
            nr++;
            i += c;
        }
        s_nrle = nr;
    }
    __syncthreads();
    build_code(s_clcnt, 19, 7, s_cllen, s_clcode, w);
    if (lane == 0) {
        const bool last = s == sh.stripes - 1;
        BitWriter bw{bitbuf + (int64_t)s * (sh.cap_full / 4), 0u};
        int hclen = 19;
        while (hclen > 4 && s_cllen[PNG_CL_ORDER[hclen - 1]] == 0) hclen--;
        bw.put(last ? 1u : 0u, 1);
        bw.put(2u, 2);
        bw.put((uint32_t)(s_hlit - 257), 5);
        bw.put(0u, 5);
        bw.put((uint32_t)(hclen - 4), 4);
        for (int k = 0; k < hclen; k++) bw.put(s_cllen[PNG_CL_ORDER[k]], 3);
        const int nr = s_nrle;
        for (int k = 0; k < nr; k++) {
            const int sym = s_rsym[k], cl = s_cllen[sym];
            bw.put(s_clcode[sym], cl);
            bw.put(s_rev[k], sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        info[s].header_bits = bw.pos;
    }
    for (int i = lane; i < NSYM_PAD; i += 64) tables[(int64_t)s * NSYM_PAD + i] = i < NSYM ? ((uint32_t)s_len[i] << 16 | s_code[i]) : 0u;
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PT) png_emit_kernel(PngShape sh, const uint16_t* __restrict__ tok, const uint32_t* __restrict__ tables,
                                                      StripeInfo* __restrict__ info, uint32_t* __restrict__ bitbuf) {
    __shared__ uint32_t s_w[PT / 64];
    __shared__ uint32_t s_tab[NSYM_PAD];
    __shared__ uint32_t s_win[WIN_WORDS];
    const int t = threadIdx.x, s = blockIdx.x;
    const int rows = min(sh.rps, sh.H - s * sh.rps);
    const int L = rows * sh.row, tiles = (L + PT - 1) / PT;
    const int64_t base = (int64_t)s * sh.rps * sh.row;
    uint32_t* out = bitbuf + (int64_t)s * (sh.cap_full / 4);
    for (int i = t; i < NSYM_PAD; i += PT) s_tab[i] = tables[(int64_t)s * NSYM_PAD + i];
    uint32_t bitpos = info[s].header_bits;
    __syncthreads();
    for (int tl = 0; tl < tiles; tl++) {
        const int i = tl * PT + t;
        const uint32_t token = i < L ? tok[base + i] : NO_TOKEN;
        uint32_t val = 0, nb = 0;
        if (token < 256u) {
            const uint32_t e = s_tab[token];
            val = e & 0xFFFFu;
            nb = e >> 16;
        } else if (token != NO_TOKEN) {
            int sym, eb, ev;
            length_symbol((int)token - 256, &sym, &eb, &ev);
            const uint32_t e = s_tab[sym], cl = e >> 16;
            val = (e & 0xFFFFu) | (uint32_t)ev << cl;
            nb = cl + (uint32_t)eb + 1u;      // + the distance code: one 0 bit
        }
        for (int k = t; k < WIN_WORDS; k += PT) s_win[k] = 0u;
        uint32_t total;
        const uint32_t ex = block_excl_sum<PT>(nb, s_w, &total);      // (its barriers order the zeroing before the ORs)
        const uint32_t lead = bitpos & 31u;
        if (nb) {
            const uint32_t o = lead + ex;
            const uint64_t x = (uint64_t)val << (o & 31u);      // at most 31 + 21 bits
            atomicOr(&s_win[o >> 5], (uint32_t)x);
            if (x >> 32) atomicOr(&s_win[(o >> 5) + 1], (uint32_t)(x >> 32));
        }
        __syncthreads();
        const int nw = (int)((lead + total + 31u) >> 5);
        for (int k = t; k < nw; k += PT) {
            const uint32_t word = s_win[k];
            if (word) atomicOr(&out[(bitpos >> 5) + k], word);
        }
        bitpos += total;
        __syncthreads();
    }
    if (t == 0) {
        const bool last = s == sh.stripes - 1;
        const uint32_t e = s_tab[256];
        BitWriter bw{out, bitpos};
        bw.put(e & 0xFFFFu, (int)(e >> 16));
        uint32_t bytes;
        if (last) {
            bytes = (bw.pos + 7u) >> 3;
        } else {      // the empty stored block: BFINAL 0, BTYPE 00, zeros up to the byte, LEN 0000, NLEN FFFF
            bytes = ((bw.pos + 3u + 7u) >> 3) + 4u;
            bw.pos = (bytes - 2u) * 8u;
            bw.put(0xFFFFu, 16);
        }
        info[s].bytes = bytes;
    }
}

// ---- layout, compaction, checksums ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PF) png_layout_kernel(PngShape sh, const uint32_t* __restrict__ rowsum, StripeInfo* __restrict__ info,
                                                        PngMeta* __restrict__ meta) {
    __shared__ uint32_t s_w[PF / 64];
    __shared__ uint64_t s_w64[PF / 64];
    const int t = threadIdx.x;
    int64_t carry = 0;
    for (int s0 = 0; s0 < sh.stripes; s0 += PF) {      // (a stripe holds at most 2 MiB and a round 256 stripes: 32 bits suffice)
        const int s = s0 + t;
        const uint32_t v = s < sh.stripes ? info[s].bytes : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_sum<PF>(v, s_w, &total);
        if (s < sh.stripes) info[s].off = carry + ex;
        carry += total;
    }
    // Adler-32 of the filtered stream from the rows' sums: s1 = 1 + sum A_r, s2 = N + sum ((N - r row) A_r - B_r)   (mod 65521)
    const uint64_t N = (uint64_t)sh.H * sh.row;
    uint64_t s1 = 0, s2 = 0;
    for (int r = t; r < sh.H; r += PF) {
        const uint64_t A = rowsum[2 * r], B = rowsum[2 * r + 1];
        s1 += A;
        s2 += ((N - (uint64_t)r * sh.row) % ADLER) * A + ADLER - B;
    }
    s1 = block_sum64<PF>(s1 % ADLER, s_w64);
    s2 = block_sum64<PF>(s2 % ADLER, s_w64);
    if (t == 0) {
        meta->total = carry;
        meta->adler = (uint32_t)((s2 + N) % ADLER) << 16 | (uint32_t)((s1 + 1u) % ADLER);
    }
}

__device__ __forceinline__ uint32_t crc_table_entry(uint32_t n) {
    uint32_t c = n;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}

// a * b mod P in the reflected representation (bit 31 = x^0)
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 nbytes) mod P
__device__ __forceinline__ uint32_t gf_xpow8(uint64_t nbytes) {
    uint32_t result = 0x80000000u, sq = 0x00800000u;      // 1, x^8
    for (uint64_t n = nbytes; n; n >>= 1) {
        if (n & 1u) result = gf_mul(result, sq);
        sq = gf_mul(sq, sq);
    }
    return result;
}

// crc(A || B) = crc(A) * x^(8 |B|) + crc(B): a part's share of the CRC-32 of a message that goes on for `behind` more bytes
__device__ __forceinline__ uint32_t crc_share(uint32_t crc, uint64_t behind) { return gf_mul(crc, gf_xpow8(behind)); }

__global__ void __launch_bounds__(PF) png_compact_kernel(PngShape sh, StripeInfo* __restrict__ info, const uint32_t* __restrict__ bitbuf,
                                                         uint8_t* __restrict__ data) {
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_w[PF / 64];
    const int t = threadIdx.x, s = blockIdx.x;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(bitbuf + (int64_t)s * (sh.cap_full / 4));
    const uint32_t bytes = info[s].bytes;
    uint8_t* out = data + info[s].off;
    s_tab[t] = crc_table_entry((uint32_t)t);
    __syncthreads();
    for (uint32_t i = t; i < bytes; i += PF) out[i] = src[i];
    const uint32_t per = (bytes + PF - 1) / PF, lo = min((uint32_t)t * per, bytes), hi = min(lo + per, bytes);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = lo; i < hi; i++) c = s_tab[(c ^ src[i]) & 255u] ^ (c >> 8);
    const uint32_t share = hi > lo ? crc_share(~c, bytes - hi) : 0u;
    const uint32_t crc = block_xor<PF>(share, s_w);
    if (t == 0) info[s].crc = crc;
}

__global__ void __launch_bounds__(PF) png_finish_kernel(PngShape sh, const StripeInfo* __restrict__ info, const PngMeta* __restrict__ meta,
                                                        PngFront front, uint32_t head_crc, uint8_t* __restrict__ dst,
                                                        int64_t* __restrict__ size) {
    __shared__ uint32_t s_w[PF / 64];
    const int t = threadIdx.x;
    const int64_t D = meta->total;
    const uint32_t adler = meta->adler;
    // CRC-32 of "IDAT", the zlib header (head_crc: those 6 bytes), the stripes and the Adler-32
    uint32_t share = 0;
    for (int s = t; s < sh.stripes; s += PF) share ^= crc_share(info[s].crc, (uint64_t)(D - info[s].off - info[s].bytes) + 4u);
    if (t == 0) {
        share ^= crc_share(head_crc, (uint64_t)D + 4u);
        uint32_t c = 0xFFFFFFFFu;
        for (int k = 0; k < 4; k++) {
            const uint32_t x = (c ^ (adler >> (24 - 8 * k))) & 255u;
            c = crc_table_entry(x) ^ (c >> 8);
        }
        share ^= ~c;
    }
    const uint32_t crc = block_xor<PF>(share, s_w);
    const uint32_t idat = (uint32_t)(D + 6);      // zlib header, deflate data, Adler-32
    if (t < SURFEL_PNG_FRONT_BYTES) dst[t] = (t >= 33 && t < 37) ? (uint8_t)(idat >> (24 - 8 * (t - 33))) : front.b[t];
    uint8_t* tail = dst + SURFEL_PNG_FRONT_BYTES + D;
    if (t >= 64 && t < 84) {
        const int k = t - 64;      // Adler-32, CRC-32, the IEND chunk
        tail[k] = k < 4 ? (uint8_t)(adler >> (24 - 8 * k)) : k < 8 ? (uint8_t)(crc >> (24 - 8 * (k - 4))) : PNG_IEND[k - 8];
    }
    if (t == 0) *size = SURFEL_PNG_FRONT_BYTES + D + 20;
}

namespace {

inline int64_t stripe_cap(int64_t L) { return (15 * L + SURFEL_PNG_STRIPE_EXTRA_BITS + 31) / 32 * 4; }

struct PngGeometry {
    PngShape sh;
    int64_t N;              // bytes of the filtered stream
    int64_t bit_bytes;      // bytes of all stripes' bit buffers (a multiple of 4)
    int64_t capacity() const { return SURFEL_PNG_FRONT_BYTES + bit_bytes + 20; }
};

inline PngGeometry png_geometry(int H, int W, int C) {
    PngGeometry g;
    PngShape& sh = g.sh;
    sh.H = H, sh.C = C, sh.n = W * C, sh.row = 1 + W * C;
    sh.rps = (SURFEL_PNG_STRIPE_BYTES + sh.row - 1) / sh.row;
    if (sh.rps > H) sh.rps = H;
    sh.stripes = (H + sh.rps - 1) / sh.rps;
    sh.cap_full = stripe_cap((int64_t)sh.rps * sh.row);
    g.N = (int64_t)H * sh.row;
    g.bit_bytes = (sh.stripes - 1) * sh.cap_full + stripe_cap((int64_t)(H - (sh.stripes - 1) * sh.rps) * sh.row);
    return g;
}

struct PngScratch {      // the scratch, described once: base == nullptr measures, the caller's pointer hands out the arrays
    uint8_t* stream; uint16_t* tok; uint32_t *rowsum, *hist, *tables; StripeInfo* info; PngMeta* meta; uint32_t* bitbuf;
    int64_t total;
    static PngScratch carve(void* base, const PngGeometry& g) {
        Carver c(base, 16); PngScratch p;
        const size_t S = (size_t)g.sh.stripes;
        p.stream = c.take<uint8_t>((size_t)g.N);
        p.tok = c.take<uint16_t>((size_t)g.N);
        p.rowsum = c.take<uint32_t>(2 * (size_t)g.sh.H);
        p.hist = c.take<uint32_t>(S * NSYM_PAD);
        p.tables = c.take<uint32_t>(S * NSYM_PAD);
        p.info = c.take<StripeInfo>(S);
        p.meta = c.take<PngMeta>(1);
        p.bitbuf = c.take<uint32_t>((size_t)g.bit_bytes / 4);
        p.total = (int64_t)c.size();
        return p;
    }
};

inline int png_size_check(const char* who, int H, int W, int C) {
    char msg[160];
    if (H <= 0 || W <= 0 || (C != 1 && C != 3)) {
        snprintf(msg, sizeof msg, "%s: bad arguments (H and W must be positive, C 1 or 3)", who);
        return api_fail(SURFEL_E_INVALID, msg);
    }
    const int64_t row = 1 + (int64_t)W * C;
    if (row > SURFEL_PNG_MAX_ROW || (int64_t)H * row > SURFEL_PNG_MAX_STREAM) {
        snprintf(msg, sizeof msg, "%s: the frame exceeds the limits (1 + W * C <= 2^20 bytes per row, H * (1 + W * C) <= 2^30)", who);
        return api_fail(SURFEL_E_LIMIT, msg);
    }
    return 0;
}

inline uint32_t host_crc32(const uint8_t* p, int n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    }
    return ~c;
}

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

}  // namespace
}  // namespace surfel

using namespace surfel;

extern "C" {

int64_t surfel_png_capacity(int H, int W, int C) {
    if (const int rc = png_size_check("png_capacity", H, W, C)) return rc;
    return png_geometry(H, W, C).capacity();
}

int64_t surfel_png_scratch_bytes(int H, int W, int C) {
    if (const int rc = png_size_check("png_scratch_bytes", H, W, C)) return rc;
    return PngScratch::carve(nullptr, png_geometry(H, W, C)).total;
}

int surfel_png_encode(int H, int W, int C, const uint8_t* pix, uint8_t* dst, int64_t capacity, int64_t* size, void* scratch,
                      int64_t scratch_bytes, void* stream) {
    if (const int rc = png_size_check("png_encode", H, W, C)) return rc;
    if (!pix || !dst || !size || !scratch || (reinterpret_cast<uintptr_t>(size) & 7) || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return api_fail(SURFEL_E_INVALID, "png_encode: bad arguments (a NULL pointer, or size / scratch not 8-byte aligned)");
    const PngGeometry g = png_geometry(H, W, C);
    if (capacity < g.capacity()) return api_fail(SURFEL_E_INVALID, "png_encode: capacity is below surfel_png_capacity(H, W, C)");
    const PngScratch p = PngScratch::carve(scratch, g);
    if (scratch_bytes < p.total) return api_fail(SURFEL_E_INVALID, "png_encode: scratch holds fewer than surfel_png_scratch_bytes(H, W, C)");
    PngFront front = {};
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    memcpy(front.b, sig, 8);
    put_be32(front.b + 8, 13);
    memcpy(front.b + 12, "IHDR", 4);
    put_be32(front.b + 16, (uint32_t)W);
    put_be32(front.b + 20, (uint32_t)H);
    front.b[24] = 8, front.b[25] = C == 1 ? 0 : 2;      // bit depth, colour type; compression, filter and interlace method 0
    put_be32(front.b + 29, host_crc32(front.b + 12, 17));
    memcpy(front.b + 37, "IDAT", 4);
    front.b[41] = 0x78, front.b[42] = 0x01;             // zlib: deflate, 32 KiB window, no preset dictionary, fastest level
    const uint32_t head_crc = host_crc32(front.b + 37, 6);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned S = (unsigned)g.sh.stripes;
    const hipError_t e = hipMemsetAsync(p.bitbuf, 0, (size_t)g.bit_bytes, s);
    if (e != hipSuccess) return api_fail(SURFEL_E_HIP, "png_encode: hipMemsetAsync", e);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)H), dim3(PF), 0, s, g.sh, pix, p.stream, p.rowsum);
    hipLaunchKernelGGL(png_token_kernel, dim3(S), dim3(PT), 0, s, g.sh, p.stream, p.tok, p.hist);
    hipLaunchKernelGGL(png_codes_kernel, dim3(S), dim3(64), 0, s, g.sh, p.hist, p.tables, p.info, p.bitbuf);
    hipLaunchKernelGGL(png_emit_kernel, dim3(S), dim3(PT), 0, s, g.sh, p.tok, p.tables, p.info, p.bitbuf);
    hipLaunchKernelGGL(png_layout_kernel, dim3(1), dim3(PF), 0, s, g.sh, p.rowsum, p.info, p.meta);
    hipLaunchKernelGGL(png_compact_kernel, dim3(S), dim3(PF), 0, s, g.sh, p.info, p.bitbuf, dst + SURFEL_PNG_FRONT_BYTES);
    hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(PF), 0, s, g.sh, p.info, p.meta, front, head_crc, dst, size);
    return launched("png_encode kernels");
}

}  // extern "C"
