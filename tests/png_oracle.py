"""numpy restatement of the PNG encoder of include/surfel_png.h (PNG.md: rules -> bytes, integers only): adaptive row filters,
distance-1 matches, one dynamic-Huffman block per ~32 KiB stripe with length-limited codes, Adler-32, CRC-32, the chunk structure.
`encode(img)` is the whole file; `analyse(img)` also returns what the tests look at (filters chosen, the stripes' code lengths, whether
the length limit was hit)."""
import struct

import numpy as np

STRIPE_BYTES = 32768                 # SURFEL_PNG_STRIPE_BYTES
MAX_STREAM = 1 << 30                 # SURFEL_PNG_MAX_STREAM
MAX_ROW = 1 << 20                    # SURFEL_PNG_MAX_ROW
STRIPE_EXTRA_BITS = 2140             # SURFEL_PNG_STRIPE_EXTRA_BITS
FRONT = 43                           # signature 8, IHDR 25, IDAT length + type 8, zlib header 2
ZLIB_HEADER = b"\x78\x01"
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def _length_tables():
    sym, eb, ev = np.zeros(259, np.int64), np.zeros(259, np.int64), np.zeros(259, np.int64)
    for ln in range(3, 259):
        k = max(j for j in range(29) if LEN_BASE[j] <= ln)
        if ln == 258:
            k = 28
        sym[ln], eb[ln], ev[ln] = 257 + k, LEN_EXTRA[k], ln - LEN_BASE[k]
    return sym, eb, ev


LEN_SYM, LEN_EB, LEN_EV = _length_tables()


# ------------------------------------------------------------------------------------------------ sizes
def rows_per_stripe(H, W, C):
    return min(H, -(-STRIPE_BYTES // (1 + W * C)))


def stripe_lengths(H, W, C):
    rps, row = rows_per_stripe(H, W, C), 1 + W * C
    return [min(rps, H - r) * row for r in range(0, H, rps)]


def stripe_capacity(L):
    """bytes (a multiple of 4) that hold any stripe of L filtered bytes: 15 bits per byte and STRIPE_EXTRA_BITS for the header
    (17 + 19 * 3 + 287 * 7 = 2083), the end-of-block (15) and the stored block behind it (3 + 7 + 32)"""
    return (15 * L + STRIPE_EXTRA_BITS + 31) // 32 * 4


def capacity(H, W, C):
    return FRONT + sum(stripe_capacity(L) for L in stripe_lengths(H, W, C)) + 4 + 4 + 12


# ------------------------------------------------------------------------------------------------ 1. filters
def filter_rows(img):
    """[H, W, C] u8 -> (the filtered stream [H, 1 + W C] u8, the filter of every row)"""
    H, W, Cn = img.shape
    n = W * Cn
    raw = img.reshape(H, n).astype(np.int64)
    up = np.vstack([np.zeros((1, n), np.int64), raw[:-1]])
    left = np.hstack([np.zeros((H, Cn), np.int64), raw[:, :n - Cn]]) if n > Cn else np.zeros((H, n), np.int64)
    upleft = np.hstack([np.zeros((H, Cn), np.int64), up[:, :n - Cn]]) if n > Cn else np.zeros((H, n), np.int64)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    res = np.stack([raw, raw - left, raw - up, raw - ((left + up) >> 1), raw - paeth]) & 255      # [5, H, n]
    signed = np.where(res >= 128, 256 - res, res)
    cost = signed.sum(axis=2)                                                                       # [5, H]
    best = np.argmin(cost, axis=0)                                                                  # ties: the lowest filter number
    out = np.empty((H, 1 + n), np.uint8)
    out[:, 0] = best
    out[:, 1:] = res[best, np.arange(H)]
    return out, best


def adler32(stream):
    """by rows, as the device accumulates it: A_r = sum d, B_r = sum j d_j (j the byte's place in its row), both mod 65521"""
    H, row = stream.shape
    N = H * row
    d = stream.astype(np.int64)
    A = d.sum(axis=1) % 65521
    B = (d * np.arange(row)).sum(axis=1) % 65521
    s1, s2 = 1, N % 65521
    for r in range(H):
        s1 = (s1 + int(A[r])) % 65521
        s2 = (s2 + ((N - r * row) % 65521) * int(A[r]) + 65521 - int(B[r])) % 65521
    return s2 << 16 | s1


# ------------------------------------------------------------------------------------------------ 3. tokens
def tokens(d):
    """per byte of a stripe: -1 no token, 0 .. 255 a literal, 256 + L a match of length L at distance 1"""
    L = len(d)
    idx = np.arange(L)
    start = np.ones(L, bool)
    start[1:] = d[1:] != d[:-1]
    gs = np.maximum.accumulate(np.where(start, idx, 0))
    nxt = np.where(start, idx, L)
    ge = np.empty(L, np.int64)
    ge[:-1] = np.minimum.accumulate(nxt[::-1])[::-1][1:]
    ge[-1] = L
    k, p = ge - gs, idx - gs
    m, q = k - 1, p - 1
    full, rem = m // 258, m % 258
    tok = np.full(L, -1, np.int64)
    lit = (p == 0) | ((q >= full * 258) & (rem < 3))
    tok[lit] = d[lit]
    m258 = (p > 0) & (q < full * 258) & (q % 258 == 0)
    tok[m258] = 256 + 258
    mrem = (p > 0) & (q == full * 258) & (rem >= 3)
    tok[mrem] = 256 + rem[mrem]
    return tok


def histogram(tok):
    t = tok[tok >= 0]
    sym = np.where(t < 256, t, LEN_SYM[np.maximum(t - 256, 0)])
    h = np.bincount(sym, minlength=286).astype(np.int64)
    h[256] += 1
    return h


# ------------------------------------------------------------------------------------------------ 4. codes
def code_lengths(cnt, limit):
    """(lengths, hit): the used symbols in ascending (count, symbol) order; Huffman by two queues (leaves, merged nodes), a leaf
    first when the weights tie; the depths' histogram folded to `limit` and repaired (the longest code loses a leaf, the deepest
    shorter one is split, until the Kraft sum is 1); lengths handed out longest first along the sorted order."""
    n = len(cnt)
    order = sorted((s for s in range(n) if cnt[s] > 0), key=lambda s: (cnt[s], s))
    m = len(order)
    lengths = np.zeros(n, np.int64)
    if m == 0:
        return lengths, False
    if m == 1:
        lengths[order[0]] = 1
        return lengths, False
    w = [int(cnt[s]) for s in order]
    node_w, leaf_parent, node_parent = [], [0] * m, [0] * (m - 1)
    i = j = 0
    for k in range(m - 1):
        total = 0
        for _ in range(2):
            if i < m and (j >= k or w[i] <= node_w[j]):
                total += w[i]
                leaf_parent[i] = k
                i += 1
            else:
                total += node_w[j]
                node_parent[j] = k
                j += 1
        node_w.append(total)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    bl = [0] * 64
    deepest = 0
    for i in range(m):
        dd = depth[leaf_parent[i]] + 1
        deepest = max(deepest, dd)
        bl[min(dd, limit)] += 1
    hit = deepest > limit
    total = sum(bl[ln] << (limit - ln) for ln in range(1, limit + 1))
    while total != 1 << limit:
        bl[limit] -= 1
        for ln in range(limit - 1, 0, -1):
            if bl[ln]:
                bl[ln] -= 1
                bl[ln + 1] += 2
                break
        total -= 1
    i = 0
    for ln in range(limit, 0, -1):
        for _ in range(bl[ln]):
            lengths[order[i]] = ln
            i += 1
    assert i == m
    return lengths, hit


def canonical_codes(lengths):
    """deflate's canonical codes (RFC 1951 3.2.2), each already bit-reversed over its length for LSB-first packing"""
    maxlen = int(lengths.max())
    bl = np.bincount(lengths, minlength=maxlen + 1)
    bl[0] = 0
    nxt, code = [0] * (maxlen + 2), 0
    for b in range(1, maxlen + 1):
        code = (code + int(bl[b - 1])) << 1
        nxt[b] = code
    out = np.zeros(len(lengths), np.int64)
    for s, ln in enumerate(lengths):
        if ln:
            c = nxt[ln]
            nxt[ln] += 1
            out[s] = int(format(c, "0%db" % ln)[::-1], 2)
    return out


def kraft(lengths, limit):
    return sum(1 << (limit - int(ln)) for ln in lengths if ln)


def rle_lengths(seq):
    """[(symbol, extra bits, extra value)] of the code-length sequence, greedy from the left: a run of >= 3 zeros -> 18 (11 .. 138)
    or 17 (3 .. 10) for min(run, 138) of them; a run of >= 3 copies of the value just before it -> 16 for min(run, 6); else the
    value itself"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        run = 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            c = min(run, 138)
            out.append((18, 7, c - 11) if c >= 11 else (17, 3, c - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and run >= 3:
            c = min(run, 6)
            out.append((16, 2, c - 3))
        else:
            c = 1
            out.append((int(v), 0, 0))
        i += c
    return out


# ------------------------------------------------------------------------------------------------ 5. emit
def _pack(values, nbits):
    """LSB-first packing of values[k] over nbits[k] bits -> (bytes, bit count)"""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    pos = np.cumsum(nbits) - nbits
    total = int(nbits.sum())
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    for b in range(int(nbits.max()) if len(nbits) else 0):
        sel = nbits > b
        bits[pos[sel] + b] = (values[sel] >> b) & 1
    return np.packbits(bits, bitorder="little").tobytes(), total


def stripe_block(d, last):
    """the bytes of one stripe: its dynamic-Huffman block and, unless it is the last, the empty stored block behind it"""
    tok = tokens(d)
    hist = histogram(tok)
    ll_len, ll_hit = code_lengths(hist, 15)
    ll_code = canonical_codes(ll_len)
    matches = bool((tok >= 256).any())
    hlit = max(s for s in range(286) if ll_len[s]) + 1
    seq = [int(x) for x in ll_len[:hlit]] + [1 if matches else 0]
    rle = rle_lengths(seq)
    cl_cnt = np.zeros(19, np.int64)
    for s, _, _ in rle:
        cl_cnt[s] += 1
    cl_len, cl_hit = code_lengths(cl_cnt, 7)
    cl_code = canonical_codes(cl_len)
    hclen = max(k for k in range(19) if cl_len[CL_ORDER[k]]) + 1
    hclen = max(hclen, 4)
    vals, nb = [1 if last else 0, 2, hlit - 257, 0, hclen - 4], [1, 2, 5, 5, 4]
    for k in range(hclen):
        vals.append(int(cl_len[CL_ORDER[k]]))
        nb.append(3)
    for s, eb, ev in rle:
        vals.append(int(cl_code[s]) | ev << int(cl_len[s]))
        nb.append(int(cl_len[s]) + eb)
    header_bits = sum(nb)
    t = tok[tok >= 0]
    lit = t < 256
    ln = np.maximum(t - 256, 0)
    sym = np.where(lit, t, LEN_SYM[ln])
    tv = np.where(lit, ll_code[sym], ll_code[sym] | LEN_EV[ln] << ll_len[sym])
    tn = np.where(lit, ll_len[sym], ll_len[sym] + LEN_EB[ln] + 1)      # (+ 1: the distance code, one 0 bit)
    vals = np.concatenate([np.asarray(vals, np.int64), tv, [ll_code[256]]])
    nb = np.concatenate([np.asarray(nb, np.int64), tn, [ll_len[256]]])
    data, bits = _pack(vals, nb)
    if not last:
        data += b"\0" * ((bits + 3 + 7) // 8 - len(data))      # BFINAL 0, BTYPE 00, zeros up to the byte
        data += b"\x00\x00\xff\xff"
    info = dict(ll_len=ll_len, cl_len=cl_len, ll_hit=ll_hit, cl_hit=cl_hit, matches=matches, header_bits=header_bits, bits=bits,
                tokens=len(t), hist=hist)
    assert len(data) <= stripe_capacity(len(d)) and header_bits <= 2083
    return data, info


# ------------------------------------------------------------------------------------------------ 6. the file
_CRC_TABLE = None


def crc32(data, crc=0):
    global _CRC_TABLE
    if _CRC_TABLE is None:
        _CRC_TABLE = []
        for n in range(256):
            c = n
            for _ in range(8):
                c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
            _CRC_TABLE.append(c)
    c = crc ^ 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def analyse(img):
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (1, 3) and img.shape[0] >= 1 and img.shape[1] >= 1
    H, W, Cn = img.shape
    assert 1 + W * Cn <= MAX_ROW and H * (1 + W * Cn) <= MAX_STREAM
    stream, filters = filter_rows(img)
    flat = stream.reshape(-1)
    lens = stripe_lengths(H, W, Cn)
    deflate, infos, off = b"", [], 0
    for k, L in enumerate(lens):
        data, info = stripe_block(flat[off:off + L], k == len(lens) - 1)
        deflate += data
        infos.append(info)
        off += L
    assert off == len(flat)
    idat = ZLIB_HEADER + deflate + struct.pack(">I", adler32(stream))
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if Cn == 1 else 2, 0, 0, 0)
    out = b"\x89PNG\r\n\x1a\n" + struct.pack(">I", 13) + b"IHDR" + ihdr + struct.pack(">I", crc32(b"IHDR" + ihdr))
    out += struct.pack(">I", len(idat)) + b"IDAT" + idat + struct.pack(">I", crc32(b"IDAT" + idat))
    out += struct.pack(">I", 0) + b"IEND" + struct.pack(">I", crc32(b"IEND"))
    assert len(out) <= capacity(H, W, Cn)
    return dict(file=out, filters=filters, stream=stream, stripes=infos, idat=idat)


def encode(img):
    return analyse(img)["file"]
