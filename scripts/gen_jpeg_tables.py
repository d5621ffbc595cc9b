#!/usr/bin/env python
"""Generates the tables of the JPEG encoder (VIDEO.md) into 2d-gaussian-splatting_amd/csrc/jpeg_tables.h.  Nothing is typed in:

  * the two Annex K quantisation tables (ITU-T T.81, K.1 / K.2) are read from the DQT segments of a file libjpeg writes at quality 50,
    where its scaling rule leaves the base tables as they are;
  * the four typical Huffman tables (K.3 - K.6) are read from the DHT segments of a file libjpeg writes without its optimisation pass;
  * the code / length arrays follow from BITS / HUFFVAL by the procedure of T.81 Annex C (codes of one length are consecutive, the
    first code of the next length is the successor shifted left);
  * the zig-zag order is walked, and the DCT matrix A[u][x] = c(u) / 2 * cos((2x + 1) u pi / 16) is carried as its cosines B[u][x] and
    the scale K[v][u] = c(v) c(u) / 4 of every coefficient, each evaluated in fp64 and rounded to fp32 once; the header carries the
    fp32 bit patterns.

    python scripts/gen_jpeg_tables.py            -> writes the header
    python scripts/gen_jpeg_tables.py --check    -> exit 1 if the committed header differs
"""
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "2d-gaussian-splatting_amd", "csrc", "jpeg_tables.h")


def segments(data):
    """[(marker, payload)] of a JPEG file's segments up to and including SOS (the payload without the two length bytes)"""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        marker = data[p + 1]
        n = int.from_bytes(data[p + 2:p + 4], "big")
        out.append((marker, data[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return out


def _libjpeg_file(**kw):
    from PIL import Image
    rng = np.random.default_rng(0)
    f = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8)).save(f, "JPEG", **kw)
    return f.getvalue()


def zigzag():
    """natural index (v * 8 + u) of the k-th coefficient of the zig-zag sequence, k = 0..63"""
    order = []
    for s in range(15):
        diag = [(v, s - v) for v in range(8) if 0 <= s - v < 8]      # v = row (vertical frequency), u = column
        order += diag if s % 2 else diag[::-1]
    return np.array([v * 8 + u for v, u in order], np.int64)


def quant_base():
    """[2, 64] (luminance, chrominance) in zig-zag order, as the DQT segments carry them"""
    tabs = {}
    for marker, payload in segments(_libjpeg_file(quality=50)):
        if marker == 0xDB:
            p = 0
            while p < len(payload):
                assert payload[p] >> 4 == 0      # 8-bit entries
                tabs[payload[p] & 15] = np.frombuffer(payload[p + 1:p + 65], np.uint8).astype(np.int64)
                p += 65
    assert sorted(tabs) == [0, 1]
    return np.stack([tabs[0], tabs[1]])


def huffman_spec():
    """{(class, id): (bits[16], huffval)}, class 0 = DC, 1 = AC; id 0 = luminance, 1 = chrominance"""
    spec = {}
    for marker, payload in segments(_libjpeg_file(quality=90, optimize=False)):
        if marker == 0xC4:
            p = 0
            while p < len(payload):
                tc, th = payload[p] >> 4, payload[p] & 15
                bits = list(payload[p + 1:p + 17])
                n = sum(bits)
                spec[(tc, th)] = (bits, list(payload[p + 17:p + 17 + n]))
                p += 17 + n
    assert sorted(spec) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    return spec


def huffman_codes(bits, huffval):
    """(code[256], length[256]) indexed by symbol; length 0 = the symbol has no code (T.81 Annex C)"""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[huffval[k]], length[huffval[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


def dct_matrix():
    """[8, 8] fp64: the orthonormal A[u][x] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt(2)"""
    u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    c = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
    return c / 2.0 * np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)


def dct_factors():
    """(B [8, 8], K [8, 8]) fp32: A = diag(c / 2) B with B[u][x] = cos((2x + 1) u pi / 16) (row 0 is exactly 1) and the scale of
    coefficient (v, u), K[v][u] = c(v) c(u) / 4 (K[0][0] is exactly 1 / 8): the DC coefficient of integer samples comes out exact."""
    u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    c = np.where(np.arange(8) == 0, 1.0 / np.sqrt(2.0), 1.0)
    B = np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)
    K = np.outer(c, c) / 4.0
    K[0, 0] = 0.125
    return B.astype(np.float32), K.astype(np.float32)


def dht_segments():
    """the four DHT segments in the file's order: DC0, AC0, DC1, AC1"""
    spec, out = huffman_spec(), b""
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = spec[(tc, th)]
        out += b"\xff\xc4" + (3 + 16 + len(vals)).to_bytes(2, "big") + bytes([tc << 4 | th]) + bytes(bits) + bytes(vals)
    return out


def _rows(values, fmt, per):
    values = [fmt % int(v) for v in values]
    return ["    " + ", ".join(values[i:i + per]) + "," for i in range(0, len(values), per)]


def render_header():
    zz, q, spec = zigzag(), quant_base(), huffman_spec()
    inv = np.argsort(zz)
    dht = dht_segments()
    lines = ["// Generated by scripts/gen_jpeg_tables.py: do not edit.  The tables of the baseline JPEG encoder (VIDEO.md): ITU-T T.81 Annex K",
             "// quantisation and Huffman tables as libjpeg writes them, the code / length arrays derived from BITS / HUFFVAL (Annex C), the",
             "// zig-zag order and the fp32 DCT matrix as bit patterns.  Host arrays are plain constants; the kernels' arrays are __device__.",
             "#pragma once", "#include <stdint.h>", "", "namespace surfel {", "",
             "// K.1 (luminance) and K.2 (chrominance) in zig-zag order, as a DQT segment carries them",
             "static const uint8_t JPEG_QBASE_ZZ[2][64] = {"]
    for t in range(2):
        lines += ["    {"] + ["    " + r for r in _rows(q[t], "%3d", 16)] + ["    },"]
    lines += ["};", "", "// the four DHT segments, markers included, in the file's order: DC0 AC0 DC1 AC1 (BITS and HUFFVAL of K.3 - K.6)",
              "#define JPEG_DHT_BYTES %d" % len(dht), "static const uint8_t JPEG_DHT_SEGMENTS[JPEG_DHT_BYTES] = {"]
    lines += _rows(dht, "0x%02x", 24) + ["};", "", "// position in the zig-zag sequence of the coefficient with natural index v * 8 + u",
                                         "__device__ constexpr uint8_t JPEG_ZZ_OF_NATURAL[64] = {"]
    lines += _rows(inv, "%2d", 16) + ["};", "", "// B[u][x] = cos((2x + 1) u pi / 16), fp32 bit patterns, index u * 8 + x",
                                      "__device__ constexpr uint32_t JPEG_DCT_COS_BITS[64] = {"]
    B, K = dct_factors()
    lines += _rows(B.view(np.uint32).reshape(-1), "0x%08x", 8) + ["};", "", "// K[v][u] = c(v) c(u) / 4, c(0) = 1 / sqrt(2), fp32 bit patterns, index v * 8 + u",
                                                                  "__device__ constexpr uint32_t JPEG_DCT_SCALE_BITS[64] = {"]
    lines += _rows(K.view(np.uint32).reshape(-1), "0x%08x", 8) + ["};", ""]
    for tc, name, count in ((0, "DC", 12), (1, "AC", 256)):
        codes = [huffman_codes(*spec[(tc, th)]) for th in range(2)]
        lines += ["// Huffman code and length of every %s symbol, [table][symbol]; length 0: no such symbol" % name,
                  "__device__ constexpr uint16_t JPEG_%s_CODE[2][%d] = {" % (name, count)]
        for th in range(2):
            assert not codes[th][1][count:].any()
            lines += ["    {"] + ["    " + r for r in _rows(codes[th][0][:count], "0x%04x", 16)] + ["    },"]
        lines += ["};", "__device__ constexpr uint8_t JPEG_%s_LEN[2][%d] = {" % (name, count)]
        for th in range(2):
            lines += ["    {"] + ["    " + r for r in _rows(codes[th][1][:count], "%2d", 32)] + ["    },"]
        lines += ["};", ""]
    lines += ["}  // namespace surfel", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = render_header()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote %s" % HEADER)
