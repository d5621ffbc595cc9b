"""numpy restatement of the JPEG encoder of include/surfel_jpeg.h (VIDEO.md: rules -> bytes, operation by operation, fp32 with one
rounding per operation) and a reader of AVI files written against the container's layout (it walks the chunks and takes nothing from
the writer).  The tables come from scripts/gen_jpeg_tables.py, which reads them out of files libjpeg writes."""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import gen_jpeg_tables as GT  # noqa: E402

f32 = np.float32
_T = {}


def tables():
    if not _T:
        spec = GT.huffman_spec()
        _T.update(zz=GT.zigzag(), qbase=GT.quant_base(), BK=GT.dct_factors(), dht=GT.dht_segments(),
                  huff={k: GT.huffman_codes(*v) for k, v in spec.items()})
    return _T


def scaled_tables(quality):
    """[2, 64] in zig-zag order: libjpeg's rule on the Annex K tables"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((tables()["qbase"] * s + 50) // 100, 1, 255)


def header(H, W, quality):
    q = scaled_tables(quality)
    mcus = (W + 15) // 16
    out = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(q[t].astype(np.uint8))
    out += b"\xff\xc0\x00\x11\x08" + struct.pack(">HH", H, W) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    out += tables()["dht"]
    out += b"\xff\xdd\x00\x04" + struct.pack(">H", mcus)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return out


def samples(img):
    """[rows, mcus, 6, 8, 8] fp32 level-shifted samples of the padded image: Y00 Y01 Y10 Y11 Cb Cr per MCU, [y][x]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    rows, mcus = (H + 15) // 16, (W + 15) // 16
    p = np.pad(img, ((0, rows * 16 - H), (0, mcus * 16 - W), (0, 0)), mode="edge").astype(f32)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = ((f32(0.299) * R + f32(0.587) * G) + f32(0.114) * B) - f32(128.0)
    Cb = (f32(-0.168736) * R + f32(-0.331264) * G) + f32(0.5) * B
    Cr = (f32(0.5) * R + f32(-0.418688) * G) + f32(-0.081312) * B
    out = np.empty((rows, mcus, 6, 8, 8), f32)
    Ym = Y.reshape(rows, 2, 8, mcus, 2, 8)          # [row, by, y, mcu, bx, x]
    for by in range(2):
        for bx in range(2):
            out[:, :, by * 2 + bx] = Ym[:, by, :, :, bx, :].transpose(0, 2, 1, 3)
    for k, Cc in enumerate((Cb, Cr)):
        m = ((Cc[0::2, 0::2] + Cc[0::2, 1::2]) + (Cc[1::2, 0::2] + Cc[1::2, 1::2])) * f32(0.25)
        out[:, :, 4 + k] = m.reshape(rows, 8, mcus, 8).transpose(0, 2, 1, 3)
    assert out.dtype == f32
    return out


def coefficients(img, quality=95, exact=False):
    """[rows, mcus, 6, 64] int quantised coefficients in zig-zag order.  exact: the same rules with an fp64 matrix DCT and an fp64 division"""
    t = tables()
    s = samples(img)
    q = scaled_tables(quality)[[0, 0, 0, 0, 1, 1]][:, np.argsort(t["zz"])].reshape(6, 8, 8)      # natural order per block
    if exact:
        A = GT.dct_matrix()
        F = np.einsum("vy,...yx,ux->...vu", A, s.astype(np.float64), A)
        F[..., 0, 0] = s.astype(np.float64).sum((-1, -2)) / 8.0      # (the same number; exact where the samples are integers)
        Q = np.rint(F / q)
    else:
        B, K = t["BK"]
        T = s[..., :, None, 0] * B[:, 0]                      # [.., y, u]
        for x in range(1, 8):
            T = T + s[..., :, None, x] * B[:, x]
        G = B[:, 0, None] * T[..., None, 0, :]                # [.., v, u]
        for y in range(1, 8):
            G = G + B[:, y, None] * T[..., None, y, :]
        F = G * K
        assert F.dtype == f32
        Q = np.rint(F / q.astype(f32))
    Q = np.clip(Q, -1023, 1023).astype(np.int64)
    return Q.reshape(Q.shape[:3] + (64,))[..., t["zz"]]


def _cat(v):
    return int(abs(int(v))).bit_length()


def _mag(v, cat):
    return "" if cat == 0 else format((v if v > 0 else v - 1) & ((1 << cat) - 1), "0%db" % cat)


def _code(table, sym):
    code, length = table
    assert length[sym] > 0, sym
    return format(int(code[sym]), "0%db" % int(length[sym]))


def encode(img, quality=95, stats=None):
    """The JFIF file (bytes).  stats: a dict that receives counters of what the symbol stream contained."""
    t = tables()
    H, W = np.asarray(img).shape[:2]
    Q = coefficients(img, quality)
    rows, mcus = Q.shape[:2]
    st = dict(zrl=0, eob=0, no_eob=0, dc_cat=0, ac_cat=0, stuffed=0, rst=[], blocks=0)
    out = bytearray(header(H, W, quality))
    for r in range(rows):
        pred = [0, 0, 0]
        bits = []
        for m in range(mcus):
            for b in range(6):
                comp = 0 if b < 4 else b - 3
                tb = 0 if b < 4 else 1
                dc, ac = t["huff"][(0, tb)], t["huff"][(1, tb)]
                blk = Q[r, m, b]
                d = int(blk[0]) - pred[comp]
                pred[comp] = int(blk[0])
                c = _cat(d)
                st["dc_cat"] = max(st["dc_cat"], c)
                bits.append(_code(dc, c) + _mag(d, c))
                run = 0
                nz = np.nonzero(blk[1:])[0] + 1
                prev = 0
                for k in nz:
                    run = int(k) - prev - 1
                    prev = int(k)
                    v = int(blk[k])
                    while run > 15:
                        bits.append(_code(ac, 0xF0))
                        st["zrl"] += 1
                        run -= 16
                    c = _cat(v)
                    st["ac_cat"] = max(st["ac_cat"], c)
                    bits.append(_code(ac, run << 4 | c) + _mag(v, c))
                if prev < 63:
                    bits.append(_code(ac, 0))
                    st["eob"] += 1
                else:
                    st["no_eob"] += 1
                st["blocks"] += 1
        s = "".join(bits)
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big")
        st["stuffed"] += raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
        if r < rows - 1:
            out += bytes([0xFF, 0xD0 + r % 8])
            st["rst"].append(r % 8)
    out += b"\xff\xd9"
    if stats is not None:
        stats.update(st)
    return bytes(out)


def capacity(H, W):
    rows, mcus = (H + 15) // 16, (W + 15) // 16
    return 629 + rows * (mcus * 2496 + 4)


# ------------------------------------------------------------------------------------------------ AVI, read back
def _chunks(buf, start, end):
    """[(fourcc, payload offset, size)] of the chunks in buf[start:end] (each padded to an even length)"""
    out, p = [], start
    while p + 8 <= end:
        cc, n = buf[p:p + 4], struct.unpack_from("<I", buf, p + 4)[0]
        assert p + 8 + n <= end, (cc, p, n, end)
        out.append((cc, p + 8, n))
        p += 8 + n + (n & 1)
    assert p == end, (p, end)
    return out


def read_avi(path_or_bytes):
    """dict of what an AVI 1.0 file holds: avih / strh / strf fields, the 00dc payloads in file order, the idx1 entries"""
    buf = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI "
    riff = struct.unpack_from("<I", buf, 4)[0]
    assert riff + 8 == len(buf), (riff, len(buf))
    out = {"frames": [], "frame_offsets": [], "index": [], "lists": []}
    for cc, p, n in _chunks(buf, 12, len(buf)):
        if cc == b"LIST":
            kind = buf[p:p + 4]
            out["lists"].append(kind)
            if kind == b"hdrl":
                for c2, p2, n2 in _chunks(buf, p + 4, p + n):
                    if c2 == b"avih":
                        assert n2 == 56
                        v = struct.unpack_from("<14I", buf, p2)
                        out["avih"] = dict(us_per_frame=v[0], flags=v[3], total_frames=v[4], streams=v[6], width=v[8], height=v[9])
                    elif c2 == b"LIST":
                        assert buf[p2:p2 + 4] == b"strl"
                        for c3, p3, n3 in _chunks(buf, p2 + 4, p2 + n2):
                            if c3 == b"strh":
                                assert n3 == 56
                                v = struct.unpack_from("<4s4sIHHIIIIIIII4H", buf, p3)
                                out["strh"] = dict(type=v[0], handler=v[1], scale=v[6], rate=v[7], length=v[9], frame=v[13:17])
                            elif c3 == b"strf":
                                assert n3 == 40
                                v = struct.unpack_from("<IiiHH4sIiiII", buf, p3)
                                out["strf"] = dict(size=v[0], width=v[1], height=v[2], planes=v[3], bits=v[4], compression=v[5], image_bytes=v[6])
            elif kind == b"movi":
                out["movi"] = p      # offset of the 'movi' fourcc
                for c2, p2, n2 in _chunks(buf, p + 4, p + n):
                    assert c2 == b"00dc", c2
                    out["frames"].append(bytes(buf[p2:p2 + n2]))
                    out["frame_offsets"].append(p2 - 8)
        elif cc == b"idx1":
            assert n % 16 == 0
            out["index"] = [struct.unpack_from("<4sIII", buf, p + 16 * k) for k in range(n // 16)]
    return out
