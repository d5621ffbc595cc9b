"""Baseline JPEG decoding on MI355X (JPEGDEC.md): the decoder behind `load_cameras(decode="device")`.

The host walks the file's segments (parse) and uploads the whole file once; everything after that is HIP (surfel_jpegdec_decode of
libsurfel_hip.so, include/surfel_jpegdec.h): unstuffing, a self-synchronising parallel Huffman decode, the DC sums, libjpeg's ISLOW
IDCT, its fancy upsampling and its colour conversion.  The pixels are bit for bit what Pillow (libjpeg-turbo) returns for the same
file.  No entropy decoding happens on the host, and there is no host decoder behind this module: a file outside the decoder's scope,
or one the device reports as not converged or damaged, raises JpegNotDecoded and the caller decides (surfel_scene hands it to Pillow).
"""
import ctypes as C
import re
import threading

import torch

import surfel_native as _n

MAX_EDGE = 32768
MAX_ROUNDS_DEFAULT = 36         # JPEGDEC.md "Rounds": twice the largest count seen at 1024 bits (18), at least 8
STATUS = {0: "ok", 1: "not converged", 2: "damaged"}
STAGE_NAMES = ("clean", "huffman", "write", "dc", "idct", "colour")
ALL_STAGES = (1 << len(STAGE_NAMES)) - 1

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


class JpegNotDecoded(RuntimeError):
    """the file is outside the device decoder's scope, or the device reported it as not converged or damaged; .reason says which"""

    def __init__(self, reason):
        RuntimeError.__init__(self, "JPEG not decoded on the device: %s" % reason)
        self.reason = reason


class Descriptor:
    """What parse() returns: the fields of surfel_jpegdec_desc as Python values, the derived counts, and .c, the ctypes structure."""

    def __init__(self, width, height, ncomp, hs, vs, restart_interval, ecs_offset, ecs_bytes, tq, td, ta, qt, bits, huffval):
        self.width, self.height, self.ncomp, self.hs, self.vs = width, height, ncomp, hs, vs
        self.restart_interval, self.ecs_offset, self.ecs_bytes = restart_interval, ecs_offset, ecs_bytes
        self.tq, self.td, self.ta = tuple(tq), tuple(td), tuple(ta)
        self.qt = qt                    # {id: 64 values, natural order}
        self.bits, self.huffval = bits, huffval      # {table: ...}, table = 0, 1: DC 0, DC 1; 2, 3: AC 0, AC 1
        self.mcux, self.mcuy = -(-width // (8 * hs)), -(-height // (8 * vs))
        self.nmcu = self.mcux * self.mcuy
        self.bpm = hs * vs + (2 if ncomp == 3 else 0)      # blocks per MCU
        self.nblocks = self.nmcu * self.bpm
        self.nintervals = -(-self.nmcu // restart_interval) if restart_interval else 1
        c = self.c = _n.JpegDecDesc()
        c.width, c.height, c.ncomp, c.hs, c.vs, c.restart_interval = width, height, ncomp, hs, vs, restart_interval
        c.ecs_offset, c.ecs_bytes = ecs_offset, ecs_bytes
        for k in range(ncomp):
            c.tq[k], c.td[k], c.ta[k] = tq[k], td[k], ta[k]
        for k, v in qt.items():
            c.qt[k][:] = v
        for k, v in bits.items():
            c.bits[k][:] = v
            c.huffval[k][:len(huffval[k])] = huffval[k]


_END = re.compile(rb"\xff[^\x00\xd0-\xd7]")      # the first marker behind the scan that is not a restart marker


def _huffman_ok(bits, vals):
    """the code lengths fit a prefix code with the all-ones code of the longest length left free, and every length has its values"""
    space = 0
    for k, n in enumerate(bits):
        space += n << (15 - k)
    return 0 < sum(bits) == len(vals) <= 256 and space < (1 << 16)


def parse(data):
    """bytes of a JPEG file -> Descriptor, or None when the device decoder does not take the file (JPEGDEC.md "Scope").  Walks the
    segments by their lengths, so markers inside a segment (an EXIF thumbnail in APP1) are never looked at."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0:2] != b"\xff\xd8":
        return None
    pos = 2
    frame = None
    qt, bits, vals, ri = {}, {}, {}, 0
    while True:
        if pos + 4 > n or data[pos] != 0xFF:
            return None
        while pos < n and data[pos] == 0xFF:      # fill bytes in front of a marker
            pos += 1
        if pos + 2 >= n:
            return None
        m = data[pos]
        pos += 1
        if m in (0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            return None
        L = (data[pos] << 8) | data[pos + 1]
        if L < 2 or pos + L > n:
            return None
        seg = data[pos + 2:pos + L]
        if m in (0xC0, 0xC1):
            if frame is not None or len(seg) < 6:
                return None
            prec, H, W, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8 or nc not in (1, 3) or len(seg) != 6 + 3 * nc or not (0 < H <= MAX_EDGE and 0 < W <= MAX_EDGE):
                return None
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(nc)]
            if [c[0] for c in comps] != [1, 2, 3][:nc] or any(c[3] > 3 for c in comps):
                return None
            if any((c[1], c[2]) != (1, 1) for c in comps[1:]) or (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)):
                return None
            if nc == 1 and (comps[0][1], comps[0][2]) != (1, 1):
                return None
            frame = (H, W, comps)
        elif 0xC2 <= m <= 0xCF and m != 0xC4:      # progressive, lossless, arithmetic (and DAC, JPG)
            return None
        elif m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                size = 64 * (1 + pq)
                if pq > 1 or tq > 3 or k + 1 + size > len(seg):
                    return None
                raw = seg[k + 1:k + 1 + size]
                zz = [(raw[2 * i] << 8) | raw[2 * i + 1] for i in range(64)] if pq else list(raw)
                if min(zz) < 1:
                    return None
                nat = [0] * 64
                for i in range(64):
                    nat[ZIGZAG[i]] = zz[i]
                qt[tq] = nat
                k += 1 + size
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg):
                    return None
                tc, th = seg[k] >> 4, seg[k] & 15
                b = list(seg[k + 1:k + 17])
                v = list(seg[k + 17:k + 17 + sum(b)])
                if tc > 1 or th > 1 or not _huffman_ok(b, v):
                    return None
                bits[2 * tc + th], vals[2 * tc + th] = b, v
                k += 17 + sum(b)
        elif m == 0xDD:
            if len(seg) != 2:
                return None
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE and seg[:5] == b"Adobe":
            return None
        elif m == 0xDA:
            if frame is None:
                return None
            H, W, comps = frame
            nc = len(comps)
            if len(seg) != 4 + 2 * nc or seg[0] != nc or [seg[1 + 2 * k] for k in range(nc)] != [c[0] for c in comps]:
                return None
            if tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
                return None
            td, ta = [seg[2 + 2 * k] >> 4 for k in range(nc)], [seg[2 + 2 * k] & 15 for k in range(nc)]
            if any(t > 1 for t in td + ta) or any(t not in bits for t in td) or any(2 + t not in bits for t in ta):
                return None
            if any(c[3] not in qt for c in comps):
                return None
            ecs = pos + L
            end = _END.search(data, ecs)
            if end is not None and data[end.start() + 1] != 0xD9:      # another scan, DNL, tables between scans, fill bytes
                return None
            if n - ecs >= (1 << 28):
                return None
            return Descriptor(W, H, nc, comps[0][1], comps[0][2], ri, ecs, n - ecs, [c[3] for c in comps], td, ta, qt, bits, vals)
        pos += L


# ------------------------------------------------------------------------------------------------ the device
_info = threading.local()


def decode_info():
    """counters of this thread's last decode_jpeg: {"status", "rounds", "subsequences", "blocks"}"""
    return dict(getattr(_info, "last", {}))


def scratch_bytes(desc, subseq_bits=1024):
    return int(_n.call(None, "surfel_jpegdec_scratch_bytes", C.byref(desc.c), int(subseq_bits)))


def _read(data_or_path):
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        return bytes(data_or_path)
    with open(data_or_path, "rb") as f:
        return f.read()


def upload(data, device="cuda"):
    """the file's bytes as a uint8 device tensor (one copy)"""
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device)


def launch(desc, file, subseq_bits=1024, max_rounds=None, stages=ALL_STAGES, out=None, scratch=None, status=None):
    """surfel_jpegdec_decode on the current stream of file's device: (out u8 [H, W, C], status int32 [4], scratch).  Nothing waits for
    the device.  stages: a mask of STAGE_NAMES bits; a later stage alone continues in the scratch an earlier call left."""
    dev = file.device
    rounds = MAX_ROUNDS_DEFAULT if max_rounds is None else int(max_rounds)
    need = scratch_bytes(desc, subseq_bits)
    if out is None:
        out = torch.empty((desc.height, desc.width, desc.ncomp), dtype=torch.uint8, device=dev)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(4, dtype=torch.int32, device=dev)
    _n.call(dev, "surfel_jpegdec_decode", C.byref(desc.c), file, file.numel(), out, scratch, scratch.numel(), int(subseq_bits), rounds,
            int(stages), status)
    return out, status, scratch


def decode_jpeg(data_or_path, device="cuda", subseq_bits=1024, max_rounds=None, desc=None):
    """A JPEG file (bytes or a path) -> its pixels as a uint8 [H, W, C] tensor on `device`, C = 1 (Pillow mode L) or 3 (RGB).  Raises
    JpegNotDecoded for a file outside the decoder's scope and for one the device reports as not converged within max_rounds or as
    damaged.  Waits for the status word (16 bytes) and for nothing else.  desc: the file's parse() result, when the caller has it."""
    data = _read(data_or_path)
    if desc is None:
        desc = parse(data)
    if desc is None:
        _info.last = {"status": "not supported", "rounds": 0, "subsequences": 0, "blocks": 0}
        raise JpegNotDecoded("not supported")
    out, status, _ = launch(desc, upload(data, device), subseq_bits, max_rounds)
    code, rounds, nsub, nblk = (int(v) for v in status.tolist())
    _info.last = {"status": STATUS.get(code, "damaged"), "rounds": rounds, "subsequences": nsub, "blocks": nblk}
    if code != 0:
        raise JpegNotDecoded(STATUS.get(code, "damaged"))
    return out
