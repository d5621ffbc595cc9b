"""numpy / Python restatement of the training log (include/surfel_log.h, LOG.md), independent of the library and of surfel_log.py:
CRC-32C and the TFRecord framing, the protobuf wire format of the Events, the step records with the running means of train.py:97-98,
and the panels' pixels.  Everything is written the slow, obvious way."""
import struct
from fractions import Fraction

import numpy as np

F32 = np.float32
TAGS = ("train_loss_patches/dist_loss", "train_loss_patches/normal_loss", "train_loss_patches/reg_loss", "train_loss_patches/total_loss",
        "iter_time", "total_points")
RECORD = np.dtype([("iteration", "<i4"), ("points", "<i4"), ("reg_loss", "<f4"), ("total_loss", "<f4"), ("ema_dist", "<f4"),
                   ("ema_normal", "<f4"), ("raw_total", "<f4"), ("seq", "<u4")])


# ------------------------------------------------------------------------------------------------ checksums and framing
def crc32c(data):
    """bit by bit: reflected CRC with the Castagnoli polynomial"""
    c = 0xffffffff
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    return c ^ 0xffffffff


def mask(c):
    return (((c >> 15) | (c << 17)) + 0xa282ead8) % (1 << 32)


def frame(payload):
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", mask(crc32c(head))) + bytes(payload) + struct.pack("<I", mask(crc32c(payload)))


def unframe(data):
    """[payload] of a file's bytes, both checksums asserted"""
    out, p = [], 0
    while p < len(data):
        n, c = struct.unpack_from("<QI", data, p)
        assert c == mask(crc32c(data[p:p + 8])), ("length crc", len(out))
        payload = data[p + 12:p + 12 + n]
        assert len(payload) == n and struct.unpack_from("<I", data, p + 12 + n)[0] == mask(crc32c(payload)), ("payload crc", len(out))
        out.append(payload)
        p += 16 + n
    return out


# ------------------------------------------------------------------------------------------------ protobuf wire format
def varint(v):
    out = b""
    while True:
        b, v = v & 127, v >> 7
        if v:
            out += bytes([b | 128])
        else:
            return out + bytes([b])


def ld(number, data):
    """length-delimited field"""
    return varint(number * 8 + 2) + varint(len(data)) + data


def scalar_value(tag, x):
    return ld(1, tag.encode()) + varint(2 * 8 + 5) + struct.pack("<f", x)


def image_value(tag, h, w, png):
    return ld(1, tag.encode()) + ld(4, varint(1 * 8) + varint(h) + varint(2 * 8) + varint(w) + varint(3 * 8) + varint(3) + ld(4, png))


def event(wall_time, step, values=(), file_version=None):
    out = varint(1 * 8 + 1) + struct.pack("<d", wall_time)
    if step:
        out += varint(2 * 8) + varint(step)
    if file_version is not None:
        out += ld(3, file_version.encode())
    if values:
        out += ld(5, b"".join(ld(1, v) for v in values))
    return out


def step_values(rec, iter_time_ms):
    """the six (tag, fp32 value) of a record"""
    return list(zip(TAGS, (F32(rec["ema_dist"]), F32(rec["ema_normal"]), F32(rec["reg_loss"]), F32(rec["total_loss"]), F32(iter_time_ms),
                           F32(int(rec["points"])))))


def encode_steps(records, iter_time_ms, wall_time):
    out = b""
    for rec in records:
        out += frame(event(wall_time, int(rec["iteration"]), [scalar_value(t, float(v)) for t, v in step_values(rec, iter_time_ms)]))
    return out


# ------------------------------------------------------------------------------------------------ the step records
def fused_ema(ema, v):
    """what a contracted 0.4 * v + 0.6 * ema would give, exactly rounded: (fma(0.4, v, round(0.6 * ema)), fma(0.6, ema, round(0.4 * v))),
    the two ways a compiler may fuse it"""
    v = float(v)
    return float(Fraction(0.4) * Fraction(v) + Fraction(0.6 * ema)), float(Fraction(0.6) * Fraction(ema) + Fraction(0.4 * v))


def records(steps, with_state=False):
    """steps: [(iteration, points, scalars6, lambda_normal, lambda_dist)] -> RECORD array, one per step in order, as the ring's kernel
    forms them (surfel_log.h); Python floats are fp64 and Python never fuses.  with_state: also (ema_dist, ema_normal, count), the
    fp64 running means and the counter the device keeps"""
    out = np.zeros(len(steps), RECORD)
    ema_dist = ema_normal = 0.0
    with np.errstate(all="ignore"):
        for k, (it, points, s, lam_n, lam_d) in enumerate(steps):
            s = np.asarray(s, F32)
            dist_loss = F32(lam_d) * s[3]           # one fp32 rounding, denormals kept
            normal_loss = F32(lam_n) * s[2]
            ema_dist = 0.4 * float(dist_loss) + 0.6 * ema_dist
            ema_normal = 0.4 * float(normal_loss) + 0.6 * ema_normal
            out[k] = (it, points, s[0], s[4], F32(ema_dist), F32(ema_normal), s[5], k & 0xffffffff)
    return (out, (ema_dist, ema_normal, len(steps))) if with_state else out


def ring_steps():
    """the ring tests' 19 scalar sets: random ones, one step with both lambdas 0, one whose lambda_dist * dist is an fp32 denormal, and
    values for which a fused 0.4 * v + 0.6 * ema differs from the unfused one in fp64 (tests/test_log_cpu.py asserts all three)"""
    rng = np.random.default_rng(1)
    steps = []
    for k in range(19):
        s = rng.uniform(1e-3, 1.0, size=6).astype(F32)
        lam_n, lam_d = 0.05, 100.0
        if k == 3:
            lam_n = lam_d = 0.0
        if k == 5:
            s[3], lam_d = F32(1e-10), 1e-30
        steps.append((k + 1, 2000 + 7 * k, s, lam_n, lam_d))
    return steps


# ------------------------------------------------------------------------------------------------ the panels
def _table(name):
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "scripts"))
    import gen_jet_table
    import gen_turbo_table
    return (gen_turbo_table if name == "turbo" else gen_jet_table).parse_header()


def quantize(x):
    """(x * 255).clip(0, 255).astype(uint8) with NaN -> 0, fp32"""
    with np.errstate(all="ignore"):
        y = np.asarray(x, F32) * F32(255)
    y = np.where(np.isnan(y), F32(0), y)
    return np.clip(y, 0, 255).astype(np.uint8)


def bins(t):
    """min(int(t * 256), 255), below the range and NaN: 0"""
    with np.errstate(all="ignore"):
        s = np.asarray(t, F32) * F32(256)
    k = np.zeros(s.shape, np.int64)
    k[s >= 255] = 255
    mid = (s > 0) & (s < 255)
    k[mid] = np.trunc(s[mid]).astype(np.int64)
    return k


def extrema(x):
    """(min, max) over the entries that are not NaN; (NaN, NaN) without any"""
    v = x[~np.isnan(x)]
    return (F32(np.nan), F32(np.nan)) if v.size == 0 else (v.min(), v.max())


def panel(mode, planes):
    """planes fp32 [C, H, W] -> uint8 [H, W, 3] (surfel_log.h)"""
    p = np.asarray(planes, F32)
    C, H, W = p.shape
    with np.errstate(all="ignore"):
        if mode == "rgb":
            return np.moveaxis(quantize(p), 0, 2)
        if mode == "gray":
            return np.repeat(quantize(p[0])[:, :, None], 3, axis=2)
        if mode == "normal":
            return np.moveaxis(quantize(p * F32(0.5) + F32(0.5)), 0, 2)
        lo, hi = extrema(p[0])
        if mode == "turbo_max":
            tab = _table("turbo")
            if not (hi > 0) or np.isinf(hi):
                return np.broadcast_to(tab[0], (H, W, 3)).copy()
            return tab[bins(p[0] / hi)]
        assert mode == "jet_minmax"
        tab = _table("jet")
        if not (hi > lo) or np.isinf(hi) or np.isinf(lo):
            return np.broadcast_to(tab[0], (H, W, 3)).copy()
        return tab[bins((p[0] - lo) / (hi - lo))]
