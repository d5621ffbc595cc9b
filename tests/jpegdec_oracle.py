"""numpy restatement of the device JPEG decoder (JPEGDEC.md, csrc/scene_jpeg.hip), stage by stage: the cleaned stream, the
self-synchronising Huffman decode round by round, the block counts and the coefficient write, the DC sums, libjpeg's ISLOW IDCT,
its fancy upsampling and its colour conversion.  decode() returns the pixels and the counters the device reports in its status
word.  Checked against Pillow in tests/test_jpegdec_cpu.py; the device is checked against this in tests/test_gpu_jpegdec.py."""
import numpy as np

import surfel_jpegdec as JD

OK, NOT_CONVERGED, DAMAGED = 0, 1, 2


# ------------------------------------------------------------------------------------------------ 1. the clean stream
def clean_stream(desc, data):
    """(clean bytes, first clean byte of every restart interval [E + 1] or None when the marker count is wrong, whether a marker ends
    the data)"""
    b = np.frombuffer(data, np.uint8)[desc.ecs_offset:desc.ecs_offset + desc.ecs_bytes].astype(np.int64)
    n = len(b)
    nxt = np.append(b[1:], 0)
    prv = np.insert(b[:-1], 0, 0)
    marker = (b == 0xFF) & (nxt != 0)
    rst = marker & (nxt >= 0xD0) & (nxt <= 0xD7)
    ends = np.flatnonzero(marker & ~rst)
    endpos = int(ends[0]) if len(ends) else n
    keep = ~marker & (prv != 0xFF)          # not a marker's first byte; not a stuffed zero or a marker's second byte
    before = np.concatenate([[0], np.cumsum(keep)])
    clean = b[:endpos][keep[:endpos]].astype(np.uint8).tobytes()
    at = np.flatnonzero(rst[:endpos])
    if len(at) != desc.nintervals - 1:
        return clean, None, endpos < n
    return clean, [0] + [int(before[i]) for i in at] + [len(clean)], endpos < n


# ------------------------------------------------------------------------------------------------ 2. Huffman
def tables(desc):
    """per table (0, 1: DC; 2, 3: AC): (look [512]: length << 8 | symbol for codes of at most 9 bits, else 0; maxcode [17]; valoff [17]:
    index of a length's first value minus its first code; values [256])"""
    out = {}
    for t, bits in desc.bits.items():
        vals = list(desc.huffval[t]) + [0] * (256 - len(desc.huffval[t]))
        look, maxcode, valoff = [0] * 512, [-1] * 17, [0] * 17
        code = k = 0
        for l in range(1, 17):
            valoff[l] = k - code
            for _ in range(bits[l - 1]):
                if l <= 9:
                    for e in range(code << (9 - l), (code + 1) << (9 - l)):
                        look[e] = (l << 8) | vals[k]
                code += 1
                k += 1
            if bits[l - 1]:
                maxcode[l] = code - 1
            code <<= 1
        out[t] = (look, maxcode, valoff, vals)
    return out


class Lanes:
    """the decode loop one lane runs over one subsequence, shared by the synchronisation rounds and the write pass"""

    def __init__(self, desc, clean):
        self.tabs = tables(desc)
        self.clean, self.padded = clean, clean + bytes(8)
        self.bpm = desc.bpm
        ny = desc.hs * desc.vs
        comp = [0] * ny + ([1, 2] if desc.ncomp == 3 else [])
        self.dc_tab = [self.tabs[desc.td[c]] for c in comp]
        self.ac_tab = [self.tabs[2 + desc.ta[c]] for c in comp]

    def run(self, pos, slot, zz, end, hard, coef=None, cur=-1):
        """decodes every symbol that starts in [pos, end) and ends at or before `hard`; -> (pos, slot, zz, blocks started).  coef: the
        [nblocks, 64] array to write into, `cur` being the index of the block the in-state continues"""
        padded, limit, bpm, zigzag = self.padded, len(self.clean), self.bpm, JD.ZIGZAG
        started = 0
        nblocks = 0 if coef is None else coef.shape[0]
        while pos < end:
            look, maxcode, valoff, vals = (self.dc_tab if zz == 0 else self.ac_tab)[slot]
            p = pos >> 3
            w = int.from_bytes(padded[p:p + 5], "big") if p < limit else 0
            c32 = (w >> (8 - (pos & 7))) & 0xFFFFFFFF
            c16 = c32 >> 16
            e = look[c16 >> 7]
            if e:
                ln, sym = e >> 8, e & 255
            else:
                ln, sym = 16, 0
                for l in range(10, 17):
                    code = c16 >> (16 - l)
                    if code <= maxcode[l]:
                        ln, sym = l, vals[(valoff[l] + code) & 255]
                        break
            s = sym & 15
            npos = pos + ln + s
            if npos > hard:
                break
            v = 0
            if s:
                v = (c32 >> (32 - ln - s)) & ((1 << s) - 1)
                if v < (1 << (s - 1)):
                    v -= (1 << s) - 1
            if zz == 0:
                started += 1
                cur += 1
                if coef is not None and 0 <= cur < nblocks:
                    coef[cur, 0] = v
                zz = 1
            elif s == 0:
                zz = zz + 16 if (sym >> 4) == 15 else 64
            else:
                zz += sym >> 4
                if coef is not None and zz < 64 and 0 <= cur < nblocks:
                    coef[cur, zigzag[zz]] = v
                zz += 1
            if zz >= 64:
                zz = 0
                slot = slot + 1 if slot + 1 < bpm else 0
            pos = npos
        return pos, slot, zz, started


def subsequences(istart, subseq_bits):
    """[(first bit, end bit, the interval's end bit, anchored)]: every restart interval is cut into pieces of subseq_bits bits"""
    subs = []
    for j in range(len(istart) - 1):
        s, e = 8 * istart[j], 8 * istart[j + 1]
        count = max(1, -(-(e - s) // subseq_bits))
        for k in range(count):
            subs.append((s + k * subseq_bits, min(s + (k + 1) * subseq_bits, e), e, k == 0))
    return subs


def synchronise(lanes, subs, max_rounds):
    """-> (out-state of every subsequence, blocks it starts, rounds used or None).  Round r reads the states round r - 1 stored."""
    n = len(subs)
    prev = [None] * n
    last_in = [None] * n
    nblk = [0] * n
    rounds = None
    for r in range(max_rounds):
        cur = list(prev)
        changed = False
        for i, (s, e, hard, anchored) in enumerate(subs):
            if r == 0:
                state = (s, 0, 0)
            elif anchored:
                continue
            else:
                state = prev[i - 1][:3]
                if state == last_in[i]:
                    continue
            if not anchored:
                changed = True
            last_in[i] = state
            res = lanes.run(state[0], state[1], state[2], e, hard)
            cur[i], nblk[i] = res[:3], res[3]
        prev = cur
        if not changed:
            rounds = r
            break
    return prev, nblk, rounds


# ------------------------------------------------------------------------------------------------ 5. IDCT
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, shift):
    """jpeg_idct_islow's 1-D pass over axis 1 of d [N, 8, M] (int64)"""
    z2, z3 = d[:, 2], d[:, 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = d[:, 0], d[:, 4]
    tmp0 = (z2 + z3) << 13
    tmp1 = (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[:, 7], d[:, 5], d[:, 3], d[:, 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rows = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([_descale(r, shift) for r in rows], axis=1)


def idct(coef, qt):
    """coef [N, 64] (natural order, DC absolute), qt [64] -> u8 [N, 8, 8]"""
    d = (coef.astype(np.int64) * np.asarray(qt, np.int64)).reshape(-1, 8, 8)
    ws = _idct_pass(d, 13 - 2)                                        # columns
    px = _idct_pass(ws.transpose(0, 2, 1), 13 + 2 + 3).transpose(0, 2, 1)      # rows
    return np.clip(px + 128, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 6. upsampling and colour
def upsample(plane, hs, vs):
    """plane [ch, cw] (the component's real samples) -> [ch * vs, cw * hs], libjpeg's fancy filters where it uses them"""
    p = plane.astype(np.int64)
    ch, cw = p.shape
    if hs == 1 and vs == 1:
        return p
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)
    if vs == 1:
        left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
        right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
        out = np.empty((ch, 2 * cw), np.int64)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
        return out
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for parity, far in ((0, up), (1, down)):
        cs = 3 * p + far
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        out[parity::2, 0::2] = (3 * cs + left + 8) >> 4
        out[parity::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the whole decoder
def decode(data, subseq_bits=1024, max_rounds=64):
    """-> (pixels u8 [H, W, C] or None, info): info = {"status", "rounds", "subsequences", "blocks"} as the device's status word"""
    desc = JD.parse(data)
    if desc is None:
        return None, {"status": "not supported", "rounds": 0, "subsequences": 0, "blocks": 0}
    clean, istart, has_eoi = clean_stream(desc, data)
    if istart is None:
        return None, {"status": "damaged", "rounds": 0, "subsequences": 0, "blocks": 0}
    lanes = Lanes(desc, clean)
    subs = subsequences(istart, subseq_bits)
    states, nblk, rounds = synchronise(lanes, subs, max_rounds)
    first = np.concatenate([[0], np.cumsum(nblk)]).astype(np.int64)
    info = {"status": "ok", "rounds": rounds if rounds is not None else max_rounds, "subsequences": len(subs), "blocks": int(first[-1])}
    if rounds is None:
        info["status"] = "not converged"
        return None, info
    # 3. the write pass
    coef = np.zeros((desc.nblocks, 64), np.int32)
    per_interval = (desc.restart_interval or desc.nmcu) * desc.bpm
    damaged = int(first[-1]) != desc.nblocks or not has_eoi
    interval = -1
    for i, (s, e, hard, anchored) in enumerate(subs):
        if anchored:
            interval += 1
            damaged |= int(first[i]) != interval * per_interval
            state = (s, 0, 0)
        else:
            state = states[i - 1]
        left = lanes.run(state[0], state[1], state[2], e, hard, coef, int(first[i]) - 1)
        damaged |= e == hard and (left[1], left[2]) != (0, 0)      # the interval ends inside a block or an MCU
    if damaged:
        info["status"] = "damaged"
        return None, info
    # 4. DC: sums per component within every restart interval
    ny = desc.hs * desc.vs
    blocks = coef.reshape(desc.nmcu, desc.bpm, 64)
    ri = desc.restart_interval or desc.nmcu
    comps = [blocks[:, :ny]] + ([blocks[:, ny:ny + 1], blocks[:, ny + 1:ny + 2]] if desc.ncomp == 3 else [])
    for c in comps:
        for m0 in range(0, desc.nmcu, ri):
            seg = c[m0:m0 + ri, :, 0]
            seg[...] = np.cumsum(seg.reshape(-1)).reshape(seg.shape)
    # 5. IDCT into the block-padded planes
    planes = []
    for k, c in enumerate(comps):
        h, v = (desc.hs, desc.vs) if k == 0 else (1, 1)
        px = idct(c.reshape(-1, 64), desc.qt[desc.tq[k]]).reshape(desc.mcuy, desc.mcux, v, h, 8, 8)
        planes.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(desc.mcuy * v * 8, desc.mcux * h * 8))
    # 6. upsampling and colour
    H, W = desc.height, desc.width
    if desc.ncomp == 1:
        return planes[0][:H, :W, None].copy(), info
    cw, ch = -(-W // desc.hs), -(-H // desc.vs)
    cb, cr = (upsample(p[:ch, :cw], desc.hs, desc.vs)[:H, :W] for p in planes[1:])
    return ycc_to_rgb(planes[0][:H, :W], cb, cr), info
