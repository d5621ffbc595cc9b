"""JPEG fixtures of the decoder tests, made at test time by Pillow's encoder from seeded arrays: every image is a smooth ramp plus
noise, so the streams are neither trivial nor incompressible.  jpeg(name) -> the file's bytes; pixels(name) -> what Pillow decodes
(read-only, computed once).  Sizes are width x height."""
import functools
import io

import numpy as np

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def ramp_noise(seed, h, w, c, noise=24, slope=None):
    """slope None: steep ramps that wrap (sharp edges); a number: gentle ramps of that relative slope"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if slope is None:
        chans = [(x * (3 + k) + y * (5 - k) + 40 * k) % 256 * 0.8 + 20 for k in range(c)]
    else:
        chans = [(x * (1 + k) * 0.7 + y * (3 - k) * 0.5) * slope + 40 + 40 * k for k in range(c)]
    a = np.stack(chans, axis=2) + rng.normal(0, noise, size=(h, w, c))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _save(a, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(f, "JPEG", **kw)
    return f.getvalue()


# (seed, noise, slope) per fixture: the noisiest content of a short search whose stream reaches its fixed point within 16 rounds at
# 128-bit subsequences (JPEGDEC.md "Rounds": half the default cap is 18).  A blind decoder has to find the bit, the coefficient index
# AND the block slot of the MCU again, so streams of long blocks (quality 100, 4:2:0) need the gentlest content.
CONTENT = {
    "rgb-40x56-420-q30": (0, 24, None), "rgb-40x56-420-q30-opt": (0, 24, None), "rgb-40x56-420-q90": (0, 4, 1.0),
    "rgb-40x56-420-q90-opt": (0, 4, 1.0), "rgb-40x56-420-q100": (3, 0.5, 0.5), "rgb-40x56-420-q100-opt": (0, 0.5, 0.5),
    "rgb-40x56-422-q30": (0, 24, None), "rgb-40x56-422-q30-opt": (0, 24, None), "rgb-40x56-422-q90": (2, 8, None),
    "rgb-40x56-422-q90-opt": (3, 8, None), "rgb-40x56-422-q100": (2, 1, 1.0), "rgb-40x56-422-q100-opt": (0, 0, 1.0),
    "rgb-40x56-444-q30": (0, 24, None), "rgb-40x56-444-q30-opt": (0, 24, None), "rgb-40x56-444-q90": (3, 12, None),
    "rgb-40x56-444-q90-opt": (0, 4, None), "rgb-40x56-444-q100": (1, 1, 1.0), "rgb-40x56-444-q100-opt": (2, 0.5, 1.0),
}


def _main(name, sub, quality, optimize):
    seed, noise, slope = CONTENT[name]
    return lambda: _save(ramp_noise(seed, 56, 40, 3, noise, slope), quality=quality, subsampling=SUBSAMPLING[sub], optimize=optimize)


FIXTURES = {}
for _sub in ("420", "422", "444"):
    for _q in (30, 90, 100):
        for _opt in (False, True):
            _name = "rgb-40x56-%s-q%d%s" % (_sub, _q, "-opt" if _opt else "")
            FIXTURES[_name] = _main(_name, _sub, _q, _opt)
FIXTURES.update({
    "rgb-33x17-420": lambda: _save(ramp_noise(0, 17, 33, 3, 12), quality=90, subsampling=2),
    "rgb-17x33-420": lambda: _save(ramp_noise(1, 33, 17, 3, 24), quality=90, subsampling=2),
    "rgb-33x17-422": lambda: _save(ramp_noise(0, 17, 33, 3, 24), quality=85, subsampling=1),
    "rgb-4x17-420": lambda: _save(ramp_noise(4, 17, 4, 3), quality=90, subsampling=2),
    "rgb-8x8-420": lambda: _save(ramp_noise(5, 8, 8, 3), quality=90, subsampling=2),
    "rgb-1x1-420": lambda: _save(ramp_noise(6, 1, 1, 3), quality=90, subsampling=2),
    "gray-40x56": lambda: _save(ramp_noise(1, 56, 40, 1, 12), quality=90),
    "rgb-48x48-420-rows": lambda: _save(ramp_noise(2, 48, 48, 3, 2), quality=90, subsampling=2, restart_marker_rows=1),
    "rgb-48x48-420-blocks3": lambda: _save(ramp_noise(2, 48, 48, 3, 2), quality=90, subsampling=2, restart_marker_blocks=3),
    # 3 MCUs per row, a restart marker every 2: intervals that do not align with the MCU rows (at 48 x 48 three MCUs are a row)
    "rgb-40x56-420-blocks2": lambda: _save(ramp_noise(1, 56, 40, 3, 4), quality=90, subsampling=2, restart_marker_blocks=2),
    # noise at quality 100: a stuffed zero every hundred bytes; a restart marker per block keeps its long blocks anchored
    "noise-64x64-q100": lambda: _save(np.random.default_rng(10).integers(0, 256, size=(64, 64, 1), dtype=np.uint8), quality=100, restart_marker_blocks=1),
    "constant-64x64": lambda: _save(np.full((64, 64, 3), (200, 90, 30), np.uint8), quality=90, subsampling=2),
})
NAMES = list(FIXTURES)
SYNC = "rgb-40x56-444-q90"            # no restart markers: at 128 bits every subsequence but the first starts blind


@functools.lru_cache(maxsize=None)
def jpeg(name):
    return FIXTURES[name]()


@functools.lru_cache(maxsize=None)
def pixels(name):
    return pillow(jpeg(name))


def pillow(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    a = a[:, :, None] if a.ndim == 2 else a
    a = np.array(a)
    a.setflags(write=False)
    return a


def own_encoder():
    """a file of the project's own encoder as tests/video_oracle.py restates it (one restart interval per MCU row)"""
    import video_oracle as VO
    return VO.encode(ramp_noise(2, 40, 56, 3, 0.5), quality=90)


def truncated(name=SYNC):
    """the fixture cut off in the middle of its entropy-coded segment"""
    import surfel_jpegdec as JD
    data = jpeg(name)
    d = JD.parse(data)
    return data[:d.ecs_offset + (len(data) - d.ecs_offset) // 2]


def cut_before_eoi(name, k, keep_eoi=False):
    """the fixture without the k bytes in front of its EOI marker, and without the marker unless keep_eoi"""
    data = jpeg(name)
    eoi = data.rindex(b"\xff\xd9")
    return data[:eoi - k] + (data[eoi:] if keep_eoi else b"")


CUT_NAMES = ("rgb-40x56-420-q90", "rgb-40x56-444-q30", "rgb-48x48-420-rows")


def progressive():
    return _save(ramp_noise(12, 30, 44, 3), quality=90, progressive=True)


def cmyk():
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(ramp_noise(13, 16, 16, 4), "CMYK").save(f, "JPEG", quality=90)
    return f.getvalue()


def with_segment(data, marker, payload):
    """the file with one more segment right behind SOI"""
    return data[:2] + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload + data[2:]


def photo(seed, h, w, quality=92):
    """a synthetic "photo": smooth ramp plus noise, 4:2:0, as a camera writes them"""
    return _save(ramp_noise(seed, h, w, 3, noise=12), quality=quality, subsampling=2)
