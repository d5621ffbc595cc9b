"""Seeded frames for the JPEG / video tests (VIDEO.md).  Sizes are the smallest at which each mechanism of the encoder can fail; every
content but the flat one appears at 150 x 218 (10 MCU rows: the restart counter wraps), every other size carries one or two.  The flat
frame sits at 37 x 51: its blocks cost two bits each, so its file is the header plus the restart intervals' fixed costs (DRI, one
marker, one padding byte and three DC resets per MCU row) and says nothing about the coded data a size ratio is meant to bound.  The 1 x 1 frame is the
flat colour too: one pixel is a flat frame whatever the generator is called, and its three samples make an error measure that moves in
steps of a third.  The other one-MCU sizes carry the checkerboard and noise: on 64 or 256 pixels of smooth content a handful of rounding
decisions decide the decoded error (over twelve seeds the ratio to libjpeg's ran from 0.72 to 1.42 at 8 x 8, median 1.00), so an
error ratio there measures the seed; where the quantiser dominates the error it ran from 0.99 to 1.01."""
import numpy as np

QUALITIES = (50, 75, 95, 100)
SIZES = ((1, 1), (8, 8), (16, 16),      # one MCU, all padding
         (17, 33), (37, 51),            # padding on both axes
         (150, 218),                    # 10 MCU rows: RST7 is followed by RST0
         (272, 16),                     # 17 rows of one MCU: the counter wraps twice
         (16, 1040))                    # 65 MCUs in a row: one more than a wave has lanes
CONTENTS = ("smooth", "edges", "noise", "flat", "checker", "highfreq")
SCENES = [("%s-150x218" % c, c, 150, 218) for c in CONTENTS if c != "flat"] + [("flat-37x51", "flat", 37, 51),
    ("flat-1x1", "flat", 1, 1), ("checker-8x8", "checker", 8, 8), ("noise-16x16", "noise", 16, 16), ("edges-17x33", "edges", 17, 33),
    ("smooth-37x51", "smooth", 37, 51), ("highfreq-272x16", "highfreq", 272, 16), ("noise-16x1040", "noise", 16, 1040)]
NAMES = [s[0] for s in SCENES]


def content(kind, H, W, seed=0):
    """uint8 [H, W, 3]"""
    rng = np.random.default_rng([seed, H, W, CONTENTS.index(kind)])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "smooth":      # sinusoids
        ch = [0.5 + 0.5 * np.sin(x / (7.0 + 3 * k) + k) * np.cos(y / (5.0 + 2 * k) - k) for k in range(3)]
        img = np.stack(ch, -1) * 255.0
    elif kind == "edges":     # two-colour checker cells with noise
        cell = ((y // 11 + x // 13) % 2)[..., None]
        img = np.where(cell > 0, np.array([230.0, 40.0, 90.0]), np.array([20.0, 200.0, 160.0])) + rng.normal(0, 6.0, (H, W, 3))
    elif kind == "noise":
        return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    elif kind == "flat":      # saturated
        img = np.broadcast_to(np.array([255.0, 0.0, 255.0]), (H, W, 3))
    elif kind == "checker":   # 1-pixel 0 / 255: the largest coefficients
        img = np.broadcast_to((((y + x) % 2) * 255.0)[..., None], (H, W, 3))
    elif kind == "highfreq":  # the highest-frequency basis function of every 8 x 8 block at a low amplitude: zero runs longer than 15
        c = np.cos((2 * (np.arange(8) % 8) + 1) * 7 * np.pi / 16)
        amp = 16.0 + 6.0 * ((y // 8 + x // 8) % 3)
        img = np.broadcast_to((128.0 + amp * c[y.astype(int) % 8] * c[x.astype(int) % 8])[..., None], (H, W, 3))
    else:
        raise KeyError(kind)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def scene(name):
    _, kind, H, W = SCENES[NAMES.index(name)]
    return content(kind, H, W)


def frames(n, H, W, seed=5):
    """n different frames of one size (a drifting smooth pattern plus a little noise)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for k in range(n):
        ch = [0.5 + 0.5 * np.sin((x + 3 * k) / (6.0 + c) + c) * np.cos((y - 2 * k) / (4.0 + c)) for c in range(3)]
        out.append(np.clip(np.rint(np.stack(ch, -1) * 255.0 + rng.normal(0, 3.0, (H, W, 3))), 0, 255).astype(np.uint8))
    return out
