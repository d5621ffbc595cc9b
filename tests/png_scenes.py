"""Seeded images for the PNG tests (PNG.md): the smallest shapes at which each stage of the encoder can go wrong.  scene(name) is a
uint8 [H, W, C] array (C = 1 or 3), the same on every call."""
import functools

import numpy as np

RUNS = (2, 3, 4, 258, 259, 260, 261, 517)


def _rng(seed):
    return np.random.default_rng(seed)


def _gradients():
    """four 12-row bands: horizontal ramp, vertical ramp, diagonal ramp, noise — every one of the five filters wins a row"""
    H, W = 12, 96
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    hor = np.broadcast_to((x * 5) % 256, (H, W))
    ver = np.broadcast_to((y * 37 + 11) % 256, (H, W))
    dia = (x * 3 + y * 7) % 256
    noise = _rng(5).integers(0, 256, size=(H, W))
    curve = ((x * x) // 16 + (y * y) * 3 + x * y // 4) % 256
    return np.concatenate([hor, ver, dia, noise, curve]).astype(np.uint8)[:, :, None]


def _runs():
    """one gray row: runs of exactly 2, 3, 4, 258, 259, 260, 261 and 517 equal bytes, neighbours differ"""
    parts = [np.full(k, 40 + 9 * i, np.uint8) for i, k in enumerate(RUNS)]
    return np.concatenate(parts)[None, :, None]


def _fibonacci():
    """one gray row whose byte values occur 1, 1, 2, 3, 5, ... times (22 values, 28 656 bytes, one stripe), shuffled: a Huffman code
    without a limit would need 21 bits"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(c, 3 + 11 * i, np.uint8) for i, c in enumerate(reversed(fib))])
    _rng(8).shuffle(vals)
    return vals[None, :, None]


def _disc():
    y, x = np.mgrid[0:40, 0:40]
    r2 = (x - 19.5) ** 2 + (y - 19.5) ** 2
    img = np.full((40, 40, 3), 255, np.uint8)
    inside = r2 < 14.0 ** 2
    shade = (200 - r2 * 0.6).clip(0, 255).astype(np.uint8)
    for c, k in enumerate((1.0, 0.7, 0.4)):
        img[:, :, c][inside] = (shade[inside] * k).astype(np.uint8)
    return img


def _stripes3():
    """33 x 700 RGB: rows of 2101 bytes, 16 rows per stripe -> three stripes, the last of one row; smooth content with flat areas"""
    H, W = 33, 700
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x // 3 + y * 2) % 256, (x * y // 50) % 256, np.where(x < 350, 90, (x + y) % 256)], axis=2).astype(np.uint8)
    noise = _rng(9).integers(0, 4, size=img.shape).astype(np.uint8)
    img[:, 500:] += noise[:, 500:]
    return img


@functools.lru_cache(maxsize=None)
def scene(name):
    img = {
        "gray-1x1": lambda: np.array([[[77]]], np.uint8),
        "rgb-1x1": lambda: np.array([[[1, 200, 30]]], np.uint8),
        "noise-17x33": lambda: _rng(1).integers(0, 256, size=(17, 33, 3), dtype=np.uint8),
        "const-5x300": lambda: np.full((5, 300, 1), 113, np.uint8),
        "runs-1x1824": _runs,
        "gradients-60x96": _gradients,
        "fibonacci-1x28656": _fibonacci,
        "stripes-33x700": _stripes3,
        "disc-40x40": _disc,
        "ragged-7x13": lambda: (_rng(2).integers(0, 3, size=(7, 13, 1)) * 100).astype(np.uint8),
        "white-9x31": lambda: np.full((9, 31, 3), 255, np.uint8),
        "noise-gray-64x64": lambda: _rng(3).integers(0, 256, size=(64, 64, 1), dtype=np.uint8),
    }[name]()
    img.setflags(write=False)
    return img


NAMES = ["gray-1x1", "rgb-1x1", "noise-17x33", "const-5x300", "runs-1x1824", "gradients-60x96", "fibonacci-1x28656", "stripes-33x700",
         "disc-40x40", "ragged-7x13", "white-9x31", "noise-gray-64x64"]
