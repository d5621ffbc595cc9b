"""numpy restatement of the capture loader's image path (include/surfel_scene.h, SCENE.md), independent of Pillow and of the library:
the BICUBIC resampling tables (a), the horizontal (b) and vertical (c) 8-bit passes, the float conversion (d), the Blender composite (e)
and the resolution rule.  Every function is exact integer / IEEE arithmetic, so the tests compare with array_equal."""
import math

import numpy as np

PRECISION_BITS = 22


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def tables(in_size, out_size):
    """(ksize, bounds [out, 2] int32 = (first source sample, taps used), coeffs [out, ksize] int32 = weights x 2^22) of one axis.  Python
    floats are IEEE doubles and every operation below is a single one, so this rounds as the C it restates."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, k in enumerate(w):
            coeffs[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, coeffs


def _pass(src, out_size, cols=None):
    """resample axis 1 of src [A, in, ...] u8 to out_size samples (cols: only these output indices)"""
    _, bounds, coeffs = tables(src.shape[1], out_size)
    idx = range(out_size) if cols is None else cols
    out = np.zeros((src.shape[0], len(idx)) + src.shape[2:], np.uint8)
    s = src.astype(np.int64)
    for j, xx in enumerate(idx):
        xmin, n = bounds[xx]
        k = coeffs[xx, :n].astype(np.int64).reshape((1, n) + (1,) * (src.ndim - 2))
        acc = (1 << (PRECISION_BITS - 1)) + (s[:, xmin:xmin + n] * k).sum(axis=1)
        assert np.abs(acc).max() < 2 ** 31
        out[:, j] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resample_h(src, W2, cols=None):
    """src [H, W, C] u8 -> [H, W2, C] u8"""
    return _pass(src, W2, cols)


def resample_v(src, H2, rows=None):
    """src [H, W, C] u8 -> [H2, W, C] u8"""
    return np.ascontiguousarray(_pass(np.ascontiguousarray(src.transpose(1, 0, 2)), H2, rows).transpose(1, 0, 2))


def resize(src, W2, H2):
    """Pillow's order: the horizontal pass first, rounded to u8, then the vertical one; a pass is skipped when its axis keeps its size.
    Returns (result, the intermediate after the horizontal pass)."""
    H, W, _ = src.shape
    mid = resample_h(src, W2) if W2 != W else src
    return (resample_v(mid, H2) if H2 != H else mid), mid


def to_float(u8):
    """[H, W, C] u8 -> (planes [min(C, 3), H, W] fp32, mask [1, H, W] fp32 or None): v / 255 with IEEE fp32 division"""
    f = (u8.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    return np.ascontiguousarray(f[:3]), (np.ascontiguousarray(f[3:4]) if u8.shape[2] == 4 else None)


def composite(rgba, white):
    """[H, W, 4] u8 -> [H, W, 3] u8 over a black or white background, fp64, truncated"""
    n = rgba.astype(np.float64) / 255.0
    bg = 1.0 if white else 0.0
    arr = n[:, :, :3] * n[:, :, 3:4] + bg * (1.0 - n[:, :, 3:4])
    return (arr * 255.0).astype(np.int64).astype(np.uint8)


def target_resolution(w, h, resolution, resolution_scale=1.0):
    """(width, height) a w x h image is loaded at for the -r value `resolution`"""
    if resolution in (1, 2, 4, 8):
        return round(w / (resolution_scale * resolution)), round(h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = w / 1600 if w > 1600 else 1
    else:
        global_down = w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(w / scale), int(h / scale)
