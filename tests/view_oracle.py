"""Numpy fp32 restatement of the viewer's image rules (include/surfel_view.h, VIEWER.md), operation by operation.  Checked against the
reference's own render_net_image and byte conversion in tests/test_view_cpu.py (fixture tests/golden/ref_view.npz); the GPU tests
compare the kernels with it.

Besides the bytes, the colouring returns t * 255 per pixel in fp64.  A pixel is INDETERMINATE when that value lies within HALF_BAND of
a half-integer: there a last-bit difference in t (the reference sums its convolution in another order than the stated one, and takes
sqrt per channel before the L2 norm) moves the rounded table index by one."""
import numpy as np

import path_oracle as PO

MODES = ["RGB", "Alpha", "Normal", "Depth", "Edge", "Curvature"]
HALF_BAND = 1e-3
f32 = np.float32


def gradient(planes, scale=1.0, bias=0.0):
    """[3, H, W] float32 -> m [H, W] float32: Sobel / 4 with zero padding per channel of planes * scale + bias, L2 over the channels,
    in the order surfel_view.h states."""
    p = np.asarray(planes, f32)
    C, H, W = p.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v = (p * f32(scale)).astype(f32) + f32(bias)
        pad = np.zeros((C, H + 2, W + 2), f32)
        pad[:, 1:-1, 1:-1] = v
        a, b, c = pad[:, :-2, :-2], pad[:, :-2, 1:-1], pad[:, :-2, 2:]
        d, f = pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]
        g, h, i = pad[:, 2:, :-2], pad[:, 2:, 1:-1], pad[:, 2:, 2:]
        gx = ((c - a) * f32(0.25) + (f - d) * f32(0.5)) + (i - g) * f32(0.25)
        gy = ((g - a) * f32(0.25) + (h - b) * f32(0.5)) + (i - c) * f32(0.25)
        q = gx * gx + gy * gy
        s = (q[0] + q[1]) + q[2]
        m = np.sqrt(s)
    assert m.dtype == f32
    return m


def limits(m):
    """(lo, hi) float32 over the pixels that are not NaN; (NaN, NaN) when there is none"""
    m = np.asarray(m, f32)
    ok = ~np.isnan(m)
    if not ok.any():
        return f32(np.nan), f32(np.nan)
    return m[ok].min(), m[ok].max()


def colour_index(m):
    """(idx [H, W] int64 with 0 where t is NaN, t255 [H, W] float64 with NaN there)"""
    m = np.asarray(m, f32)
    lo, hi = limits(m)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (m - lo) / (hi - lo)
        assert t.dtype == f32
        r = np.rint(t * f32(255))
        t255 = (m.astype(np.float64) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 255.0
    bad = np.isnan(t)
    idx = np.clip(np.where(bad, 0, r), 0, 255).astype(np.int64)
    return idx, np.where(bad, np.nan, t255)


def colour(m):
    """m [H, W] float32 -> (bytes [H, W, 3] uint8, t255 [H, W] float64)"""
    idx, t255 = colour_index(m)
    return PO.turbo_table()[idx], t255


def indeterminate(t255):
    """[H, W] bool: t * 255 within HALF_BAND of k + 0.5"""
    with np.errstate(invalid="ignore"):
        frac = t255 - np.floor(t255)
        return np.abs(frac - 0.5) <= HALF_BAND


def scalar_map(pkg, mode):
    """the map m of a colour-mapped mode"""
    name = MODES[mode] if isinstance(mode, int) else mode
    if name == "Alpha":
        return np.asarray(pkg["rend_alpha"], f32).reshape(pkg["rend_alpha"].shape[-2:])
    if name == "Depth":
        return np.asarray(pkg["surf_depth"], f32).reshape(pkg["surf_depth"].shape[-2:])
    if name == "Edge":
        return gradient(pkg["render"])
    if name == "Curvature":
        return gradient(pkg["rend_normal"], 0.5, 0.5)
    raise KeyError(name)


def net_image(pkg, mode):
    """(bytes [H, W, 3] uint8, indeterminate [H, W] bool) of a render package (numpy arrays) in one of the six modes"""
    name = MODES[mode] if isinstance(mode, int) else mode
    if name == "RGB":
        out = PO.quantize(pkg["render"], 1.0, 0.0)
        return out, np.zeros(out.shape[:2], bool)
    if name == "Normal":
        out = PO.quantize(pkg["rend_normal"], 0.5, 0.5)
        return out, np.zeros(out.shape[:2], bool)
    out, t255 = colour(scalar_map(pkg, name))
    return out, indeterminate(t255)
