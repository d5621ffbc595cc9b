"""Numpy restatements of the frame kernels of include/surfel_vis.h and of the percentile built on the selection (RENDER.md).  Checked
against the real thing — the reference's save_img_u8 expression, matplotlib's turbo colormap, np.percentile — in
tests/test_path_cpu.py; the GPU tests compare the kernels with these."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

FLT_MAX = np.finfo(np.float32).max


def quantize(planes, scale=1.0, bias=0.0):
    """[C, H, W] float32 -> [H, W, C] uint8, operation by operation as surfel_vis_quantize: fp32 multiply, fp32 add, NaN -> 0,
    +-inf -> +-FLT_MAX, clip, fp32 multiply by 255, truncation."""
    v = np.asarray(planes, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (v * np.float32(scale)).astype(np.float32) + np.float32(bias)
    y = np.where(np.isnan(y), np.float32(0), y)
    y = np.where(y == np.inf, FLT_MAX, np.where(y == -np.inf, -FLT_MAX, y)).astype(np.float32)
    y = np.minimum(np.maximum(y, np.float32(0)), np.float32(1))
    return (y * np.float32(255)).astype(np.float32).astype(np.uint8).transpose(1, 2, 0)


_TURBO = None


def turbo_table():
    """[256, 3] uint8: the committed csrc/vis_turbo_table.h"""
    global _TURBO
    if _TURBO is None:
        import gen_turbo_table
        _TURBO = gen_turbo_table.parse_header()
    return _TURBO


def turbo_index(depth, lo, hi):
    """(bin [H, W] int, black [H, W] bool) of surfel_vis_depth_turbo: fp32 log, fp64 normalisation, clip, bin = min(int(t * 256), 255)"""
    d = np.asarray(depth, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.log(d)
        assert x.dtype == np.float32
        t = (x.astype(np.float64) - np.minimum(np.float64(lo), np.float64(hi))) / np.abs(np.float64(hi) - np.float64(lo))
    black = np.isnan(t)
    t = np.clip(np.where(black, 0.0, t), 0.0, 1.0)
    return np.minimum((t * 256.0).astype(np.int64), 255), black


def depth_turbo(depth, lo, hi):
    """[H, W] float32 -> [H, W, 3] uint8"""
    idx, black = turbo_index(depth, lo, hi)
    out = turbo_table()[idx]
    out[black] = 0
    return out


def order_stats(x, ranks):
    """np.sort(x)[ranks]: numpy's order, NaN last"""
    return np.sort(np.asarray(x, np.float32).reshape(-1))[np.asarray(ranks, np.int64)]


def percentile(x, q):
    """np.percentile's linear method from order statistics: virtual index (n - 1) * (q / 100), the two neighbours, numpy's two-sided
    lerp with b - a in fp32 and the rest in fp64; NaN when the data holds one."""
    x = np.asarray(x, np.float32).reshape(-1)
    n = x.size
    s = np.sort(x)
    vi = (n - 1) * (np.asarray(q, np.float64).reshape(-1) / 100)
    lo = np.clip(np.floor(vi).astype(np.int64), 0, n - 1)
    hi = np.minimum(lo + 1, n - 1)
    g = vi - lo
    a, b = s[lo], s[hi]
    with np.errstate(invalid="ignore"):
        d = b - a                      # fp32
        out = np.where(g >= 0.5, b - d * (1 - g), a + d * g)
    if np.isnan(s[-1]):
        out = np.full_like(out, np.nan)
    return out.astype(np.float64)
