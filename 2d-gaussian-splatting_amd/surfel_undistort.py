"""Undistortion of a COLMAP capture (UNDISTORT.md): what the reference leaves to COLMAP's image_undistorter (convert.py:68-78).

The camera rule runs on the host in numpy fp64, once per COLMAP camera: the four supported models become one 12-parameter vector, the
distorted image's border is carried through the inverse of the distortion formula (Newton), and the undistorted size follows from the
border's extremes.  The image runs on the device in HIP (include/surfel_undistort.h, csrc/scene_undistort.hip): one fp64 bilinear
sample per output pixel.  There is no host fallback for the image: a CPU tensor is refused.
"""
import ctypes as C

import numpy as np
import torch

import surfel_native as _n

# model -> number of COLMAP parameters; the fisheye, FOV and thin-prism models need atan and stay refused
MODELS = {"SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "FULL_OPENCV": 12}
MIN_SCALE, MAX_SCALE = 0.2, 2.0      # image_undistorter's defaults [UPSTREAM-RECALL]
NEWTON_TOL, NEWTON_ITERATIONS = 1e-12, 100


def distortion_params(model, params):
    """q[12] = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) of a COLMAP camera, zeros for what its model lacks"""
    if model not in MODELS:
        raise ValueError("COLMAP camera model %s cannot be undistorted: supported are %s" % (model, ", ".join(MODELS)))
    p = np.asarray(params, np.float64).reshape(-1)
    if p.size != MODELS[model]:
        raise ValueError("COLMAP camera model %s takes %d parameters, got %d" % (model, MODELS[model], p.size))
    q = np.zeros(12)
    if model == "SIMPLE_RADIAL":          # f, cx, cy, k
        q[:5] = p[0], p[0], p[1], p[2], p[3]
    elif model == "RADIAL":               # f, cx, cy, k1, k2
        q[:6] = p[0], p[0], p[1], p[2], p[3], p[4]
    else:                                 # fx, fy, cx, cy, k1, k2, p1, p2 [, k3, k4, k5, k6]
        q[:p.size] = p
    if not np.all(np.isfinite(q)) or q[0] <= 0 or q[1] <= 0:
        raise ValueError("COLMAP camera model %s: parameters must be finite and the focal lengths positive" % model)
    return q


def _distort_jacobian(q, u, v):
    """(ud, vd) of the formula and its Jacobian d(ud, vd) / d(u, v), on arrays"""
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(x) for x in q[4:])
    r2 = u * u + v * v
    r4 = r2 * r2
    r6 = r4 * r2
    num = 1 + k1 * r2 + k2 * r4 + k3 * r6
    den = 1 + k4 * r2 + k5 * r4 + k6 * r6
    rad = num / den
    uv = u * v
    ud = u * rad + 2 * p1 * uv + p2 * (r2 + 2 * u * u)
    vd = v * rad + 2 * p2 * uv + p1 * (r2 + 2 * v * v)
    drad = ((k1 + 2 * k2 * r2 + 3 * k3 * r4) * den - num * (k4 + 2 * k5 * r2 + 3 * k6 * r4)) / (den * den)      # d rad / d r2
    ru, rv = 2 * u * drad, 2 * v * drad
    return ud, vd, rad + u * ru + 2 * p1 * v + 6 * p2 * u, u * rv + 2 * p1 * u + 2 * p2 * v, v * ru + 2 * p2 * v + 2 * p1 * u, rad + v * rv + 2 * p2 * u + 6 * p1 * v


def undistort_points(q, ud, vd):
    """(u, v) whose distortion is (ud, vd): Newton from (ud, vd) until the step falls below 1e-12, at most 100 iterations"""
    ud, vd = np.asarray(ud, np.float64), np.asarray(vd, np.float64)
    u, v = ud.copy(), vd.copy()
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_ITERATIONS):
            fu, fv, a, b, c, d = _distort_jacobian(q, u, v)
            eu, ev = fu - ud, fv - vd
            det = a * d - b * c
            su, sv = (d * eu - b * ev) / det, (a * ev - c * eu) / det
            u, v = u - su, v - sv
            step = max(float(np.max(np.abs(su))), float(np.max(np.abs(sv))))      # a NaN step compares false and never converges
            if step < NEWTON_TOL:
                return u, v
    raise ValueError("the inverse of the distortion did not converge in %d iterations: the parameters do not describe a lens" % NEWTON_ITERATIONS)


def undistorted_camera(q, W, H, blank=0.0):
    """(W2, H2, fx, fy, cx2, cy2): the PINHOLE camera an image of W x H taken with q is undistorted into (UNDISTORT.md, the camera
    rule).  blank = 0: no output pixel looks outside the source; blank = 1: every source pixel is kept."""
    q = np.asarray(q, np.float64)
    W, H = int(W), int(H)
    fx, fy, cx, cy = (float(x) for x in q[:4])
    rows, cols = np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5

    def border(px, py):
        u, v = undistort_points(q, (px - cx) / fx, (py - cy) / fy)
        return fx * u + cx, fy * v + cy
    left_x = border(np.full(H, 0.5), rows)[0]
    right_x = border(np.full(H, W - 0.5), rows)[0]
    top_y = border(cols, np.full(W, 0.5))[1]
    bottom_y = border(cols, np.full(W, H - 0.5))[1]
    max_scale_x = max(cx / (cx - left_x.max()), (W - 0.5 - cx) / (right_x.min() - cx))
    min_scale_x = min(cx / (cx - left_x.min()), (W - 0.5 - cx) / (right_x.max() - cx))
    max_scale_y = max(cy / (cy - top_y.max()), (H - 0.5 - cy) / (bottom_y.min() - cy))
    min_scale_y = min(cy / (cy - top_y.min()), (H - 0.5 - cy) / (bottom_y.max() - cy))
    scale_x = min(max(1.0 / (min_scale_x * blank + max_scale_x * (1.0 - blank)), MIN_SCALE), MAX_SCALE)
    scale_y = min(max(1.0 / (min_scale_y * blank + max_scale_y * (1.0 - blank)), MIN_SCALE), MAX_SCALE)
    if not (np.isfinite(scale_x) and np.isfinite(scale_y)):
        raise ValueError("the undistorted camera's scale is not finite: the principal point lies on the image border")
    W2, H2 = max(1, int(scale_x * W)), max(1, int(scale_y * H))
    return W2, H2, fx, fy, cx * W2 / W, cy * H2 / H


def undistort(src, q, pinhole, size):
    """u8 [H, W, C] on the device (C = 1, 3, 4), taken with the camera q[12] -> u8 [H2, W2, C] as the pinhole (fx2, fy2, cx2, cy2)
    sees it; size = (W2, H2).  Pixels that look outside the source are 0 in every channel."""
    if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() != 3:
        raise ValueError("expected a uint8 [H, W, C] tensor")
    src = _n.device_tensor("libsurfel_hip", src).contiguous()
    H, W, Cn = (int(v) for v in src.shape)
    W2, H2 = int(size[0]), int(size[1])
    qa = (C.c_double * 12)(*[float(v) for v in np.asarray(q, np.float64).reshape(12)])
    pa = (C.c_double * 4)(*[float(v) for v in np.asarray(pinhole, np.float64).reshape(4)])
    if W2 <= 0 or H2 <= 0:
        raise ValueError("the undistorted size must be positive, got %d x %d" % (W2, H2))
    out = torch.empty((H2, W2, Cn), dtype=torch.uint8, device=src.device)
    _n.call(src.device, "surfel_scene_undistort", H, W, Cn, H2, W2, qa, pa, src, out)
    return out
