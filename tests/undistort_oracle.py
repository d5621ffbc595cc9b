"""numpy fp64 restatement of UNDISTORT.md: the distortion formula, its inverse, the undistorted camera and the image.  Independent of
the product's host code (surfel_undistort.py): the inverse here is a Newton iteration whose Jacobian comes from central differences,
the product's is analytic; every expression of the formula and of the image is written in the document's order, one rounding per
operation, which is what the device kernel (compiled without contraction) computes."""
import numpy as np

MODELS = {"SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "FULL_OPENCV": 12}

# the cameras of the issue's table: (model, params, W, H) -> (W2, H2) at blank = 0
CAMERAS = [
    ("SIMPLE_RADIAL", (60, 33.5, 24.2, 0.12), 67, 49, (62, 45)),
    ("SIMPLE_RADIAL", (60, 33.5, 24.2, -0.08), 67, 49, (67, 48)),
    ("RADIAL", (300, 161, 119, -0.15, 0.04), 320, 240, (333, 244)),
    ("OPENCV", (310, 305, 158.3, 121.9, -0.2, 0.06, 0.002, -0.003), 320, 240, (334, 246)),
    ("FULL_OPENCV", (310, 305, 158.3, 121.9, 0.1, 0.02, 0.001, -0.002, 0.003, 0.25, 0.03, 0.001), 320, 240, (331, 245)),
]


def distortion_params(model, params):
    """q = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6)"""
    p = [float(v) for v in params]
    if model not in MODELS or len(p) != MODELS[model]:
        raise ValueError("%s with %d parameters" % (model, len(p)))
    q = np.zeros(12)
    if model == "SIMPLE_RADIAL":
        q[[0, 1, 2, 3, 4]] = p[0], p[0], p[1], p[2], p[3]
    elif model == "RADIAL":
        q[[0, 1, 2, 3, 4, 5]] = p[0], p[0], p[1], p[2], p[3], p[4]
    else:
        q[:len(p)] = p
    return q


def distort(q, u, v):
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = (float(x) for x in q)
    with np.errstate(all="ignore"):
        r2 = u * u + v * v
        r4 = r2 * r2
        r6 = r4 * r2
        rad = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
        uv = u * v
        ud = u * rad + 2 * p1 * uv + p2 * (r2 + 2 * u * u)
        vd = v * rad + 2 * p2 * uv + p1 * (r2 + 2 * v * v)
    return ud, vd


def undistort_points(q, ud, vd, tol=1e-12, max_iter=100, h=1e-6):
    """(u, v) with distort(q, u, v) = (ud, vd): Newton from (ud, vd), Jacobian by central differences"""
    ud, vd = np.asarray(ud, np.float64), np.asarray(vd, np.float64)
    u, v = ud.copy(), vd.copy()
    for _ in range(max_iter):
        fu, fv = distort(q, u, v)
        au, av = distort(q, u + h, v)
        bu, bv = distort(q, u - h, v)
        cu, cv = distort(q, u, v + h)
        du_, dv_ = distort(q, u, v - h)
        j00, j10 = (au - bu) / (2 * h), (av - bv) / (2 * h)
        j01, j11 = (cu - du_) / (2 * h), (cv - dv_) / (2 * h)
        eu, ev = fu - ud, fv - vd
        det = j00 * j11 - j01 * j10
        su, sv = (j11 * eu - j01 * ev) / det, (j00 * ev - j10 * eu) / det
        u, v = u - su, v - sv
        if max(np.max(np.abs(su)), np.max(np.abs(sv))) < tol:
            return u, v
    raise RuntimeError("the inverse of the distortion did not converge")


def camera_scales(q, W, H, blank=0.0):
    """(scale_x, scale_y) of the undistorted camera before the sizes are truncated"""
    fx, fy, cx, cy = (float(x) for x in q[:4])
    rows, cols = np.arange(H) + 0.5, np.arange(W) + 0.5

    def to_pixels(px, py):
        u, v = undistort_points(q, (px - cx) / fx, (py - cy) / fy)
        return fx * u + cx, fy * v + cy
    left = to_pixels(np.full(H, 0.5), rows)[0]
    right = to_pixels(np.full(H, W - 0.5), rows)[0]
    top = to_pixels(cols, np.full(W, 0.5))[1]
    bottom = to_pixels(cols, np.full(W, H - 0.5))[1]
    max_sx = max(cx / (cx - left.max()), (W - 0.5 - cx) / (right.min() - cx))
    min_sx = min(cx / (cx - left.min()), (W - 0.5 - cx) / (right.max() - cx))
    max_sy = max(cy / (cy - top.max()), (H - 0.5 - cy) / (bottom.min() - cy))
    min_sy = min(cy / (cy - top.min()), (H - 0.5 - cy) / (bottom.max() - cy))
    sx = float(np.clip(1.0 / (min_sx * blank + max_sx * (1.0 - blank)), 0.2, 2.0))
    sy = float(np.clip(1.0 / (min_sy * blank + max_sy * (1.0 - blank)), 0.2, 2.0))
    return sx, sy


def undistorted_camera(q, W, H, blank=0.0):
    """(W2, H2, fx, fy, cx2, cy2)"""
    sx, sy = camera_scales(q, W, H, blank)
    W2, H2 = max(1, int(sx * W)), max(1, int(sy * H))
    return W2, H2, float(q[0]), float(q[1]), float(q[2]) * W2 / W, float(q[3]) * H2 / H


def source_coordinates(q, pinhole, size):
    """(xs, ys) [H2, W2]: where every output pixel centre falls in the source, in pixel-index coordinates"""
    W2, H2 = size
    fx2, fy2, cx2, cy2 = (float(x) for x in pinhole)
    x, y = np.meshgrid(np.arange(W2, dtype=np.float64), np.arange(H2, dtype=np.float64))
    u, v = (x + 0.5 - cx2) / fx2, (y + 0.5 - cy2) / fy2
    ud, vd = distort(q, u, v)
    with np.errstate(all="ignore"):
        return float(q[0]) * ud + float(q[2]) - 0.5, float(q[1]) * vd + float(q[3]) - 0.5


def undistort(src, q, pinhole, size, return_valid=False):
    """u8 [H, W, C] -> u8 [H2, W2, C]; size = (W2, H2)"""
    H, W, C = src.shape
    xs, ys = source_coordinates(q, pinhole, size)
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(xs), np.floor(ys)
        valid = (0 <= x0) & (x0 + 1 <= W - 1) & (0 <= y0) & (y0 + 1 <= H - 1)
        dx, dy = xs - x0, ys - y0
    xi, yi = np.where(valid, x0, 0).astype(np.int64), np.where(valid, y0, 0).astype(np.int64)
    out = np.zeros((size[1], size[0], C), np.uint8)
    if W < 2 or H < 2:
        return (out, valid) if return_valid else out
    s = src.astype(np.float64)
    dxv, dyv = np.where(valid, dx, 0.0), np.where(valid, dy, 0.0)
    for c in range(C):
        top = (1 - dxv) * s[yi, xi, c] + dxv * s[yi, xi + 1, c]
        bot = (1 - dxv) * s[yi + 1, xi, c] + dxv * s[yi + 1, xi + 1, c]
        val = (1 - dyv) * top + dyv * bot
        out[:, :, c] = np.where(valid, np.floor(val + 0.5), 0).astype(np.uint8)
    return (out, valid) if return_valid else out


# ---- the geometry anchor: a pattern of the undistorted ray direction, painted without the forward map
def pattern(u, v):
    return np.stack([127.5 + 100 * np.sin(3 * u + 1) * np.cos(2 * v), 127.5 + 100 * np.cos(4 * u * v + u), 127.5 + 100 * np.sin(2.5 * v - u)], axis=-1)


def paint_distorted(q, W, H):
    """u8 [H, W, 3]: the pattern as the distorted camera sees it, through the inverse at every distorted pixel centre"""
    fx, fy, cx, cy = (float(x) for x in q[:4])
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    u, v = undistort_points(q, (x - cx) / fx, (y - cy) / fy)
    return np.floor(pattern(u, v) + 0.5).astype(np.uint8)


def warp_to_distorted(img, q, pinhole):
    """u8 [H, W, C] taken with the pinhole (fx, fy, cx, cy) -> the same view as the distorted camera q of the same size sees it
    (bilinear, clamped to the frame): how the end-to-end test makes a distorted capture out of pinhole renders"""
    H, W, C = img.shape
    fx, fy, cx, cy = (float(x) for x in q[:4])
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    u, v = undistort_points(q, (x - cx) / fx, (y - cy) / fy)
    xs = np.clip(pinhole[0] * u + pinhole[2] - 0.5, 0, W - 1)
    ys = np.clip(pinhole[1] * v + pinhole[3] - 0.5, 0, H - 1)
    x0, y0 = np.minimum(np.floor(xs), W - 2).astype(np.int64), np.minimum(np.floor(ys), H - 2).astype(np.int64)
    dx, dy = (xs - x0)[:, :, None], (ys - y0)[:, :, None]
    s = img.astype(np.float64)
    val = (1 - dy) * ((1 - dx) * s[y0, x0] + dx * s[y0, x0 + 1]) + dy * ((1 - dx) * s[y0 + 1, x0] + dx * s[y0 + 1, x0 + 1])
    return np.floor(val + 0.5).astype(np.uint8)
