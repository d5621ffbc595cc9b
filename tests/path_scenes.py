"""Seeded inputs of the trajectory tests (tests/test_path_cpu.py, tests/test_gpu_path.py, tests/path_guard_run.py) and of
tests/golden/make_golden_path.py: camera sets, frames with the values a quantiser can get wrong, data sets for the selection.
Input generation only; numpy."""
import math

import numpy as np

SETS = ("ring", "dome")


def _look_at_w2c(eye, target, up=(0.0, 0.0, 1.0)):
    """world-to-camera [4,4] of a COLMAP-convention camera (x right, y down, z forward) at `eye` looking at `target`"""
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 0)          # rows: camera axes in world coordinates
    w2c = np.eye(4)
    w2c[:3, :3] = R
    w2c[:3, 3] = -R @ eye
    return w2c


def camera_set(name):
    """(world_view_transform [N,4,4] float32 = W2C transposed, image height, image width); the sizes are odd on purpose"""
    if name == "ring":      # 12 cameras on a jittered ring of radius ~4 at height ~1.2, looking at a jittered point near the origin
        rng = np.random.default_rng(11)
        eyes = []
        for k in range(12):
            a = 2 * math.pi * (k + rng.uniform(-0.25, 0.25)) / 12
            r = 4.0 * (1 + rng.uniform(-0.15, 0.15))
            eyes.append(np.array([1.3 * r * math.cos(a) + 0.4, r * math.sin(a) - 0.2, 1.2 + rng.uniform(-0.3, 0.3)]))
        w2c = [_look_at_w2c(e, rng.normal(0, 0.15, 3)) for e in eyes]
        H, W = 49, 65
    elif name == "dome":    # 9 cameras on one side of a dome (a 3 x 3 grid of directions), looking down at a point, as in DTU
        rng = np.random.default_rng(23)
        w2c = []
        for i in range(3):
            for j in range(3):
                az = math.radians(-35 + 35 * j + rng.uniform(-5, 5))
                el = math.radians(35 + 15 * i + rng.uniform(-4, 4))
                r = 2.5 + rng.uniform(-0.2, 0.2)
                eye = np.array([r * math.cos(el) * math.sin(az) + 1.0, -r * math.cos(el) * math.cos(az) + 2.0, r * math.sin(el) - 0.5])
                w2c.append(_look_at_w2c(eye, np.array([1.0, 2.0, -0.5]) + rng.normal(0, 0.05, 3)))
        H, W = 37, 53
    else:
        raise KeyError(name)
    return np.stack([m.T for m in w2c]).astype(np.float32), H, W


def projection(H, W, focal_mult=1.2, znear=0.01, zfar=100.0):
    """projection_matrix (transposed, float32) of a camera with focal length focal_mult * W"""
    tx, ty = 0.5 / focal_mult, 0.5 * H / (focal_mult * W)
    P = np.zeros((4, 4), np.float32)
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / tx, 1.0 / ty, 1.0
    P[2, 2], P[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return np.ascontiguousarray(P.T)


def fov(H, W, focal_mult=1.2):
    return 2 * math.atan(0.5 / focal_mult), 2 * math.atan(0.5 * H / (focal_mult * W))


# ------------------------------------------------------------------------------------------------ frames
ODD_VALUES = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1e-3, -5.0, 1.0000001, 2.5, 3e38, -3e38, 1e-45, 0.99999994, 0.5, 1 / 3], np.float32)


def edge_values():
    """k / 255 and one ulp either side of it: where the truncation flips"""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))]).astype(np.float32)


def special_values():
    """what a quantiser can get wrong: NaN, +-inf, negatives, values above 1, +-0, and the truncation edges"""
    return np.concatenate([ODD_VALUES, edge_values()])


def frame(seed, C, H, W, normal=False):
    """[C, H, W] float32: uniform values in [-0.1, 1.1] (normal=False) or [-1.1, 1.1], with ODD_VALUES (all of them, from 15 elements
    on) and truncation edges (as many as fit into half of the rest) scattered through it"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.1 if normal else -0.1, 1.1, size=(C, H, W)).astype(np.float32)
    edge = edge_values()
    if normal:      # the values whose halves + 0.5 are the truncation edges
        edge = np.concatenate([edge, (edge * 2 - 1).astype(np.float32)])
    flat = a.reshape(-1)
    pos = rng.permutation(flat.size)
    n_odd = min(flat.size, ODD_VALUES.size)
    n_edge = min((flat.size - n_odd) // 2, edge.size)
    flat[pos[:n_odd]] = ODD_VALUES[:n_odd]
    flat[pos[n_odd:n_odd + n_edge]] = rng.permutation(edge)[:n_edge]
    return a


def depth_frame(seed, H, W, zero_frac=0.0, lo=0.8, hi=6.0):
    """[H, W] float32 depths, log-uniform in [lo, hi], with a fraction of holes (0)"""
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(math.log(lo), math.log(hi), size=(H, W))).astype(np.float32)
    nz = int(round(zero_frac * H * W))
    if nz:
        d.reshape(-1)[rng.permutation(H * W)[:nz]] = 0.0
    return d


ORDER_SIZES = (1, 2, 63, 64, 65, 257, 4097, 70001)
ORDER_KINDS = ("uniform", "three", "equal", "mixed", "ulps")


def order_data(kind, n, seed=0):
    rng = np.random.default_rng(seed + n)
    if kind == "uniform":
        return rng.uniform(-3, 3, n).astype(np.float32)
    if kind == "three":
        return rng.choice(np.array([-1.5, 0.25, 7.0], np.float32), n)
    if kind == "equal":
        return np.full(n, 1.25, np.float32)
    if kind == "mixed":      # zeros, negatives, -0, +-inf and denormals among ordinary values
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -3e-39, 1.0, -1.0, 3e38, -3e38, 0.5], np.float32)
        a = rng.choice(pool, n)
        m = rng.random(n) < 0.3
        a[m] = rng.normal(0, 1, int(m.sum())).astype(np.float32)
        return a
    if kind == "ulps":       # 2.0 + k ulp, k < 200: only the last radix pass separates them
        return (np.float32(2.0).view(np.uint32) + rng.integers(0, 200, n).astype(np.uint32)).view(np.float32)
    raise KeyError(kind)


def order_ranks(n):
    """{0, n - 1, middle, a repeated rank}, ascending"""
    return sorted([0, n // 2, n // 2, n - 1])
