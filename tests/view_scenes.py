"""Seeded inputs of the viewer tests (tests/test_view_cpu.py, tests/test_gpu_view.py, tests/view_guard_run.py) and of
tests/golden/make_golden_view.py: render packages (smooth fields plus noise, so that the Sobel modes see edges and flat areas) and the
viewer's camera messages.  Input generation only; numpy."""
import json
import math

import numpy as np

RENDER_ITEMS = ["RGB", "Alpha", "Normal", "Depth", "Edge", "Curvature"]
GOLDEN_SHAPES = ((23, 37), (48, 64))
GPU_SHAPES = ((1, 1), (1, 5), (7, 1), (23, 37), (48, 64), (33, 130), (180, 320))


def package(H, W, seed=None):
    """The four maps of a render package a viewer mode reads, float32: render [3,H,W] in about [-0.05, 1.05] (the quantiser's clamp
    has work to do), rend_alpha [1,H,W] in [0, 1], rend_normal [3,H,W] of at most unit length, surf_depth [1,H,W] with holes (0)."""
    rng = np.random.default_rng(1000 * H + W if seed is None else seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)

    def smooth(k):
        f = np.zeros((H, W))
        for _ in range(3):
            a, b, p = rng.uniform(1, 6, 3)
            f += rng.uniform(0.2, 1.0) * np.sin(a * u * math.pi + p) * np.cos(b * v * math.pi - p)
        step = (u * rng.uniform(0.5, 1.5) + v * rng.uniform(0.5, 1.5) > rng.uniform(0.6, 1.2)) * rng.uniform(0.3, 0.8)      # a hard edge
        return f / 3 + step + k

    render = np.stack([0.5 + 0.4 * smooth(0.0) + rng.normal(0, 0.02, (H, W)) for _ in range(3)])
    alpha = np.clip(0.5 + 0.6 * smooth(0.0) + rng.normal(0, 0.01, (H, W)), 0.0, 1.0)[None]
    nrm = np.stack([smooth(0.0), smooth(0.0), 0.7 + 0.3 * smooth(0.0)]) + rng.normal(0, 0.03, (3, H, W))
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=0, keepdims=True), 1e-6) * alpha
    depth = (2.5 + 1.5 * smooth(0.0) + rng.normal(0, 0.01, (H, W)))[None] * (alpha > 0.05)
    return {"render": render.astype(np.float32), "rend_alpha": alpha.astype(np.float32), "rend_normal": nrm.astype(np.float32),
            "surf_depth": depth.astype(np.float32)}


def scalar_map(H, W, seed):
    return package(H, W, seed)["surf_depth"][0]


# ------------------------------------------------------------------------------------------------ the viewer's messages
def message(width, height, mode, seed=0, train=1, keep_alive=1, scaling_modifier=1.0):
    """A camera message as the remote viewer sends it (the field names network_gui.receive reads): a look-at camera, the matrices as
    flat lists of 16 floats."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * math.pi)
    eye = np.array([4 * math.cos(a), rng.uniform(-1, 1), 4 * math.sin(a)])
    z = -eye / np.linalg.norm(eye)
    xax = np.cross(z, [0.0, -1.0, 0.0]); xax /= np.linalg.norm(xax)
    yax = np.cross(z, xax)
    R = np.stack([xax, yax, z], 0)
    w2c = np.eye(4); w2c[:3, :3] = R; w2c[:3, 3] = -R @ eye
    fovx = math.radians(50.0)
    fovy = 2 * math.atan(math.tan(fovx / 2) * max(height, 1) / max(width, 1))
    zn, zf = 0.01, 100.0
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2] = 1 / math.tan(fovx / 2), 1 / math.tan(fovy / 2), 1.0
    P[2, 2], P[2, 3] = zf / (zf - zn), -(zf * zn) / (zf - zn)
    flip = np.diag([1.0, -1.0, -1.0, 1.0])      # the viewer's axes: network_gui.receive negates columns 1 and 2 again
    view = (w2c.T @ flip).astype(np.float32)
    full = ((w2c.T @ P.T) @ np.diag([1.0, -1.0, 1.0, 1.0])).astype(np.float32)
    return {"resolution_x": int(width), "resolution_y": int(height), "train": int(train), "fov_y": fovy, "fov_x": fovx, "z_near": zn,
            "z_far": zf, "keep_alive": int(keep_alive), "scaling_modifier": float(scaling_modifier),
            "view_matrix": [float(t) for t in view.reshape(-1)], "view_projection_matrix": [float(t) for t in full.reshape(-1)],
            "render_mode": int(mode)}


def frame_message(msg):
    """4-byte little-endian length + JSON: what the viewer puts on the wire"""
    body = json.dumps(msg).encode("utf-8")
    return len(body).to_bytes(4, "little") + body
