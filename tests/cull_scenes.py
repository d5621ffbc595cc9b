"""The scene of the view-culling tests (CULL.md §Pinning), regenerated from parameters and never stored: a bumpy lat-long ellipsoid of
1800 triangles with its pole slivers at distance 2 from 24 cameras on an arc, one camera looking away, and the triangles a rasteriser
can go wrong on — one that crosses the near plane and the eye plane of the middle camera, a backdrop behind the object that fills the
middle camera's screen inside [znear, zfar], one beyond zfar, two with det = 0, two with an index outside the vertices, one with a
NaN vertex.  Images are 96 x 64 and 67 x 45 with the principal point off the centre by a non-integer: the smallest shapes at which both
size classes, the queue, the conservative box, the clamps and batching with a remainder are all live."""
import functools
import json

import numpy as np

SCENE = {"nlat": 24, "nlon": 36, "axes": [0.75, 0.55, 0.7], "bump": 0.08, "distance": 2.0, "views": 24, "arc_deg": 14.0, "elev": 0.1,
         "znear": 0.01, "zfar": 20.0, "eps": 0.005, "jitter_seed": 24}
# (H, W, f, cx - (W - 1) / 2, cy - (H - 1) / 2)
SIZES = {"large": (64, 96, 85.0, 2.3, -1.7), "small": (45, 67, 60.0, 1.3, -0.7)}
FIXTURE_SIZE = "small"          # the size of the depth images stored in tests/golden/ref_tnt_cull.npz
MIN_VIEWS = (20, 3)
TRAJ = {"frames": 30, "seed": 11}


def intrinsics(size):
    H, W, f, dx, dy = SIZES[size]
    return (f, f * 1.01, (W - 1) / 2 + dx, (H - 1) / 2 + dy)


def _look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """OpenCV camera-to-world (x right, y down, z forward) at eye looking at target"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-np.asarray(up, np.float64), z)      # y is down: x = down x z, then y = z x x
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


@functools.lru_cache(maxsize=None)
def cameras():
    """OpenCV camera-to-world poses [25, 4, 4] (float32): SCENE["views"] on an arc around the object (the middle one is view 12's
    neighbourhood), then one that looks away from everything.  The arc's last camera sees only the special triangles of mesh()."""
    s = SCENE
    out = []
    for k in range(s["views"]):
        az = np.radians(s["arc_deg"]) * (2 * k / (s["views"] - 1) - 1)
        el = s["elev"] * np.sin(1.7 * k + 0.3)
        eye = s["distance"] * np.array([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el)])
        out.append(_look_at(eye, [0.03 * np.sin(k), 0.02 * np.cos(2 * k), 0.0]))
    out.append(_look_at([0.0, 0.1, -s["distance"]], [0.3, 0.2, -9.0]))
    return np.asarray(out, np.float32)


def cameras_opengl(c2w=None):
    c = np.array(cameras() if c2w is None else c2w, np.float32)
    c[:, :3, 1:3] *= -1
    return c


def _ellipsoid():
    s = SCENE
    nlat, nlon = s["nlat"], s["nlon"]
    rng = np.random.default_rng(s["jitter_seed"])
    theta = np.pi * (np.arange(nlat + 1) + 0.03) / (nlat + 0.06)
    phi = 2 * np.pi * np.arange(nlon) / nlon
    T, P = np.meshgrid(theta, phi, indexing="ij")
    r = 1 + s["bump"] * np.sin(3 * P + 0.4) * np.sin(4 * T)
    a = np.asarray(s["axes"])
    v = np.stack([a[0] * r * np.sin(T) * np.cos(P), a[1] * r * np.cos(T), a[2] * r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    # off the pixel rays: the seed is one of those at which no image has more than 0.1 % undecided pixels and no vertex is undecided
    # (tests/test_cull_cpu.py::test_scene_conditions); about one seed in ten is
    v += rng.uniform(-1e-3, 1e-3, size=v.shape)
    poles = np.array([[0.0, a[1] * 1.0005, 0.0], [0.0, -a[1] * 1.0005, 0.0]])
    idx = lambda i, j: i * nlon + (j % nlon)
    t = []
    for i in range(nlat):
        for j in range(nlon):
            t.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            t.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    n = len(v)
    for j in range(nlon):      # the pole slivers
        t.append([n, idx(0, j + 1), idx(0, j)])
        t.append([n + 1, idx(nlat, j), idx(nlat, j + 1)])
    return np.concatenate([v, poles]), np.asarray(t, np.int64)


@functools.lru_cache(maxsize=None)
def mesh(special=True):
    """(vertices [V, 3] float32, triangles [F, 3] int32, colours [V, 3] float32).  special = False: the ellipsoid, the near-plane
    triangle, the backdrop and the far triangle only — the scene the degenerate, out-of-range and NaN inputs must not change."""
    v, t = _ellipsoid()
    last = cameras()[SCENE["views"] - 1].astype(np.float64)      # the special triangles sit in front of the arc's last camera
    to_world = lambda p: (last[:3, :3] @ np.asarray(p, np.float64).T).T + last[:3, 3]
    extra_v, extra_t = [], []

    def add(tri_points):
        k = len(v) + len(extra_v)
        extra_v.extend(tri_points)
        extra_t.append([k, k + 1, k + 2])

    add(to_world([[0.002, -0.03, -0.02], [-0.012, 0.004, 0.04], [0.014, 0.008, 0.045]]))        # crosses the eye plane and the near plane
    add(to_world([[-0.12, -0.05, 0.05], [0.13, -0.055, 0.052], [0.004, 0.16, 0.051]]))          # behind it: fills that camera's screen
    add(to_world([[-60.0, -40.0, 31.0], [60.0, -41.0, 30.0], [1.0, 80.0, 32.0]]))               # beyond zfar
    if special:
        k = len(v) + len(extra_v)
        extra_v.extend([[0.0, 0.0, 0.9], [0.1, 0.1, 1.0], [0.2, 0.2, 1.1], [np.nan, 0.3, 0.2]])
        extra_t.append([k, k + 1, k + 1])                      # det = 0: a repeated vertex
        extra_t.append([k, k + 1, k + 2])                      # det = 0 up to rounding: three points on a line
        extra_t.append([0, 1, k + 400])                        # an index past the vertices
        extra_t.append([-1, 5, 6])                             # a negative index
        extra_t.append([3, k + 3, 40])                         # a NaN vertex
    verts = np.concatenate([v, np.asarray(extra_v, np.float64).reshape(-1, 3)]).astype(np.float32)
    tris = np.concatenate([t, np.asarray(extra_t, np.int64)]).astype(np.int32)
    rng = np.random.default_rng(3)
    return verts, tris, rng.uniform(0, 1, size=verts.shape).astype(np.float32)


def quad_anchor():
    """A single large quad (two triangles) in the plane n . p = d of camera space, an identity camera: z is known in closed form at every
    pixel, z = d / (n . ray).  Returns (vertices, triangles, n, d)."""
    n, d = np.array([0.21, -0.13, 1.0]), 3.0
    corners = np.array([[-40.0, -30.0], [40.0, -30.0], [40.0, 30.0], [-40.0, 30.0]])
    v = np.array([[x, y, (d - n[0] * x - n[1] * y) / n[2]] for x, y in corners], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), n, d


def transforms_json():
    """A synthetic instant-ngp style transforms.json of TRAJ["frames"] frames in shuffled order: OpenGL camera-to-world poses around a
    tilted up axis, file_path "images/frame_%05d.png" (characters 13:18 hold the 1-based frame number)."""
    rng = np.random.default_rng(TRAJ["seed"])
    n = TRAJ["frames"]
    frames = []
    for k in range(n):
        az = 2 * np.pi * k / n
        eye = np.array([3.0 * np.cos(az) + 0.7, 3.0 * np.sin(az) - 0.4, 1.2 + 0.3 * np.sin(3 * az)]) + rng.normal(0, 0.05, 3)
        c = _look_at(eye, rng.normal(0, 0.1, 3), up=(0.1, -0.15, 1.0))
        c[:3, 1:3] *= -1      # OpenGL
        frames.append({"file_path": "images/frame_%05d.png" % (k + 1), "transform_matrix": c.tolist()})
    order = rng.permutation(n)
    return {"camera_angle_x": 0.8, "frames": [frames[i] for i in order]}


def fingerprint():
    return json.dumps({"scene": SCENE, "sizes": SIZES, "fixture": FIXTURE_SIZE, "traj": TRAJ}, sort_keys=True)
