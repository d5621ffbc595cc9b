"""Seeded scenes of the mesh-evaluation tests (EVAL.md).  tests/golden/ref_eval.npz stores only the parameters below and what the
reference computed from the scene they generate; the inputs themselves are regenerated here."""
import numpy as np

FIXTURE = dict(subdivisions=5, radius=12.0, center=(30.0, 40.0, 50.0), gt_radius=12.35, gt_points=60000, gt_seed=7,
               bb=((10.0, 20.0, 30.0), (50.0, 60.0, 70.0)), res=0.5, obs_zero_from_x=38.0, plane=(0.0, 0.0, 1.0, -44.0))
# the two parameter sets of the fixture: the reference's defaults, and one where max_dist and the asymmetric bounding box bite
PARAMS = (dict(density=0.2, patch=60.0, max_dist=20.0), dict(density=0.2, patch=1.0, max_dist=0.4))
SEEDS = (0, 1, 2, 3, 4)
# the fixture five times as large, two subdivisions finer (327 680 triangles), 500 000 ground-truth points: what make_golden_eval.py --time and
# scripts/eval_bench.py --states sphere run
SCALED = dict(FIXTURE, radius=60.0, gt_radius=61.75, gt_points=500000, center=(150.0, 200.0, 250.0), subdivisions=7, bb=((50.0, 100.0, 150.0), (250.0, 300.0, 350.0)),
              obs_zero_from_x=190.0, plane=(0.0, 0.0, 1.0, -220.0))


def icosphere(subdivisions):
    """(vertices [V,3] float64 on the unit sphere, triangles [F,3] int32): 20 * 4^subdivisions triangles."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, g = {}, []

        def m(a, b):
            k = (a, b) if a < b else (b, a)
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v), np.array(f, np.int32)


def fixture_mesh(p=FIXTURE):
    """The icosphere plus hand-made extras: a zero-area triangle, a sliver with n = 0, an unreferenced vertex, one triangle with
    n1 = n2 = 51 reaching past the upper bounding-box margin of the second parameter set and one with n = 10 across the lower one.
    The extras sit at x >= 38 (or x < 10.3), outside the observation mask and away from the sphere: they feed no mean."""
    v, f = icosphere(p["subdivisions"])
    v = v * p["radius"] + np.array(p["center"])
    extra = np.array([(45, 32, 40), (46, 32, 40), (47, 32, 40),                       # collinear: zero area
                      (45, 30, 40), (45.3, 30, 40), (45.15, 30.00001, 40),            # sliver: thr >> both edges
                      (44, 44, 44),                                                   # unreferenced
                      (49, 36, 46), (59.3, 36, 46), (49, 46.3, 46),                   # large
                      (8.2, 40, 50), (10.3, 40, 50), (8.2, 42.1, 50)], np.float64)    # across the lower margin
    n = len(v)
    ef = np.array([(n, n + 1, n + 2), (n + 3, n + 4, n + 5), (n + 7, n + 8, n + 9), (n + 10, n + 11, n + 12)], np.int32)
    return np.concatenate([v, extra]).astype(np.float32), np.concatenate([f, ef]).astype(np.int32)


def fixture_ground_truth(p=FIXTURE):
    rng = np.random.default_rng(p["gt_seed"])
    d = rng.normal(size=(p["gt_points"], 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * p["gt_radius"] + np.array(p["center"])).astype(np.float32)


def fixture_obs(p=FIXTURE):
    """(ObsMask uint8 [X,Y,Z], BB float32 [2,3], Res float, plane float64 [4])"""
    bb = np.array(p["bb"], np.float32)
    shape = tuple(int(round((bb[1, k] - bb[0, k]) / p["res"])) + 1 for k in range(3))
    mask = np.ones(shape, np.uint8)
    mask[int(round((p["obs_zero_from_x"] - bb[0, 0]) / p["res"])):] = 0
    return mask, bb, float(p["res"]), np.array(p["plane"], np.float64)


def cluster_cloud(density, seed=3):
    """Thinning stress: 1 000 points within density / 4 of each other, a chain spaced 0.99 density in increasing input order, and
    3 000 background points a few densities apart."""
    rng = np.random.default_rng(seed)
    blob = np.array([5.0, 5.0, 5.0]) + rng.uniform(-1, 1, size=(1000, 3)) * density / (8 * 3 ** 0.5)
    chain = np.array([0.0, 1.0, 2.0]) + np.arange(200)[:, None] * np.array([0.99 * density, 0.0, 0.0])
    back = rng.uniform(0, 12 * density, size=(3000, 3)) + np.array([20.0, 10.0, 0.0])
    return np.concatenate([blob, chain, back]).astype(np.float32)


def cull_scene(W=160, H=120, focal=150.0):
    """Six views (along +-x, +-y, +-z from distance 4) of the unit ball (silhouette radius 150 / sqrt(15) = 38.7 px) with disc masks:
    radius 25 along x (they cut a ring off), 36 along y and z (wider than the silhouette once dilated by 6), the last one off centre;
    the ball's vertices are turned by a seeded rotation so that none projects onto the image's centre lines; plus 40 stray vertices
    around the cameras.
    Returns (vertices float32 [V,3], triangles int32 [F,3], intrinsics [6,4,4], poses camera-to-world [6,4,4], masks uint8 [6,H,W])."""
    v, f = icosphere(4)
    rng = np.random.default_rng(11)
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    v = np.concatenate([v @ rot.T, rng.uniform(-6, 6, size=(40, 3))]).astype(np.float32)
    K = np.array([[focal, 0, (W - 1) / 2, 0], [0, focal, (H - 1) / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    poses, masks = [], []
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(6):
        eye = np.zeros(3); eye[k // 2] = 4.0 * (1 - 2 * (k % 2))
        z = -eye / np.linalg.norm(eye)
        up = np.array([0.0, 1.0, 0.0]) if k // 2 != 1 else np.array([0.0, 0.0, 1.0])
        x = np.cross(up, z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        pose = np.eye(4); pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
        poses.append(pose)
        cx, cy = (W - 1) / 2 + (9 if k == 5 else 0), (H - 1) / 2
        disc = 25 if k < 2 else 36
        masks.append((((xx - cx) ** 2 + (yy - cy) ** 2 <= disc * disc) * 255).astype(np.uint8))
    return v, f, np.stack([K] * 6), np.stack(poses), np.stack(masks)
