"""The synthetic Tanks-and-Temples-shaped scene of the TNT tests (TNT.md §Pinning): generated from the parameters below, never stored.
A bumpy ellipsoid (not rotationally symmetric, so ICP's rotation is pinned) as the ground-truth cloud; a noisy lat-long mesh of it with
a missing cap, given in another frame (a similarity of a few degrees, scale 1.03, a shift); a concave crop polygon that cuts through the
object; a ring of cameras in both frames."""
import numpy as np

FIXTURE = {"scene": "Barn", "tau": 0.01, "axes": [0.4, 0.32, 0.24], "bump": 0.06, "center": [1.0, 0.5, 0.3], "gt_points": 120000,
           "nlat": 100, "nlon": 200, "cap": 0.25, "noise": 0.009, "rot_deg": [3.0, -2.0, 4.0], "scale": 1.03, "shift": [0.3, -0.2, 0.1],
           "cameras": 40, "camera_radius": 1.5, "camera_noise": 0.01, "seed": 3, "camera_seed": 8,
           "polygon": [[0.55, 0.1], [1.5, 0.1], [1.5, 0.45], [1.05, 0.45], [1.05, 0.9], [0.55, 0.9]], "axis_min": 0.12, "axis_max": 0.6}
# the two recorded cases: the reference's effective criteria, and a loop that runs
CASES = [{"relative_fitness": 1e-6, "relative_rmse": 20.0, "max_iteration": 30}, {"relative_fitness": 1e-6, "relative_rmse": 1e-6, "max_iteration": 30}]
RANSAC_SEED = 0


def _rot(deg):
    a, b, c = np.radians(deg)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


def similarity(rot_deg, scale, shift):
    T = np.eye(4)
    T[:3, :3] = scale * _rot(rot_deg)
    T[:3, 3] = shift
    return T


def truth(scene=FIXTURE):
    """The similarity that maps the estimate's frame onto the ground truth's."""
    return similarity(scene["rot_deg"], scene["scale"], scene["shift"])


def _surface(dirs, scene):
    """Points of the surface along unit directions [N, 3], in the ground truth's frame."""
    th, ph = np.arccos(np.clip(dirs[:, 2], -1, 1)), np.arctan2(dirs[:, 1], dirs[:, 0])
    r = 1.0 + scene["bump"] * (np.sin(3 * ph) * np.sin(2 * th) + 0.5 * np.cos(2 * ph + 1.0) * np.sin(th) ** 2 + 0.7 * np.cos(3 * th + 0.5))
    return dirs * np.asarray(scene["axes"]) * r[:, None] + np.asarray(scene["center"])


def ground_truth(scene=FIXTURE):
    n = scene["gt_points"]
    k = np.arange(n) + 0.5
    z, ph = 1 - 2 * k / n, np.pi * (1 + 5 ** 0.5) * k
    s = np.sqrt(1 - z * z)
    return _surface(np.stack([s * np.cos(ph), s * np.sin(ph), z], 1), scene).astype(np.float32)


def _apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def mesh(scene=FIXTURE):
    """(vertices [V, 3] float32, triangles [F, 3] int32) of the estimate, in its own frame: a lat-long grid without the cap around +z,
    every vertex moved along its direction by gaussian noise."""
    nlat, nlon = scene["nlat"], scene["nlon"]
    rng = np.random.default_rng(scene["seed"])
    th = np.linspace(np.pi * scene["cap"], np.pi * 0.995, nlat)
    ph = np.arange(nlon) * (2 * np.pi / nlon)
    T, P = np.meshgrid(th, ph, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    v = _surface(dirs, scene) + dirs * rng.normal(0, scene["noise"], size=(len(dirs), 1))
    i, j = np.meshgrid(np.arange(nlat - 1), np.arange(nlon), indexing="ij")
    a, b = (i * nlon + j).reshape(-1), (i * nlon + (j + 1) % nlon).reshape(-1)
    c, d = a + nlon, b + nlon
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    return _apply(np.linalg.inv(truth(scene)), v).astype(np.float32), tris


def crop_fields(scene=FIXTURE):
    """The fields of the crop JSON: orthogonal axis Z, a concave L of 6 vertices that cuts through the object."""
    return {"orthogonal_axis": "Z", "axis_min": scene["axis_min"], "axis_max": scene["axis_max"],
            "bounding_polygon": [[x, y, 0.0] for x, y in scene["polygon"]]}


def alignment(scene=FIXTURE):
    """SCENE_trans.txt: moves the COLMAP frame onto the ground truth's."""
    return similarity([10.0, 20.0, -15.0], 1.0, [0.5, 0.25, -0.4])


def cameras(scene=FIXTURE):
    """(estimated poses, COLMAP poses) [N, 4, 4] camera-to-world: a ring around the object in the ground truth's frame, seen from the
    estimate's frame (plus a little noise on the centres) and from the COLMAP frame."""
    n = scene["cameras"]
    rng = np.random.default_rng(scene["camera_seed"])
    a = np.arange(n) * (2 * np.pi / n)
    centres = np.asarray(scene["center"]) + scene["camera_radius"] * np.stack([np.cos(a), np.sin(a), 0.3 * np.sin(2 * a) + 0.2], 1)
    est, col = np.tile(np.eye(4), (n, 1, 1)), np.tile(np.eye(4), (n, 1, 1))
    est[:, :3, 3] = _apply(np.linalg.inv(truth(scene)), centres) + rng.normal(0, scene["camera_noise"], size=(n, 3))
    col[:, :3, 3] = _apply(np.linalg.inv(alignment(scene)), centres)
    return est, col


def icp_pair(scene=FIXTURE, n_source=30000, n_target=60000):
    """One ICP evaluation's inputs: (source [n_source, 3] in the estimate's frame, target [n_target, 3], both float32, the transform the
    source is moved by, the threshold 2 tau).  The source is every other point of the mesh's vertices and centroids."""
    v, t = mesh(scene)
    cloud = np.concatenate([v.astype(np.float64), v.astype(np.float64)[t].mean(axis=1)]).astype(np.float32)
    src = cloud[np.linspace(0, len(cloud) - 1, n_source).astype(np.int64)]
    return src, ground_truth(dict(scene, gt_points=n_target)), truth(scene), 2 * scene["tau"]


def crop_case(axis, n=50000, seed=11):
    """The crop test's volume (a concave 12-gon seen along `axis`) and points: n random ones, then points exactly on edges, on vertices,
    level with vertices and on axis_min / axis_max (all float32-exact)."""
    rng = np.random.default_rng(seed)
    uv = np.array([[0, 0], [4, 0], [4, 1], [1, 1], [1, 2], [3, 2], [3, 3], [1.5, 3.5], [3, 4], [0, 4], [0.5, 2.5], [-0.5, 1.25]], np.float64)
    u, v, w = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}[axis]
    poly = np.zeros((len(uv), 3))
    poly[:, u], poly[:, v] = uv[:, 0], uv[:, 1]
    fields = {"orthogonal_axis": axis, "axis_min": -0.25, "axis_max": 0.75, "bounding_polygon": poly.tolist()}
    p = np.zeros((n, 3))
    p[:, u], p[:, v], p[:, w] = rng.uniform(-1, 5, n), rng.uniform(-0.5, 4.5, n), rng.uniform(-0.5, 1.0, n)
    nxt = np.roll(uv, -1, axis=0)
    special = [uv, (uv + nxt) / 2, uv * 0.25 + nxt * 0.75]                                  # vertices, points on edges
    for du in (-0.5, 0.25, 0.5, 7.0):                                                     # level with vertices
        special.append(uv + [du, 0.0])
    sp = np.concatenate(special)
    q = np.zeros((len(sp) * 4, 3))
    q[:, u], q[:, v] = np.tile(sp[:, 0], 4), np.tile(sp[:, 1], 4)
    q[:, w] = np.repeat([0.25, -0.25, 0.75, np.float32(0.75) + np.float32(1e-7)], len(sp))      # inside, on both bounds, just outside
    return fields, np.concatenate([p, q]).astype(np.float32)


def anchor_pair(scene=FIXTURE, n_target=3000, every=3):
    """The analytic anchor: (source, target, init, truth): the source is every third target point seen from the estimate's frame, so the
    true similarity maps it onto target points exactly (up to its float32 store); init is the truth turned by 1 degree about the object's
    centre and shifted by 0.01.  The target is sparse (spacing about 0.02) so that the start lies inside the basin where every nearest
    neighbour is the true partner's; on a dense target point-to-point ICP stalls sliding along the surface."""
    tgt = ground_truth(dict(scene, gt_points=n_target))
    T = truth(scene)
    src = _apply(np.linalg.inv(T), tgt[::every].astype(np.float64)).astype(np.float32)
    c = np.asarray(scene["center"], np.float64)
    turn = similarity([0.0, 0.0, 1.0], 1.0, [0.0, 0.0, 0.0])
    turn[:3, 3] = c - turn[:3, :3] @ c + np.array([0.01, 0.0, 0.0])
    return src, tgt, turn @ T, T
