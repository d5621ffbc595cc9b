"""Label images and the separable scene of the label-pass tests (tests/test_select_cpu.py, tests/test_gpu_select.py) — TEST
INFRASTRUCTURE.  The surfel scenes are those of the contribution tests (tests/contrib_scenes.py), seeds and all.

A label image is a uint8 [H, W] numpy array; 255 = unlabelled (any label >= K is ignored by the pass).
"""
import math

import numpy as np

IGNORE = 255
CUT_X = 37      # the vertical cut of `halves`: neither a multiple of 16 (tiles) nor of 4 (sub-tile rows)


def _xy(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return xs, ys


def halves(W, H, K=2):
    """label 0 left of x = 37, label 1 right of it (label 0 everywhere for K = 1)"""
    xs, _ = _xy(W, H)
    return np.where(xs < CUT_X, 0, min(1, K - 1)).astype(np.uint8)


def checker(W, H, K=2):
    """(x + y) % K: every row of 16 lanes (a 4 x 4 sub-tile) mixes labels"""
    xs, ys = _xy(W, H)
    return ((xs + ys) % K).astype(np.uint8)


def blocks4(W, H, K=2):
    """(x // 4 + y // 4) % K: every 4 x 4 sub-tile is uniform"""
    xs, ys = _xy(W, H)
    return ((xs // 4 + ys // 4) % K).astype(np.uint8)


def random(W, H, K=2, seed=0, ignored=0.1):
    """uniform in 0 .. K - 1, about 10 % of the pixels 255"""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, K, (H, W)).astype(np.uint8)
    L[rng.uniform(size=(H, W)) < ignored] = IGNORE
    return L


def constant(W, H, k):
    return np.full((H, W), k, np.uint8)


def all_ignored(W, H):
    return np.full((H, W), IGNORE, np.uint8)


PATTERNS = {"halves": halves, "checker": checker, "blocks4": blocks4, "random": lambda W, H, K: random(W, H, K, ignored=0.0)}


# ------------------------------------------------------------------------------------------------ the separable scene (end to end)
SEP_W, SEP_H, SEP_PER_CLUSTER, SEP_VIEWS = 96, 64, 60, 3


def separable_scene(view_index=0, seed=5):
    """Two clusters of 60 small tilted surfels left and right of the optical axis (|x| in 0.35 .. 1.0 at depth 3 .. 4: a gap of more
    than 20 px in a 96 x 64 frame, footprints of about 5 px), seen by a camera on the axis with a small jitter per view.  Surfel i
    belongs to cluster i // 60 (0 = left).  Returns the scene dict of tests/analytic.py's vocabulary."""
    import synthetic
    rng = np.random.default_rng(seed)
    n = SEP_PER_CLUSTER
    P = 2 * n
    side = np.repeat([-1.0, 1.0], n)
    xyz = np.stack([side * rng.uniform(0.35, 1.0, P), rng.uniform(-0.6, 0.6, P), rng.uniform(3.0, 4.0, P)], 1)
    scales = rng.uniform(0.02, 0.045, (P, 2))
    rots = np.concatenate([np.ones((P, 1)), rng.normal(0.0, 0.25, (P, 3))], 1)
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    opac = rng.uniform(0.5, 0.95, (P, 1))
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0] = rng.normal(0.0, 1.0, (P, 3))
    jitter = [(0.0, 0.0, 0.0, 0.0), (0.03, -0.02, 0.0, 0.004), (-0.03, 0.02, 0.05, -0.004)][view_index]
    a = jitter[3]
    Rcw = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    sc = dict(means3D=xyz.astype(np.float32), scales=scales.astype(np.float32), rotations=rots.astype(np.float32),
              opacities=opac.astype(np.float32), shs=shs, sh_degree=0, bg=np.zeros(3, np.float32), scale_modifier=1.0)
    sc.update(synthetic.look_at_camera(SEP_W, SEP_H, Rcw=Rcw, t=np.array(jitter[:3])))
    return sc


def separable_labels():
    """0 left of the frame's centre, 1 right of it"""
    xs, _ = _xy(SEP_W, SEP_H)
    return (xs >= SEP_W // 2).astype(np.uint8)


def separable_cluster():
    return np.repeat([0, 1], SEP_PER_CLUSTER)


def model_of(sc, device):
    """the scene's surfels as a GaussianModel (raw parameters: logit of the opacity, log of the scales)"""
    import torch
    import surfel_model
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    P = sc["means3D"].shape[0]
    m = surfel_model.GaussianModel(3, device=device)
    o = t(sc["opacities"]).reshape(P, 1)
    m.set_parameters(t(sc["means3D"]), t(sc["shs"][:, :1]), t(sc["shs"][:, 1:]), torch.log(o / (1 - o)), torch.log(t(sc["scales"])), t(sc["rotations"]))
    m.active_sh_degree = 0
    return m


def camera_of(sc, name, device):
    """the scene's camera as a surfel_render.Camera: R = camera-to-world rotation, T = world-to-camera translation of its view matrix"""
    import torch
    from surfel_render import Camera
    w2c = np.asarray(sc["viewmatrix"], np.float64).T
    W, H = int(sc["W"]), int(sc["H"])
    return Camera(colmap_id=0, R=w2c[:3, :3].T.copy(), T=w2c[:3, 3].copy(), FoVx=2 * math.atan(float(sc["tanfovx"])), FoVy=2 * math.atan(float(sc["tanfovy"])),
                  image=torch.zeros(3, H, W), image_name=name, uid=0, data_device=device)
