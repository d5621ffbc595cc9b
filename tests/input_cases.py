"""Input settings the parity tests otherwise never vary: scale_modifier != 1, cameras with fx != fy or an off-centre principal point,
SH stores of fewer than 16 coefficients.  No GPU import here: tests/test_inputs_cpu.py proves on the CPU that a plain-fp32 run of the
oracle meets the parity bars on every case, tests/test_gpu_inputs.py then holds the device to the same bars.

case(name, size) -> the scene_args dict of one case:

  size    scene                                                   why
  s64     make_scene(64, 40, 24, seed, px_radius=3.0)             one wave, 3 x 2 tiles, ragged right and bottom tile edges
  s300    make_scene(300, 96, 80, seed, px_radius=4.0)            four full waves and one of 44 surfels (test_gpu_preprocess_dma.py's scene)

  name                  change
  mod0.5, mod2          scale_modifier 0.5 / 2.0
  aniso1.25, aniso0.8   fy = k fx at unchanged W and H: tanfovy / k, projection matrix rebuilt
  offcentre             the scene's projection with Pm[0, 2] = 0.15, Pm[1, 2] = -0.10 (principal point ~7 % / 5 % of the frame off centre)
  M1_D0, M4_D1, M9_D2   shs[:, :M] contiguous, sh_degree D
  M9_D1, M4_D0          a store wider than the active degree: the coefficients above the degree are never read, their gradient is 0
  all                   aniso1.25 + mod2 + M4_D1
  mod0.5_M1             mod0.5 + M1_D0

The seed of a (name, size) pair is the size's default (SIZES) unless SEEDS names another one: a pair whose plain-fp32 reference misses
a bar in tests/test_inputs_cpu.py gets another seed there, never a wider bar.
"""
import math

import numpy as np

from helpers import scene_args

BG = (0.2, 0.5, 0.9)
SIZES = {"s64": dict(P=64, W=40, H=24, seed=1, px_radius=3.0),
         "s300": dict(P=300, W=96, H=80, seed=300, px_radius=4.0)}
NAMES = ("mod0.5", "mod2", "aniso1.25", "aniso0.8", "offcentre", "M1_D0", "M4_D1", "M9_D2", "M9_D1", "M4_D0", "all", "mod0.5_M1")
COMPOSED = {"all": ("aniso1.25", "mod2", "M4_D1"), "mod0.5_M1": ("mod0.5", "M1_D0")}
SEEDS = {}          # (name, size) -> seed, where the default seed's reference misses a bar of test_inputs_cpu.py
PAIRS = [(name, size) for size in SIZES for name in NAMES]
OFFCENTRE = (0.15, -0.10)
ZNEAR, ZFAR = 0.01, 100.0      # synthetic.look_at_camera's


def parts(name):
    """the elementary changes a case name stands for"""
    return COMPOSED.get(name, (name,))


def sh_shape(name):
    """(M, D) of a case: the store's coefficient count and the active degree (16, 3 unless an M* part says otherwise)"""
    for p in parts(name):
        if p[0] == "M":
            m, d = p[1:].split("_D")
            return int(m), int(d)
    return 16, 3


def modifier(name):
    for p in parts(name):
        if p.startswith("mod"):
            return float(p[3:])
    return 1.0


def _projection(a, tanfovy, centre=(0.0, 0.0)):
    import synthetic
    Pm = synthetic.projection_matrix(ZNEAR, ZFAR, 2 * math.atan(a["tanfovx"]), 2 * math.atan(tanfovy))
    Pm[0, 2], Pm[1, 2] = centre
    return np.ascontiguousarray((a["viewmatrix"].astype(np.float32) @ Pm.T).astype(np.float32))


def anisotropic(a, k):
    """fy = k fx at unchanged W, H (k = 1 reproduces the scene's own matrix bit for bit: test_inputs_cpu.py asserts it)"""
    a["tanfovy"] = float(a["tanfovy"] / k)
    a["projmatrix"] = _projection(a, a["tanfovy"])


def apply(a, name):
    """scene_args dict `a` with the changes of case `name` applied in place; returns it"""
    for p in parts(name):
        if p.startswith("mod"):
            a["scale_modifier"] = float(p[3:])
        elif p.startswith("aniso"):
            anisotropic(a, float(p[5:]))
        elif p == "offcentre":
            a["projmatrix"] = _projection(a, a["tanfovy"], OFFCENTRE)
        else:
            M, D = sh_shape(p)
            a["shs"] = np.ascontiguousarray(a["shs"][:, :M])
            a["sh_degree"] = D
    return a


def case(name, size):
    import synthetic
    assert name in NAMES, name
    s = SIZES[size]
    sc = synthetic.make_scene(s["P"], s["W"], s["H"], seed=SEEDS.get((name, size), s["seed"]), px_radius=s["px_radius"])
    sc["bg"] = np.array(BG, np.float32)
    return apply(scene_args(sc), name)


def _stress_scene(kind, seed):
    """Scenes built to break a culling rule: needle-thin, huge, grazing-angle, tiny and near-camera surfels."""
    import synthetic
    rng = np.random.default_rng(seed)
    sc = synthetic.make_scene(1500, 208, 136, seed=seed, px_radius=5.0, z_near=0.6, z_far=9.0)
    P = sc["means3D"].shape[0]
    if kind == "needles":        # 100:1 anisotropy, every orientation
        sc["scales"] = sc["scales"] * np.where(rng.random((P, 1)) < 0.5, [[12.0, 0.12]], [[0.1, 10.0]]).astype(np.float32)
    elif kind == "huge":         # footprints of hundreds of pixels, some crossing the camera plane
        sc["scales"] = sc["scales"] * rng.choice([1.0, 8.0, 40.0], size=(P, 1)).astype(np.float32)
    elif kind == "tiny":         # sub-pixel surfels: the low-pass disc carries the whole footprint
        sc["scales"] = sc["scales"] * rng.choice([0.02, 0.2, 1.0], size=(P, 1)).astype(np.float32)
    elif kind == "grazing":      # discs seen almost edge-on (normal ~ perpendicular to the view ray)
        d = sc["means3D"] - sc["campos"][None]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        t1 = np.cross(d, rng.normal(size=(P, 3))); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
        n = t1 + 0.03 * rng.normal(size=(P, 1)) * d                     # normal almost perpendicular to the ray
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        a = np.cross(n, d); a /= np.linalg.norm(a, axis=1, keepdims=True)
        b = np.cross(n, a)
        R = np.stack([a, b, n], 2)                                      # columns = disc axes, normal
        R[np.linalg.det(R) < 0, :, 0] *= -1
        w = np.sqrt(np.maximum(0, 1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2])) / 2 + 1e-9
        q = np.stack([w, (R[:, 2, 1] - R[:, 1, 2]) / (4 * w), (R[:, 0, 2] - R[:, 2, 0]) / (4 * w), (R[:, 1, 0] - R[:, 0, 1]) / (4 * w)], 1)
        sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        sc["scales"] = (sc["scales"] * 3.0).astype(np.float32)
    elif kind == "huge_faint":   # wide, nearly transparent discs close to the camera: the 3-sigma box centre runs far off screen
        sc = synthetic.make_scene(4000, 96, 64, seed=seed, px_radius=30.0, z_near=2.0, z_far=8.0)
        sc["opacities"] = np.full_like(sc["opacities"], 0.02)
    elif kind == "opaque_faint":  # opacities at both ends: 1/255-ish (empty footprints) and ~1 (widest footprints)
        sc["opacities"] = rng.choice([0.0035, 0.0045, 0.02, 0.999], size=(P, 1)).astype(np.float32)
    sc["bg"] = np.array([0.1, 0.3, 0.7], np.float32)
    return sc


STRESS_VARIANTS = ("mod2", "aniso1.25", "all")


def stress_case(kind, seed, variant):
    """scene_args of _stress_scene(kind, seed) (1500 surfels, 208 x 136) with one of STRESS_VARIANTS applied"""
    assert variant in STRESS_VARIANTS, variant
    return apply(scene_args(_stress_scene(kind, seed)), variant)
