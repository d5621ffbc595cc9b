"""Scenes of the texturing tests (TEXTURE.md), generated in code from what the suite already builds: the ellipsoid of cull_scenes with
its special triangles and 24 + 1 views at the small image size, the cube of simplify_scenes (layout only), and two closed-form scenes —
a plate of 12 x 12 quads under five cameras, and two parallel plates 0.2 apart under one camera."""
import functools

import numpy as np

import cull_oracle as CO
import cull_scenes as CS
import simplify_scenes as SS

WA = 1000                              # a multiple of no cell side (8, 12, 20, 36, 68, 132)
ELLIPSOID_DENSITIES = (40.0, 200.0)    # 40: classes 0, 1, 2 and 5 with both clamps live; 200: the middle classes
CUBE_DENSITIES = (60.0, 150.0)         # every cube triangle's longest edge is a quad's diagonal: one class of 19 200 (28 scan tiles of 6 F)
BAKE_DENSITY, BAKE_WA = 40.0, 400      # the bake comparisons: about 10^5 owned texels
SIZE = "small"                         # 45 x 67
VIEWS, BATCH = 24, 7
ZNEAR, ZFAR, EPS = CS.SCENE["znear"], CS.SCENE["zfar"], CS.SCENE["eps"]


@functools.lru_cache(maxsize=None)
def ellipsoid(special=True):
    """(verts, tris, colors, w2c [25, 4, 4] fp32, intrinsics, H, W)"""
    v, t, c = CS.mesh(special)
    H, W = CS.SIZES[SIZE][:2]
    return v, t, c, CO.world_to_camera(CS.cameras()), CS.intrinsics(SIZE), H, W


def cube():
    return SS.special_cube()


@functools.lru_cache(maxsize=None)
def noise_images(n=VIEWS, seed=5):
    H, W = CS.SIZES[SIZE][:2]
    return np.random.default_rng(seed).random((n, 3, H, W)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ closed forms
PLATE_Q = 12
PLATE_HALF = 0.5
PLATE_DENSITY = 100.0                  # the quad's diagonal 0.118 -> 11.8 texels -> legs of 16
PLATE_SIZE = (60, 80, 70.0)            # H, W, f
PLATE_COLORS = np.array([[0.9, 0.1, 0.2], [0.2, 0.8, 0.3], [0.1, 0.3, 0.95], [0.7, 0.7, 0.1], [0.4, 0.2, 0.6]], np.float32)
# eye (in front of the plate: z < 0) and target on the plate, per camera
PLATE_EYES = np.array([[0.0, 0.0, -2.0], [0.6, 0.2, -1.7], [-0.5, 0.4, -2.4], [0.3, -0.7, -1.5], [-0.8, -0.3, -2.1]])
PLATE_TARGETS = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, -0.05, 0.0], [-0.04, 0.03, 0.0], [0.02, 0.02, 0.0]])
PLATE_A = np.array([[0.3, 0.1, 0.0], [-0.2, 0.25, 0.0], [0.1, -0.3, 0.5]])      # the affine vertex colours c = A p + b of the plates
PLATE_B = np.array([0.5, 0.45, 0.4])


def plate(z=0.0, q=PLATE_Q, half=PLATE_HALF):
    """(verts [(q + 1)^2, 3] float32, tris [2 q^2, 3] int32) of the square [-half, half]^2 at height z"""
    g = np.linspace(-half, half, q + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X.reshape(-1), Y.reshape(-1), np.full((q + 1) ** 2, z)], 1).astype(np.float32)
    a, b = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    at = lambda i, j: i * (q + 1) + j
    t = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], 1), np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], 1)])
    return v, t.astype(np.int32)


def plate_cameras():
    """(w2c [5, 4, 4] fp32, intrinsics, H, W)"""
    H, W, f = PLATE_SIZE
    c2w = np.asarray([CS._look_at(e, t) for e, t in zip(PLATE_EYES, PLATE_TARGETS)], np.float32)
    return CO.world_to_camera(c2w), (f, f, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2), H, W


def two_plates():
    """(verts, tris, colors, rear: the first triangle of the rear plate): the front plate at z = 0, the rear one at z = 0.2, affine
    vertex colours; the camera of plate_cameras()[0] looks at them square on from z = -2"""
    v0, t0 = plate(0.0)
    v1, t1 = plate(0.2)
    v = np.concatenate([v0, v1])
    t = np.concatenate([t0, t1 + len(v0)]).astype(np.int32)
    return v, t, affine_colors(v), len(t0)


def affine_colors(verts):
    return (np.asarray(verts, np.float64) @ PLATE_A.T + PLATE_B).astype(np.float32)


def depth_images(verts, tris, w2c, intr, H, W, znear=ZNEAR, zfar=ZFAR):
    """the fp32 twin of the depth oracle for every view: what a device without a depth image of its own bakes against on the CPU"""
    return np.stack([CO.depth_image(verts, tris, m, intr, H, W, znear, zfar, np.float32)[0] for m in w2c]).astype(np.float32)
