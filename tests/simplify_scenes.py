"""Fixtures of the simplification tests (SIMPLIFY.md), generated in code: a shared-vertex cube, a UV sphere with random colours, two
stacked plates with a thin slab, and the cube extended by the inputs the rules skip.  Each is the smallest size at which the kernels
can still go wrong: more than two scan tiles of 4 096 vertices, sorts that span several workgroups."""
import numpy as np

CUBE_Q = 40                      # quads per cube edge: 9 602 vertices, 19 200 triangles
CUBE_GRIDS = (2, 5, 8, 13)       # grid resolutions n (cell = longest extent / n); n = 2: eight clusters of thousands of incidences each
SPHERE_GRIDS = (5, 8, 13)
LAM = 1e-3


def cube(q=CUBE_Q):
    """(verts [V, 3] float32, tris [F, 3] int32) of the cube [-1, 1]^3: the surface points of a (q + 1)^3 lattice, every face q x q quads of
    two triangles, outward winding."""
    idx = -np.ones((q + 1,) * 3, np.int64)
    g = np.arange(q + 1)
    I, J, K = np.meshgrid(g, g, g, indexing="ij")
    surface = (I == 0) | (I == q) | (J == 0) | (J == q) | (K == 0) | (K == q)
    idx[surface] = np.arange(surface.sum())
    verts = (np.stack([I[surface], J[surface], K[surface]], 1).astype(np.float64) * (2.0 / q) - 1.0).astype(np.float32)
    tris = []
    a, b = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    for axis in range(3):
        for side in (0, q):
            def at(u, v):
                c = [None, None, None]
                c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = np.full_like(u, side), u, v
                return idx[c[0], c[1], c[2]]
            p00, p10, p11, p01 = at(a, b), at(a + 1, b), at(a + 1, b + 1), at(a, b + 1)
            quads = [np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)]      # normal along +axis
            if side == 0:
                quads = [t[:, ::-1] for t in quads]
            tris += quads
    return verts, np.concatenate(tris).astype(np.int32)


def cube_face_normals(verts, tris):
    """the axis (0..2) and the side (-1, +1) of the face every cube triangle lies in"""
    p = verts[tris].astype(np.float64)
    same = np.all(p == p[:, :1], axis=1) & (np.abs(p[:, 0]) == 1.0)
    axis = np.argmax(same, 1)
    return axis, p[np.arange(len(p)), 0, axis]


def sphere(rings=69, segments=140, seed=7):
    """(verts, tris, colors): a UV sphere of radius 1 about (0.1, -0.2, 0.3): 2 + (rings - 1) * segments = 9 522 vertices, random colours"""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    T, P = np.meshgrid(th, ph, indexing="ij")
    body = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    verts = (np.concatenate([[[0, 0, 1.0]], body, [[0, 0, -1.0]]]) + np.array([0.1, -0.2, 0.3])).astype(np.float32)
    ring = lambda r: 1 + r * segments + np.arange(segments)
    nxt = lambda x: np.roll(x, -1)
    tris = [np.stack([np.zeros(segments, np.int64), ring(0), nxt(ring(0))], 1)]
    for r in range(rings - 2):
        a, b = ring(r), ring(r + 1)
        tris += [np.stack([a, b, nxt(b)], 1), np.stack([a, nxt(b), nxt(a)], 1)]
    last = len(verts) - 1
    tris.append(np.stack([ring(rings - 2), np.full(segments, last), nxt(ring(rings - 2))], 1))
    colors = np.random.default_rng(seed).random((len(verts), 3)).astype(np.float32)
    return verts, np.concatenate(tris).astype(np.int32), colors


PLATE_Q = 16
PLATE_CELL = np.float32(0.0625)
PLATE_ORIGIN = np.array([-0.03125, -0.03125, -0.01], np.float32)


def _plate(z, flip, base):
    q = PLATE_Q
    g = np.arange(q + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X.reshape(-1) / 16.0, Y.reshape(-1) / 16.0, np.full((q + 1) ** 2, z)], 1)
    a, b = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    at = lambda u, w: base + u * (q + 1) + w
    t = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], 1), np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], 1)])
    return v, (t[:, ::-1] if flip else t)


def plates():
    """(verts, tris, info): two plates facing +z at z = 0 and z = 0.02 and a slab with its front at z = 0.5 (+z) and its back at z = 0.52
    (-z), all on the same 17 x 17 lattice of spacing 1 / 16.  With PLATE_ORIGIN and PLATE_CELL every lattice point is the centre of its
    own cell in x and y, each pair of sheets shares its cells in z: the second plate repeats the first plate's triples, the slab's back
    holds the front's triples with the opposite winding.  info: triangles per sheet."""
    parts, tris, base = [], [], 0
    for z, flip in ((0.0, False), (0.02, False), (0.5, False), (0.52, True)):
        v, t = _plate(z, flip, base)
        parts.append(v)
        tris.append(t)
        base += len(v)
    return np.concatenate(parts).astype(np.float32), np.concatenate(tris).astype(np.int32), {"sheet_tris": 2 * PLATE_Q * PLATE_Q}


def special_cube():
    """the cube with, appended last: a NaN vertex; a triangle that names it, one with the index -1, one with the index V (counted after
    the NaN vertex: outside), one that repeats an index and a zero-area one (three neighbours on an edge of the cube)"""
    v, t = cube()
    V = len(v)
    on_edge = np.nonzero((v[:, 1] == -1.0) & (v[:, 2] == -1.0))[0]
    on_edge = on_edge[np.argsort(v[on_edge, 0])][:3]
    v2 = np.concatenate([v, [[np.nan, 0.5, 0.5]]]).astype(np.float32)
    extra = np.array([[0, 1, V], [-1, 0, 1], [0, 1, V + 1], [0, 0, 1], on_edge], np.int32)
    return v2, np.concatenate([t, extra]).astype(np.int32)
