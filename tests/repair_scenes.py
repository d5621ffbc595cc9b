"""Fixtures of the repair tests (REPAIR.md), generated in code on top of the simplification's and the smoothing's (tests/simplify_scenes.py,
tests/smooth_scenes.py): the closed cube and the inputs rule 1 drops, the noisy sphere with five kinds of hole punched into it and the
same mesh with triangle order and vertex indices permuted, the plates before and after clustering (edges in four triangles), the open
fan whose one loop is longer than any workgroup, closed fans on both sides of the wave and workgroup sizes, two umbrellas that share
their hub, and the cube with one triangle flipped or duplicated.  Each case names the caps it is run with."""
import numpy as np

import simplify_scenes as S
import smooth_scenes as M

SEGMENTS = 140      # of S.sphere()
SMALL_CUBE_Q = 6


def _sphere_tri(ring, seg, second=False):
    """the index of S.sphere()'s triangle (a, b, next b) — second: (a, next b, next a) — between rings `ring` and `ring + 1` at segment `seg`"""
    return SEGMENTS + ring * 2 * SEGMENTS + (SEGMENTS if second else 0) + seg


def punched_sphere():
    """(verts, tris, colors, loop lengths): the noisy sphere without one triangle (a loop of 3), two triangles that share an edge (4),
    the six triangles around an ordinary vertex (6), the 140 around the first pole (140), and two triangles that share one vertex only
    (after the split one loop of 6)"""
    v, t, c = M.noisy_sphere()
    gone = np.zeros(len(t), bool)
    gone[_sphere_tri(30, 50)] = True
    gone[[_sphere_tri(40, 20), _sphere_tri(40, 20, True)]] = True
    gone[(t == 1 + 20 * SEGMENTS + 10).any(1)] = True
    gone[(t == 0).any(1)] = True
    gone[[_sphere_tri(50, 100), _sphere_tri(50, 101)]] = True
    assert gone.sum() == 1 + 2 + 6 + 140 + 2
    return v, t[~gone], c, sorted([3, 4, 6, 140, 6])


def relabelled(v, t, c, seed=23):
    """the same mesh with the triangles in a seeded random order, every triangle rotated, and the vertex indices permuted"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(v))            # new index -> old index
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(v))
    t2 = inv[t[rng.permutation(len(t))]]
    rot = rng.integers(0, 3, len(t2))
    t2 = np.stack([t2[np.arange(len(t2)), (rot + k) % 3] for k in range(3)], 1)
    return v[perm], t2.astype(np.int32), None if c is None else c[perm]


def bow_tie(n0=5, n1=7):
    """two closed umbrellas of n0 and n1 triangles around the same hub, vertex 0: one vertex with two closed fans"""
    a0, a1 = 2 * np.pi * np.arange(n0) / n0, 2 * np.pi * np.arange(n1) / n1
    v = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(a0), np.sin(a0), np.full(n0, 1.0)], 1),
                        np.stack([np.cos(a1), np.sin(a1), np.full(n1, -1.0)], 1)])
    i0, i1 = np.arange(n0), np.arange(n1)
    t = np.concatenate([np.stack([np.zeros(n0, int), 1 + i0, 1 + (i0 + 1) % n0], 1),
                        np.stack([np.zeros(n1, int), 1 + n0 + (i1 + 1) % n1, 1 + n0 + i1], 1)])
    return v.astype(np.float32), t.astype(np.int32)


def flipped_cube(index=37):
    v, t = S.cube(SMALL_CUBE_Q)
    t = t.copy()
    t[index] = t[index, ::-1]
    return v, t


def duplicated_cube(index=37):
    v, t = S.cube(SMALL_CUBE_Q)
    return v, np.concatenate([t, t[index:index + 1]]).astype(np.int32)


def cases():
    """name -> (verts, tris, colors or None, the caps to run with)"""
    base = M.meshes()
    pv, pt, pc, _ = punched_sphere()
    rng = np.random.default_rng(29)
    col = lambda v: rng.random((len(v), 3)).astype(np.float32)
    uv, ut = base["umbrellas"]
    out = {
        "cube": S.cube() + (None, (32,)),
        "special": base["special"] + (None, (32,)),
        "no-vertex": base["no-vertex"] + (None, (32,)),
        "no-triangle": base["no-triangle"] + (None, (32,)),
        "all-dropped": base["all-dropped"] + (None, (32,)),
        "one-triangle": base["one-triangle"] + (None, (0, 3)),
        "punched": (pv, pt, pc, (0, 3, 4, 32, 200)),
        "relabelled": relabelled(pv, pt, pc) + ((5, 6, 200),),
        "clustered": base["clustered"] + (col(base["clustered"][0]), (32, 100)),
        "plates": base["plates"] + (None, (32, 63, 64)),
        "fan": base["fan"] + (col(base["fan"][0]), (32, 6000)),
        "fan-one-tile": base["fan-one-tile"] + (None, (4098,)),
        "umbrellas": (uv, ut, col(uv), (32, 600)),
        "bow-tie": bow_tie() + (None, (32,)),
        "flipped": flipped_cube() + (None, (5, 6)),
        "duplicated": duplicated_cube() + (None, (32,)),
    }
    return out
