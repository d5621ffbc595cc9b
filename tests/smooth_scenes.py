"""Fixtures of the smoothing tests (SMOOTH.md), generated in code on top of the simplification's (tests/simplify_scenes.py): the cube
and the sphere with seeded noise, the cube with the inputs the rules skip, four open plates with z noise and their clustered,
non-manifold version, an open fan whose hub has 5 000 neighbours, closed fans whose hub degrees sit on both sides of the filter
kernel's row lengths (32: lane or workgroup; 256: one parked tile or two), and the empty cases.  The main ones have more than two scan
tiles of 4 096 vertices and 115 200 half-edges, so the sort spans several workgroups."""
import numpy as np

import simplify_oracle as SO
import simplify_scenes as S

SPHERE_CENTRE = np.array([0.1, -0.2, 0.3])
FAN_RIM = 5000
UMBRELLA_DEGREES = (3, 31, 32, 33, 64, 255, 256, 257, 513)


def noisy_cube(seed=5, sigma=0.004):
    v, t = S.cube()
    rng = np.random.default_rng(seed)
    return (v.astype(np.float64) + sigma * rng.standard_normal(v.shape)).astype(np.float32), t


def noisy_sphere():
    """(verts, tris, colors): every vertex moved along its radius by a relative 1 % (standard deviation), seed 11"""
    v, t, c = S.sphere()
    rng = np.random.default_rng(11)
    d = v.astype(np.float64) - SPHERE_CENTRE
    return (SPHERE_CENTRE + d * (1 + 0.01 * rng.standard_normal((len(v), 1)))).astype(np.float32), t, c


def radial_stats(verts):
    """(standard deviation, mean) of the distance to the sphere's centre, fp64"""
    r = np.linalg.norm(np.asarray(verts, np.float64) - SPHERE_CENTRE, axis=1)
    return float(r.std()), float(r.mean())


def noisy_plates(seed=9, sigma=0.003):
    v, t, _ = S.plates()
    rng = np.random.default_rng(seed)
    v = v.astype(np.float64)
    v[:, 2] += sigma * rng.standard_normal(len(v))
    return v.astype(np.float32), t


def clustered_plates():
    """the plates after the simplification's oracle: 578 vertices, 1 536 triangles, edges that four triangles share"""
    pv, pt, _ = S.plates()
    out = SO.simplify(pv, pt, S.PLATE_CELL, None, S.PLATE_ORIGIN, S.LAM)
    return out[0], out[1]


def fan(rim=FAN_RIM, seed=13):
    """hub 0 and a rim of `rim` vertices on a wavy circle, triangles (0, i, i + 1), not closed: one row of `rim` entries and a border"""
    a = 1.9 * np.pi * np.arange(rim) / rim
    rng = np.random.default_rng(seed)
    r = 1.0 + 0.05 * rng.standard_normal(rim)
    v = np.concatenate([[[0.0, 0.0, 0.2]], np.stack([r * np.cos(a), r * np.sin(a), 0.05 * rng.standard_normal(rim)], 1)])
    i = np.arange(1, rim)
    return v.astype(np.float32), np.stack([np.zeros_like(i), i, i + 1], 1).astype(np.int32)


def umbrellas(degrees=UMBRELLA_DEGREES, seed=17):
    """one closed fan per entry of `degrees`, side by side: hub degrees on both sides of every row length at which the step kernel takes
    another path.  (verts, tris, hubs)"""
    rng = np.random.default_rng(seed)
    verts, tris, hubs, base = [], [], [], 0
    for k, n in enumerate(degrees):
        a = 2 * np.pi * np.arange(n) / n
        rim = np.stack([np.cos(a) + 3.0 * k, np.sin(a), 0.1 * rng.standard_normal(n)], 1)
        verts += [[[3.0 * k, 0.0, 0.5]], rim]
        i = np.arange(n)
        tris.append(np.stack([np.full(n, base), base + 1 + i, base + 1 + (i + 1) % n], 1))
        hubs.append(base)
        base += n + 1
    return np.concatenate(verts).astype(np.float32), np.concatenate(tris).astype(np.int32), np.array(hubs)


def all_dropped():
    """V > 0 and every triangle dropped: a bad index, a repeated index or the NaN vertex in each"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    t = np.array([[0, 1, 4], [0, 0, 1], [0, 1, 3], [-1, 1, 2]], np.int32)
    return v, t


def meshes():
    """name -> (verts, tris): every fixture the adjacency is checked on"""
    sv, st, _ = noisy_sphere()
    cases = {"cube": noisy_cube(), "sphere": (sv, st), "special": S.special_cube(), "plates": noisy_plates(), "clustered": clustered_plates(),
             "fan": fan(), "umbrellas": umbrellas()[:2], "no-vertex": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
             "no-triangle": (noisy_cube()[0][:300], np.zeros((0, 3), np.int32)), "all-dropped": all_dropped()}
    # the scans' edges: 4 096 triangles are one full scan tile of keep flags and six full tiles of half-edges; one triangle is a scan of
    # one flag, and its three vertices make each sort a single pass, which leaves the sorted pairs in the second buffer pair
    cases["fan-one-tile"] = fan(rim=4097)
    cases["one-triangle"] = (noisy_cube()[0][:3], np.array([[0, 1, 2]], np.int32))
    return cases
