"""CPU checks of the mesh texturing (TEXTURE.md): the numpy restatement (tests/texture_oracle.py) against things that share nothing with
it — the atlas invariants re-derived from the texture coordinates alone, the class rule in fp64, a plate and two stacked plates in
closed form — the density search's end condition, the OBJ round trip, the library surface, and the bake kernel's resources."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import texture_oracle as O
import texture_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_texture.h"
CASES = [("ellipsoid", d) for d in S.ELLIPSOID_DENSITIES] + [("cube", d) for d in S.CUBE_DENSITIES]
_LAYOUTS = {}


def _scene(name):
    return S.ellipsoid()[:2] if name == "ellipsoid" else S.cube()


def _layout(name, density):
    if (name, density) not in _LAYOUTS:
        v, t = _scene(name)
        _LAYOUTS[name, density] = O.layout(v, t, density, S.WA)
    return _LAYOUTS[name, density]


def _patch_samples(n, step):
    """patch coordinates (du, dv) of a dense sample of the closed triangle du, dv >= 0, du + dv <= n: vertices and edge midpoints included"""
    g = np.arange(0, n + step / 2, step)
    du, dv = np.meshgrid(g, g, indexing="ij")
    keep = du + dv <= n
    return du[keep], dv[keep]


def _footprints(lay):
    """per class: (triangle ids, x [T, S, 4], y [T, S, 4]) — the four texels a bilinear fetch reads at every sample of every UV triangle,
    from the texture coordinates alone (fp64)"""
    out = {}
    for c in range(O.CLASSES):
        ids = np.nonzero(lay["cls"] == c)[0]
        if not len(ids):
            continue
        n = O.legs(c)
        du, dv = _patch_samples(n, 0.25 if n <= 16 else 0.5)
        uv = lay["uv"][ids].astype(np.float64)
        k = lay["tri"]["corner"][ids]
        rows = np.arange(len(ids))
        A, B, C = uv[rows, k], uv[rows, (k + 1) % 3], uv[rows, (k + 2) % 3]
        P = A[:, None] + (du / n)[None, :, None] * (B - A)[:, None] + (dv / n)[None, :, None] * (C - A)[:, None]
        x0, y0 = np.floor(P[..., 0]).astype(np.int64), np.floor(P[..., 1]).astype(np.int64)
        out[c] = (ids, np.stack([x0, x0 + 1, x0, x0 + 1], -1), np.stack([y0, y0, y0 + 1, y0 + 1], -1))
    return out


# ------------------------------------------------------------------------------------------------ the layout's invariants
@pytest.mark.parametrize("name,density", CASES)
def test_layout_invariants(name, density):
    v, t = _scene(name)
    lay = _layout(name, density)
    Wa, Ha = lay["Wa"], lay["Ha"]
    tri, _, _, _ = O.owners(lay)
    touched = -np.ones((Ha, Wa), np.int64)
    for c, (ids, xs, ys) in _footprints(lay).items():
        # every texel a fetch reads lies inside the atlas ...
        assert xs.min() >= 0 and ys.min() >= 0 and xs.max() < Wa and ys.max() < Ha, (c, xs.min(), xs.max(), ys.min(), ys.max())
        # ... belongs to the triangle by the analytic owner rule ...
        assert np.array_equal(tri[ys, xs], np.broadcast_to(ids[:, None, None], xs.shape)), c
        # ... and to no other triangle's footprint (from the texture coordinates alone)
        who = np.broadcast_to(ids[:, None, None], xs.shape)
        before = touched[ys, xs]
        assert ((before == -1) | (before == who)).all(), c
        touched[ys, xs] = who
    assert ((touched == -1) | (touched == tri)).all()
    # every triangle with a patch owns exactly its half of a cell: (n + 3)(n + 4) / 2 texels below the diagonal, the rest above
    owned_by = np.bincount(tri[tri >= 0], minlength=len(t))
    for c in range(O.CLASSES):
        ids = np.nonzero(lay["cls"] == c)[0]
        n = O.legs(c)
        lower = (n + 3) * (n + 4) // 2                     # x + y <= n + 2
        upper = (n + 4) ** 2 - lower
        assert set(owned_by[ids]) <= {lower, upper}, c
        assert (owned_by[ids] == lower).sum() == (len(ids) + 1) // 2
    assert (owned_by[lay["cls"] < 0] == 0).all() and (lay["uv"][lay["cls"] < 0] == 0).all()
    print("%s at %g: classes %s, atlas %d x %d, %.1f %% owned" % (name, density, lay["counts"], Wa, Ha, 100.0 * (tri >= 0).mean()))


def test_the_densities_use_four_classes_both_clamps_an_odd_count_and_a_partial_row():
    v, t = _scene("ellipsoid")
    used = set()
    for d in S.ELLIPSOID_DENSITIES:
        lay = _layout("ellipsoid", d)
        used |= {c for c in range(O.CLASSES) if lay["counts"][c]}
    assert len(used) >= 4 and 0 in used and 5 in used
    lay = _layout("ellipsoid", S.ELLIPSOID_DENSITIES[0])
    p = v[np.where(lay["tri"]["ok"][:, None], t, 0)].astype(np.float64)
    L = np.sqrt(np.maximum.reduce([((p[:, a] - p[:, b]) ** 2).sum(1) for a, b in ((0, 1), (1, 2), (2, 0))]))
    s = L[lay["tri"]["ok"]] * S.ELLIPSOID_DENSITIES[0]
    assert s.min() < 4 and s.max() > 128                   # both clamps are live
    odd = partial = False
    for name, d in CASES:
        lay = _layout(name, d)
        tri = O.owners(lay)[0]
        for c in range(O.CLASSES):
            y0, per, first, count = (int(x) for x in lay["table"][c])
            if not count:
                continue
            cells, cell = (count + 1) // 2, O.legs(c) + O.PAD
            if count % 2:      # the last cell's upper half stays empty
                odd = True
                row, col = (cells - 1) // per, (cells - 1) % per
                block = tri[y0 + row * cell:y0 + (row + 1) * cell, col * cell:(col + 1) * cell]
                assert (block >= 0).sum() == (O.legs(c) + 3) * (O.legs(c) + 4) // 2 and len(set(block[block >= 0])) == 1
            if cells % per:    # the rest of the last row stays empty
                partial = True
                row = cells // per
                assert (tri[y0 + row * cell:y0 + (row + 1) * cell, (cells % per) * cell:] == -1).all()
    assert odd and partial


@pytest.mark.parametrize("name,density", CASES)
def test_class_rank_and_corner_rules(name, density):
    v, t = _scene(name)
    lay = _layout(name, density)
    ok = lay["cls"] >= 0
    # the skips: an index outside the vertices, a non-finite coordinate, a zero cross product
    inside = ((t >= 0) & (t < len(v))).all(1)
    p = v[np.where(inside[:, None], t, 0)].astype(np.float64)
    with np.errstate(invalid="ignore"):
        cross = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        want_ok = inside & np.isfinite(p).all((1, 2)) & (np.linalg.norm(cross, axis=1) > 1e-12)
    assert np.array_equal(ok, want_ok)
    # the class against an fp64 log2, away from the powers of two
    e = np.stack([np.linalg.norm(p[:, 2] - p[:, 1], axis=1), np.linalg.norm(p[:, 0] - p[:, 2], axis=1), np.linalg.norm(p[:, 1] - p[:, 0], axis=1)], 1)
    s = e.max(1)[ok] * np.float64(np.float32(density))
    k = np.clip(np.ceil(np.log2(s)), 2, 7)
    clear = np.abs(s / 2.0 ** np.round(np.log2(s)) - 1) > 1e-5
    assert clear.mean() > 0.99 and np.array_equal(lay["cls"][ok][clear] + 2, k[clear].astype(np.int64))
    # the right angle lies opposite the longest edge; among equal edges at the lowest corner
    srt = np.sort(e, 1)
    tie = (srt[:, 2] - srt[:, 1]) <= 1e-6 * srt[:, 2]
    sure = ok & ~tie
    assert np.array_equal(lay["tri"]["corner"][sure], e.argmax(1)[sure])
    exact = ok & (e[:, 0] == e[:, 1]) & (e[:, 1] == e[:, 2])
    assert (lay["tri"]["corner"][exact] == 0).all()
    # within a class the rank is the triangle order: rank r sits in cell r / 2, half r % 2, cells row-major
    for c in range(O.CLASSES):
        ids = np.nonzero(lay["cls"] == c)[0]
        if not len(ids):
            continue
        y0, per, first, count = (int(x) for x in lay["table"][c])
        n, cell = O.legs(c), O.legs(c) + O.PAD
        assert count == len(ids) and per == S.WA // cell
        uv = lay["uv"][ids].astype(np.float64)
        rows = np.arange(len(ids))
        k = lay["tri"]["corner"][ids]
        A, B, C = uv[rows, k], uv[rows, (k + 1) % 3], uv[rows, (k + 2) % 3]
        half = (B[:, 0] < A[:, 0]).astype(np.int64)
        origin = A - np.where(half[:, None] == 1, cell - 2, 0)
        assert (origin % cell == [0, y0 % cell]).all()
        rank = 2 * (((origin[:, 1] - y0) // cell) * per + origin[:, 0] // cell) + half
        assert np.array_equal(rank, rows)
        # right isosceles, legs of n texels along the axes, every triangle with the same orientation
        assert np.array_equal(B - A, np.where(half[:, None] == 1, [-n, 0], [n, 0])) and np.array_equal(C - A, np.where(half[:, None] == 1, [0, -n], [0, n]))
        assert np.array_equal(lay["order"][first:first + count], ids)
    # bands: largest class first, one below the other
    y = 0
    for c in range(O.CLASSES - 1, -1, -1):
        y0, per, first, count = (int(x) for x in lay["table"][c])
        assert y0 == y
        if count:
            y += -(-((count + 1) // 2) // per) * (O.legs(c) + O.PAD)
    assert lay["Ha"] == max(y, 1)


def test_limits_of_the_layout():
    v, t = _scene("ellipsoid")
    with pytest.raises(O.LimitError):
        O.layout(v, t, 40.0, 100)            # the far triangle's cell (132) does not fit
    vc, tc = S.cube()
    with pytest.raises(O.LimitError):
        O.layout(vc, tc, 1e6, S.WA)          # 9 600 cells of 132 texels, 7 per row
    lay = O.layout(v, np.zeros((0, 3), np.int32), 40.0, S.WA)
    assert lay["Ha"] == 1 and lay["counts"] == [0] * 6 and (O.owners(lay)[0] == -1).all()


# ------------------------------------------------------------------------------------------------ the density search
@pytest.mark.parametrize("size", [256, 700, 2048])
def test_bisection_meets_its_condition(size):
    sys.path.insert(0, PKG)
    import surfel_texture as P
    v, t = S.ellipsoid(False)[:2]
    t = t[:-1]                                                 # without the triangle beyond zfar, whose cell alone is 132 texels wide
    probe = lambda d: O.classify(v, t, d)[1]
    density, counts, probes, above = P.bisect_density(probe, size, start=size / 2.0)
    print("size %d: density %.6g (next candidate %.6g) after %d probes, height %d" % (size, density, above, probes, O.band_table(counts, size)[1]))
    assert probes <= P.MAX_PROBES and counts == probe(density) and np.float32(density) == density
    assert above is not None and O.bisect_ok(probe, size, density, above)
    assert above / density < 1.001                             # the bracket closed: the candidates are fp32 neighbours or nearly so
    for start in (1e-3, 1e5):                                  # from far below and far above: the same condition
        d2, _, p2, a2 = P.bisect_density(probe, size, start=start)
        assert p2 <= P.MAX_PROBES and O.bisect_ok(probe, size, d2, a2)
    # the host's band table is the restatement's
    for c in ([0, 0, 0, 0, 0, 0], [5, 0, 3, 0, 0, 1], counts):
        tab, Ha = P.band_table(c, size)
        assert np.array_equal(tab, O.band_table(c, size)[0]) and Ha == O.band_table(c, size)[1]
    with pytest.raises(P.MeshLimitError):
        P.bisect_density(lambda d: [10 ** 7, 0, 0, 0, 0, 0], 64)
    assert P.bisect_density(lambda d: [0, 0, 0, 0, 0, 3], 512)[3] is None      # every patch at the largest class: nothing above


# ------------------------------------------------------------------------------------------------ closed forms
def _texel_geometry(lay, verts, tris):
    """From the texture coordinates alone (fp64): per owned texel strictly inside its UV triangle the triangle and the 3D point."""
    Ha, Wa = lay["Ha"], lay["Wa"]
    tri_of = -np.ones((Ha, Wa), np.int64)
    point = np.zeros((Ha, Wa, 3))
    v = np.asarray(verts, np.float64)
    for f in np.nonzero(lay["cls"] >= 0)[0]:
        q = lay["uv"][f].astype(np.float64)
        M = np.array([q[1] - q[0], q[2] - q[0]]).T
        lo, hi = np.floor(q.min(0)).astype(int), np.ceil(q.max(0)).astype(int)
        xs, ys = np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1))
        l12 = np.linalg.solve(M, np.stack([xs.reshape(-1) - q[0, 0], ys.reshape(-1) - q[0, 1]]))
        l = np.stack([1 - l12[0] - l12[1], l12[0], l12[1]])
        inside = (l >= -1e-9).all(0)
        x, y = xs.reshape(-1)[inside], ys.reshape(-1)[inside]
        assert (tri_of[y, x] == -1).all()
        tri_of[y, x] = f
        point[y, x] = (l[:, inside].T[:, :, None] * v[tris[f]][None]).sum(1)
    return tri_of, point


@pytest.fixture(scope="module")
def plate_run():
    v, t = S.plate()
    w2c, intr, H, W = S.plate_cameras()
    lay = O.layout(v, t, S.PLATE_DENSITY, 256)
    depth = S.depth_images(v, t, w2c, intr, H, W)
    return v, t, w2c, intr, H, W, lay, depth


def _plate_weights(point, w2c, power):
    """fp64 weights [5, ...] of points on the plate z = 0 (normal +-z): c^power / z^2 from the geometry"""
    out = []
    for m in np.asarray(w2c, np.float64):
        R, tr = m[:3, :3], m[:3, 3]
        o = -R.T @ tr
        d = point - o
        dist = np.linalg.norm(d, axis=-1)
        c = np.abs(d[..., 2]) / dist
        z = d @ R[2]
        out.append(c ** power / z ** 2)
    return np.stack(out)


@pytest.mark.parametrize("power", [1, 2])
def test_plate_in_closed_form(plate_run, power):
    v, t, w2c, intr, H, W, lay, depth = plate_run
    assert len(t) == 2 * S.PLATE_Q ** 2 and set(lay["cls"]) == {2}
    images = np.broadcast_to(S.PLATE_COLORS[:, :, None, None], (5, 3, H, W)).astype(np.float32)
    acc = O.bake(lay, np.zeros((lay["Ha"], lay["Wa"], 4), np.float32), w2c, intr, depth, images, S.EPS, 0.1, power, O.AVERAGE)
    atlas, colour, owned, seen = O.resolve(lay, acc, None, O.AVERAGE)
    tri_of, point = _texel_geometry(lay, v, t)
    # two pixel footprints, by geometry alone: a pixel at the plate is |p - o| / (f cos) wide at most
    eyes = np.array([-m[:3, :3].T @ m[:3, 3] for m in np.asarray(w2c, np.float64)])
    far = max(np.linalg.norm(np.array([sx * 0.5, sy * 0.5, 0.0]) - e) ** 2 / abs(e[2]) for e in eyes for sx in (-1, 1) for sy in (-1, 1)) / S.PLATE_SIZE[2]
    inner = (tri_of >= 0) & (np.abs(point[..., :2]).max(-1) < S.PLATE_HALF - 2 * far)
    assert inner.sum() > 2000, (inner.sum(), far)
    w = _plate_weights(point[inner], w2c, power)
    want = (w[:, :, None] * S.PLATE_COLORS.astype(np.float64)[:, None, :]).sum(0) / w.sum(0)[:, None]
    err = np.abs(colour[inner].astype(np.float64) - want).max()
    werr = np.abs(acc[inner][:, 3] / w.sum(0) - 1).max()
    print("power %d: %d interior texels (margin %.3f), colour off by %.2e, the weight sum by %.2e relative" % (power, inner.sum(), 2 * far, err, werr))
    assert (acc[inner][:, 3] > 0).all()
    assert err <= 1e-4 and werr <= 1e-4


def test_plate_of_one_colour(plate_run):
    v, t, w2c, intr, H, W, lay, depth = plate_run
    colour = np.array([0.3, 0.6, 0.9], np.float32)
    images = np.broadcast_to(colour[None, :, None, None], (5, 3, H, W)).astype(np.float32)
    for blend in (O.AVERAGE, O.BEST):
        acc = O.bake(lay, np.zeros((lay["Ha"], lay["Wa"], 4), np.float32), w2c, intr, depth, images, S.EPS, 0.1, 2, blend)
        atlas = O.resolve(lay, acc, None, blend)[0]
        # every texel (gutters included) of a triangle whose corners lie well inside the outline
        tri, _, _, _ = O.owners(lay)
        well = (np.abs(v[t][..., :2]).max((1, 2)) < S.PLATE_HALF - 0.15)
        sel = (tri >= 0) & well[np.maximum(tri, 0)]
        assert sel.sum() > 2000
        code = (colour.astype(np.float64) * 255)
        assert np.abs(atlas[sel].astype(np.float64) - np.floor(code)).max() <= 1


def test_rear_plate_falls_back_to_its_vertex_colours():
    v, t, c, first_rear = S.two_plates()
    w2c, intr, H, W = S.plate_cameras()
    w2c = w2c[:1]
    lay = O.layout(v, t, S.PLATE_DENSITY, 256)
    depth = S.depth_images(v, t, w2c, intr, H, W)
    images = np.full((1, 3, H, W), 1.0, np.float32)
    acc = O.bake(lay, np.zeros((lay["Ha"], lay["Wa"], 4), np.float32), w2c, intr, depth, images, S.EPS, 0.1, 2, O.AVERAGE)
    atlas, _, owned, seen = O.resolve(lay, acc, c, O.AVERAGE)
    tri_of, point = _texel_geometry(lay, v, t)
    rear = (tri_of >= first_rear) & (np.abs(point[..., :2]).max(-1) < S.PLATE_HALF - 0.1)
    front = (tri_of >= 0) & (tri_of < first_rear) & (np.abs(point[..., :2]).max(-1) < S.PLATE_HALF - 0.1)
    assert rear.sum() > 2000 and front.sum() > 2000
    assert (acc[rear][:, 3] == 0).all() and (acc[front][:, 3] > 0).all()
    want = np.floor(np.clip(point[rear] @ S.PLATE_A.T + S.PLATE_B, 0, 1) * 255)
    assert np.abs(atlas[rear].astype(np.float64) - want).max() <= 1
    assert (atlas[front] >= 254).all() and 0 < seen < owned      # (w 1) / w may round to the fp32 below 1: one code
    grey = O.resolve(lay, acc, None, O.AVERAGE)[0]
    assert (grey[rear] == int(np.float32(0.8) * np.float32(255))).all()


# ------------------------------------------------------------------------------------------------ files
def test_obj_round_trip(tmp_path):
    sys.path.insert(0, PKG)
    import surfel_io
    v, t = S.plate()
    lay = O.layout(v, t, S.PLATE_DENSITY, 256)
    vt = np.stack([(lay["uv"][..., 0] + 0.5) / lay["Wa"], 1 - (lay["uv"][..., 1] + 0.5) / lay["Ha"]], -1).astype(np.float32)
    path = str(tmp_path / "plate.obj")
    surfel_io.write_obj(path, v, t, vt, texture="plate.png")
    text = open(path).read().split("\n")
    assert text[0] == "mtllib plate.mtl" and sum(l.startswith("vt ") for l in text) == 3 * len(t) and sum(l.startswith("v ") for l in text) == len(v)
    assert "f 1/1 14/2 15/3" in text and "map_Kd plate.png" in open(str(tmp_path / "plate.mtl")).read()
    v2, t2, vt2, tex = surfel_io.read_obj(path)
    assert np.array_equal(v2, v) and np.array_equal(t2, t) and t2.dtype == np.int32 and tex == "plate.png"
    assert np.array_equal(vt2, vt) and vt2.min() >= 0 and vt2.max() <= 1
    plain = str(tmp_path / "plain.obj")
    surfel_io.write_obj(plain, v, t)
    v3, t3, vt3, tex3 = surfel_io.read_obj(plain)
    assert np.array_equal(v3, v) and np.array_equal(t3, t) and vt3 is None and tex3 is None
    with open(plain, "w") as fh:
        fh.write("# by hand\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\nf -3/-3/1 -2/-2/1 -1/-1/1\n")
    v4, t4, vt4, _ = surfel_io.read_obj(plain)
    assert np.array_equal(t4, [[0, 1, 2]]) and np.array_equal(vt4[0], [[0, 0], [1, 0], [0, 1]])


# ------------------------------------------------------------------------------------------------ library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_texture_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", hdr, re.M)
    assert len(decl) == 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.TEXTURE_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    others = [name for h, group in surfel_native.SIGNATURES.items() if h != HEADER for name in group]
    assert not set(decl) & set(others)
    lib = surfel_native.load()
    for name in surfel_native.TEXTURE_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
    assert surfel_native.call(None, "surfel_abi_version") == 1
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_texture", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "mesh_texture.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["mesh_texture.hip"] and any(h.endswith(HEADER) for h in mod.HEADERS)
    import surfel_texture as P
    for name, value in (("CLASSES", P.CLASSES), ("MIN_LOG2", P.MIN_LOG2), ("PAD", P.PAD), ("MAX_SIDE", P.MAX_SIDE), ("BAND_INTS", P.BAND_INTS),
                        ("AVERAGE", P.BLENDS["average"]), ("BEST", P.BLENDS["best"]), ("MAX_POWER", P.MAX_POWER)):
        assert int(re.search(r"#define SURFEL_TEXTURE_%s (\d+)" % name, hdr).group(1)) == value, name
    assert (P.CLASSES, P.MIN_LOG2, P.PAD, P.MAX_SIDE, P.BLENDS["average"], P.BLENDS["best"]) == (O.CLASSES, O.MIN_LOG2, O.PAD, O.MAX_SIDE, O.AVERAGE, O.BEST)
    assert P.EPS == S.EPS and P.GREY == O.GREY


def test_texture_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_texture.h."""
    import ctypes as C
    sys.path.insert(0, PKG)
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 5
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES[HEADER])
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is returns[ret], (name, ret, fn.restype)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            else:
                assert ctype.endswith("*"), where
                assert at in (n.DevPtr, n.Stream, C.c_void_p) or issubclass(at, C._Pointer), where
                host = pname in ("counts", "table", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_arguments_and_limits_are_refused_before_a_device_is_touched():
    import ctypes as C
    sys.path.insert(0, PKG)
    import surfel_native as n
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    p = C.c_void_p(256)
    counts = (C.c_int64 * 6)(0, 0, 0, 0, 0, 1)
    table = (C.c_int * 24)(*([7] * 24))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # density 0
        n.call(None, "surfel_texture_classify", cb, None, 3, 1, p, p, 0.0, p, counts)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*narrower than a cell"):
        n.call(None, "surfel_texture_layout", cb, None, 3, 1, p, p, p, counts, 100, table, p, p)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*wider"):
        n.call(None, "surfel_texture_layout", cb, None, 3, 1, p, p, p, counts, 16385, table, p, p)
    many = (C.c_int64 * 6)(0, 0, 0, 0, 0, 2000)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*higher"):             # 1 000 cells of 132 texels, 7 per row: 18 876 rows
        n.call(None, "surfel_texture_layout", cb, None, 3, 2000, p, p, p, many, 1000, table, p, p)
    assert list(table) == [7] * 24 and not taken
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # power 9
        n.call(None, "surfel_texture_bake", 3, 1, p, p, table, p, 1000, 132, 1, p, p, 1, 45, 67, p, p, 0.005, 0.1, 9, 0, p)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*band table"):         # a table of sevens describes no atlas
        n.call(None, "surfel_texture_bake", 3, 1, p, p, table, p, 1000, 132, 1, p, p, 1, 45, 67, p, p, 0.005, 0.1, 2, 0, p)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*SURFEL_TEXTURE_MAX_SIDE"):
        n.call(None, "surfel_texture_resolve", 3, 1, p, p, None, table, p, 16385, 132, p, 0, 0.0, 0.0, 0.0, p, p)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # ssaa 5
        n.call(None, "surfel_texture_shade", 3, 1, p, p, p, p, 64, 64, 1, p, p, 1, 45, 67, 5, p, 1.0, 1.0, 1.0, p)


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    sys.path.insert(0, PKG)
    import torch
    import surfel_texture as P
    import surfel_meshview as MV
    import surfel_mesh
    import surfel_view as SV
    from surfel_mesh import TriangleMesh
    mesh = TriangleMesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.classify(mesh, 10.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.atlas_layout(mesh, density=10.0)
    with pytest.raises(ValueError, match="density or atlas_size"):
        P.atlas_layout(mesh)
    with pytest.raises(ValueError, match="density or atlas_size"):
        P.atlas_layout(mesh, density=1.0, atlas_size=64)
    with pytest.raises(ValueError, match="needs texture="):
        MV.render_mesh(mesh, [], mode="textured")
    with pytest.raises(ValueError, match="shaded, normal, color, depth, textured"):
        MV.render_mesh(mesh, [], mode="wireframe")
    uv = torch.tensor([[[0.0, 0.0], [3.0, 1.0]]])
    assert torch.equal(P.obj_uv(uv, 4, 2), torch.tensor([[[0.125, 0.75], [0.875, 0.25]]]))
    a = surfel_mesh.build_parser().parse_args(["-m", "x"])
    assert not a.texture and a.atlas_size == 4096
    a = surfel_mesh.build_parser().parse_args(["-m", "x", "--texture", "--atlas_size", "512", "--simplify_faces", "100"])
    assert a.texture and a.atlas_size == 512
    a = P.build_parser().parse_args(["--ply-path", "m.ply", "-m", "model"])
    assert (a.source, a.atlas_size, a.density, a.blend, a.png, a.power, a.cos_min) == ("render", 4096, None, "average", "pillow", 2, 0.1)
    a = P.build_parser().parse_args(["--ply-path", "m.ply", "-m", "model", "-s", "cap", "--source", "gt", "--density", "50", "--blend", "best", "--png", "device"])
    assert (a.source, a.source_path, a.density, a.blend, a.png) == ("gt", "cap", 50.0, "best", "device")
    with pytest.raises(SystemExit, match="needs -s"):
        P.main(["--ply-path", "m.ply", "-m", "model", "--source", "gt"])
    a = MV.build_parser().parse_args(["--ply-path", "m.obj", "-m", "x", "--mesh_modes", "textured", "shaded"])
    assert a.mesh_modes == ["textured", "shaded"]
    assert list(SV.TEXTURE_ITEMS) == ["Mesh Textured"] and SV.TEXTURE_ITEMS["Mesh Textured"] == MV.TEXTURED


# ------------------------------------------------------------------------------------------------ kernel resources
def test_bake_kernel_has_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("mesh_texture.hip"))
    names = [k for k in ks if "texture_" in k]
    assert len(names) == 6, names
    for k in names:
        md = ks[k][1]
        print("%s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (isa_count.demangle(k).split("(")[0], md.get("next_free_vgpr", 0), md.get("next_free_sgpr", 0),
                                                                   md.get("group_segment_fixed_size", 0), md.get("private_segment_fixed_size", 0)))
        assert int(md.get("private_segment_fixed_size", 0)) == 0, k
        assert md.get("group_segment_fixed_size", 0) == 0, k
    bake = [k for k in names if "texture_bake_kernel" in k]
    assert len(bake) == 1 and ks[bake[0]][1].get("next_free_vgpr", 0) <= 64      # 8 waves per SIMD
