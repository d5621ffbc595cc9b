"""CPU checks of the mesh simplification (SIMPLIFY.md): the numpy restatement (tests/simplify_oracle.py) against closed forms that
share nothing with it — the corner of a cube, its flat faces, the movement bound, a grid finer than every edge, the duplicate rule on
stacked plates, the inputs the rules skip, the bisection's condition — and the library surface (header, exports, signatures)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import simplify_oracle as O
import simplify_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_simplify.h"


@pytest.fixture(scope="module")
def cube():
    return S.cube()


@pytest.fixture(scope="module")
def cube_results(cube):
    v, t = cube
    return {n: O.simplify(v, t, O.grid_cell(v, n), lam=S.LAM, full=True) for n in S.CUBE_GRIDS}


def test_fixture_sizes(cube):
    v, t = cube
    assert v.shape == (9602, 3) and t.shape == (19200, 3) and v.dtype == np.float32 and t.dtype == np.int32
    assert len(v) > 2 * 4096      # more than two scan tiles
    p = v[t].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.all((n * p.mean(1)).sum(1) > 0)      # outward winding
    axis, side = S.cube_face_normals(v, t)
    assert np.array_equal(np.sign(n[np.arange(len(n)), axis]), side)
    sv, st, sc = S.sphere()
    assert 9000 < len(sv) < 10000 and st.min() == 0 and st.max() == len(sv) - 1 and sc.shape == sv.shape
    q = sv[st].astype(np.float64)
    centre = np.array([0.1, -0.2, 0.3])
    assert np.all((np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]) * (q.mean(1) - centre)).sum(1) > 0)


@pytest.mark.parametrize("n,left", [(5, 192), (8, 588), (13, 1728)])
def test_cube_corner_is_kept(cube, cube_results, n, left):
    """Three orthogonal planes of equal weight through the corner c, the mean m in the same cell: (A + mu I) x = b + mu m with A = w I,
    mu = 3 lam w gives x - c = 3 lam / (1 + 3 lam) (m - c), and |m - c| < cell in every coordinate."""
    v, t = cube
    verts, tris, _, cluster, stats, full = cube_results[n]
    cell = float(O.grid_cell(v, n))
    corner = int(np.nonzero((v == 1.0).all(1))[0][0])
    c = cluster[corner]
    err = np.abs(full["pos"][c].astype(np.float64) - 1.0).max()
    mean_err = np.abs(full["centre"][c] + full["mean"][c] - 1.0).max()
    print("n = %d: corner off by %.4f cell (bound %.4f), the plain mean by %.3f cell; %d triangles left" %
          (n, err / cell, 3 * S.LAM / (1 + 3 * S.LAM), mean_err / cell, len(tris)))
    assert err <= 3 * S.LAM / (1 + 3 * S.LAM) * cell
    assert mean_err > cell / 4
    assert len(tris) == stats["triangles"] == left


@pytest.mark.parametrize("n", S.CUBE_GRIDS)
def test_flat_clusters_stay_on_their_plane(cube, cube_results, n):
    v, t = cube
    _, _, _, cluster, _, full = cube_results[n]
    axis, side = S.cube_face_normals(v, t)
    face = axis * 2 + (side > 0)
    touched = np.zeros((len(full["pos"]), 6), bool)
    touched[cluster[t].reshape(-1), np.repeat(face, 3)] = True
    flat = np.nonzero(touched.sum(1) == 1)[0]
    assert len(flat) >= (6 if n > 2 else 0)
    f = np.argmax(touched[flat], 1)
    got = full["pos"][flat, f // 2].astype(np.float64)
    want = np.where(f % 2 == 1, 1.0, -1.0)
    assert np.abs(got - want).max(initial=0.0) <= 2.0 ** -23      # one fp32 step at 1


@pytest.mark.parametrize("n", S.CUBE_GRIDS)
def test_no_vertex_moves_further_than_a_cell_diagonal(cube, cube_results, n):
    v, _ = cube
    verts, _, _, cluster, stats, full = cube_results[n]
    cell = float(O.grid_cell(v, n))
    used = full["used"][cluster]
    assert used.all() and stats["vertices"] == stats["clusters"] == len(verts)
    d = np.linalg.norm(v.astype(np.float64) - verts[full["newid"][cluster]].astype(np.float64), axis=1)
    assert d.max() <= np.sqrt(3.0) * cell


def test_a_grid_finer_than_every_edge_returns_the_triangles(cube):
    v, t = cube
    cell = O.grid_cell(v, 81)      # 2 / 81 < 2 / 40, the shortest edge: one vertex per cell
    verts, tris, _, cluster, stats, full = O.simplify(v, t, cell, full=True)
    assert stats["clusters"] == stats["vertices"] == len(v) and stats["triangles"] == len(t) and stats["collapsed"] == stats["duplicates"] == 0
    idx = np.floor((v - v.min(0)) / cell).astype(np.int64)
    order = np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))      # key order: z, then y, then x
    # a cell's only member is its mean, and every plane of its quadric passes through it: x = m in exact arithmetic.  The cofactor solve
    # keeps about six of fp64's sixteen digits on a flat cell (det ~ lam^2), the cast to fp32 then lands on the input's own value except
    # beside zero, where fp32 is finer than that error
    assert np.abs(verts.astype(np.float64) - v[order]).max() <= 1e-9 * float(cell)
    assert np.array_equal(cluster[order], np.arange(len(v)))
    # the same geometry: every output triangle is its input triangle rotated to start at its smallest new index
    mapped = cluster[t]
    r = np.argmin(mapped, 1)
    rows = np.arange(len(t))
    assert np.array_equal(tris, np.stack([mapped[rows, r], mapped[rows, (r + 1) % 3], mapped[rows, (r + 2) % 3]], 1))
    assert np.abs(verts[tris[:, 0]].astype(np.float64) - v[t[rows, r]]).max() <= 1e-9 * float(cell)


def test_stacked_plates_lose_one_of_every_pair_and_the_slab_keeps_both_sides():
    v, t, info = S.plates()
    k = info["sheet_tris"]
    verts, tris, _, cluster, stats, full = O.simplify(v, t, S.PLATE_CELL, origin=S.PLATE_ORIGIN, full=True)
    assert stats["duplicates"] == k and stats["collapsed"] == stats["dropped"] == 0 and stats["triangles"] == 3 * k
    assert np.array_equal(full["survivors"], np.concatenate([np.arange(k), np.arange(2 * k, 4 * k)]))      # the lower id of every pair
    per = len(v) // 4
    assert np.array_equal(cluster[:per], cluster[per:2 * per]) and np.array_equal(cluster[2 * per:3 * per], cluster[3 * per:])
    front, back = tris[k:2 * k], tris[2 * k:]
    as_sets = lambda a: {tuple(x) for x in a}
    rot = lambda a: np.stack([a[:, 0], a[:, 2], a[:, 1]], 1)      # the opposite winding, smallest index still first
    assert as_sets(front) == as_sets(rot(back)) and not as_sets(front) & as_sets(back)


@pytest.mark.parametrize("n", S.CUBE_GRIDS)
def test_special_inputs_change_nothing(cube, cube_results, n):
    v, t = cube
    v2, t2 = S.special_cube()
    assert len(v2) == len(v) + 1 and len(t2) == len(t) + 5 and np.array_equal(v2[:-1], v)
    p = v2[t2[-1]].astype(np.float64)
    assert not np.cross(p[1] - p[0], p[2] - p[0]).any() and len(set(t2[-1])) == 3
    want = cube_results[n]
    verts, tris, _, cluster, stats = O.simplify(v2, t2, O.grid_cell(v, n), lam=S.LAM)
    assert O.grid_cell(v2, n) == O.grid_cell(v, n)
    assert np.array_equal(verts.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(tris, want[1])
    assert np.array_equal(cluster[:-1], want[3]) and cluster[-1] == -1
    assert stats["dropped"] == want[4]["dropped"] + 3 and stats["collapsed"] == want[4]["collapsed"] + 2
    assert stats["duplicates"] == want[4]["duplicates"]


def test_limit_and_degenerate_inputs(cube):
    v, t = cube
    with pytest.raises(O.LimitError):
        O.simplify(v, t, np.float32(2.0 / (1 << 21)))
    with pytest.raises(O.LimitError):
        O.simplify(v, t, np.float32(0.5), origin=[0.0, -1.0, -1.0])      # vertices below the origin
    nan = np.full((5, 3), np.nan, np.float32)
    verts, tris, _, cluster, stats = O.simplify(nan, t[:4] % 5, np.float32(1.0))
    assert len(verts) == len(tris) == 0 and (cluster == -1).all() and stats["dropped"] == 4
    verts, tris, _, cluster, stats = O.simplify(v, np.zeros((0, 3), np.int32), np.float32(0.5))
    assert len(verts) == len(tris) == 0 and stats["clusters"] > 0 and cluster.min() == 0


@pytest.mark.parametrize("target", [100, 1000, 5000])
def test_bisection_meets_its_condition(cube, target):
    v, t = cube
    verts, tris, _, _, stats = O.simplify_target(v, t, target)
    n = stats["n"]
    faces = lambda k: O.count_faces(v, t, O.grid_cell(v, k))
    print("target %d: n = %d after %d probes, %d <= target < %d" % (target, n, stats["probes"], faces(n), faces(n + 1)))
    assert faces(n) == len(tris) <= target < faces(n + 1)
    assert stats["probes"] <= 2 * int(np.ceil(np.log2(n + 1))) + 1
    same = O.simplify_target(v, t, len(t))
    assert same[0] is not None and np.array_equal(same[1], t) and same[4]["n"] == 0


# ------------------------------------------------------------------------------------------------ library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_simplify_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", HEADER)).read(), re.M)
    assert len(decl) == 4
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.SIMPLIFY_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    others = [name for h, group in surfel_native.SIGNATURES.items() if h != HEADER for name in group]
    assert not set(decl) & set(others)
    lib = surfel_native.load()
    for name in surfel_native.SIMPLIFY_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_simplify", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "mesh_simplify.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["mesh_simplify.hip"] and any(h.endswith(HEADER) for h in mod.HEADERS)
    import surfel_simplify as P
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    assert int(re.search(r"#define SURFEL_SIMPLIFY_AXIS_BITS (\d+)", hdr).group(1)) == O.AXIS_BITS
    assert int(re.search(r"#define SURFEL_SIMPLIFY_COUNTS (\d+)", hdr).group(1)) == len(P.COUNTS)
    assert int(re.search(r"#define SURFEL_SIMPLIFY_STAGES (\d+)", hdr).group(1)) == len(P.STAGES)
    assert P.N_MAX == O.N_MAX and P.LAM == S.LAM


def test_simplify_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_simplify.h."""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 4
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
                host = pname in ("bounds", "origin", "counts", "stage_ms", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_python_surface_refuses_host_tensors_and_bad_arguments():
    sys.path.insert(0, PKG)
    import torch
    import surfel_simplify as P
    from surfel_mesh import TriangleMesh
    mesh = TriangleMesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), None)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.simplify_mesh(mesh, cell=0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.vertex_clusters(mesh, 0.5)
    with pytest.raises(ValueError, match="cell or target_faces"):
        P.simplify_mesh(mesh)
    with pytest.raises(ValueError, match="cell or target_faces"):
        P.simplify_mesh(mesh, cell=0.5, target_faces=10)
    import surfel_mesh
    args = surfel_mesh.build_parser().parse_args(["-m", "x"])      # without the flags the mesh CLI simplifies nothing
    assert args.simplify_cell is None and args.simplify_faces is None
    with pytest.raises(SystemExit, match="not both"):
        surfel_mesh.main(["-m", "x", "--simplify_cell", "2", "--simplify_faces", "10"])
    # the search itself, on a count that is monotone: the same answer as the oracle's, the local condition, few probes
    for target in (0, 1, 7, 1000, 10 ** 9):
        faces = lambda k: 6 * (k - 1) ** 2
        n, probes = P.bisect_resolution(faces, target)
        assert (n, probes) == O.bisect(faces, target)
        assert faces(n) <= target and (n == P.N_MAX or target < faces(n + 1)) and probes <= 41
