"""GPU checks of the mesh simplification (include/surfel_simplify.h, SIMPLIFY.md): every fixture and grid against the numpy restatement
(tests/simplify_oracle.py) — clusters, triangles and stats equal, vertex positions and colours equal as bit patterns — run-to-run
identity, the inputs the rules skip, empty meshes, the index limit, canaries around every output buffer, the bisection, and the mesh
CLI end to end on a mesh of the project's own bounded extraction."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import simplify_oracle as O  # noqa: E402
import simplify_scenes as S  # noqa: E402
from device_mesh import dev as _dev, mesh as _mesh, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_KEYS = ("clusters", "vertices", "triangles", "dropped", "collapsed", "duplicates")


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _cases():
    """name -> (verts, tris, colors, cell, origin): every fixture at every grid"""
    cv, ct = S.cube()
    sv, st, sc = S.sphere()
    xv, xt = S.special_cube()
    pv, pt, _ = S.plates()
    rng = np.random.default_rng(3)
    cases = {}
    for n in S.CUBE_GRIDS:
        cases["cube-%d" % n] = (cv, ct, rng.random(cv.shape).astype(np.float32) if n == 8 else None, O.grid_cell(cv, n), None)
        cases["special-%d" % n] = (xv, xt, None, O.grid_cell(cv, n), None)
    for n in S.SPHERE_GRIDS:
        cases["sphere-%d" % n] = (sv, st, sc, O.grid_cell(sv, n), None)
    cases["plates"] = (pv, pt, None, S.PLATE_CELL, S.PLATE_ORIGIN)
    cases["cube-fine"] = (cv, ct, None, O.grid_cell(cv, 81), None)
    cases["cube-moved-origin"] = (cv, ct, None, np.float32(0.3), np.array([-1.25, -1.0, -1.5], np.float32))
    # the scans' edges.  A 64 x 64 lattice, every point the centre of its own cell, with its first 4 096 triangles: vertices, triangles,
    # candidates and cells are one full scan tile each.  One triangle over three cells: scans of one flag, and two key bits, so that each
    # of the three sorts is a single pass and leaves the sorted pairs in the second buffer pair.
    g = np.arange(64)
    X, Y = np.meshgrid(g, g, indexing="ij")
    lv = np.stack([X.reshape(-1) / 16.0, Y.reshape(-1) / 16.0, np.zeros(4096)], 1).astype(np.float32)
    a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(63), np.arange(63), indexing="ij"))
    at = lambda u, w: u * 64 + w
    lt = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], 1), np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], 1)])[:4096].astype(np.int32)
    cases["lattice-one-tile"] = (lv, lt, None, S.PLATE_CELL, S.PLATE_ORIGIN)
    cases["one-triangle"] = (lv[[0, 1, 64]], np.array([[0, 1, 2]], np.int32), None, S.PLATE_CELL, S.PLATE_ORIGIN)
    return cases


CASES = _cases()
_WANT = {}


def _want(name):
    if name not in _WANT:
        v, t, c, cell, origin = CASES[name]
        _WANT[name] = O.simplify(v, t, cell, c, origin, S.LAM, full=True)
    return _WANT[name]


def _run(name, **kw):
    import surfel_simplify as P
    v, t, c, cell, origin = CASES[name]
    return P.simplify_mesh(_mesh(v, t, c), cell=float(cell), origin=origin, lam=S.LAM, **kw)


def _same(got, stats, want):
    verts, tris, cols, cluster, wstats, full = want
    assert {k: stats[k] for k in STAT_KEYS} == {k: wstats[k] for k in STAT_KEYS}
    assert np.array_equal(stats["cluster"].cpu().numpy(), cluster)
    assert np.array_equal(stats["cluster_vertex"].cpu().numpy(), full["newid"])
    assert np.array_equal(got.triangles.cpu().numpy(), tris)
    assert got.vertices.dtype == torch.float32 and got.triangles.dtype == torch.int32
    diff = np.argwhere(_bits(got.vertices) != _bits(verts))
    assert not len(diff), (len(diff), diff[:5], got.vertices.cpu().numpy()[diff[0][0]], verts[diff[0][0]])
    if cols is None:
        assert got.vertex_colors is None
    else:
        assert np.array_equal(_bits(got.vertex_colors), _bits(cols))


# ------------------------------------------------------------------------------------------------ 1: the oracle, byte for byte
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_restatement_bit_for_bit(name):
    import surfel_simplify as P
    got, stats = _run(name)
    want = _want(name)
    print("%s: %d -> %d vertices, %d -> %d triangles (%d collapsed, %d duplicates)" %
          (name, len(CASES[name][0]), stats["vertices"], len(CASES[name][1]), stats["triangles"], stats["collapsed"], stats["duplicates"]))
    _same(got, stats, want)
    v, t, c, cell, origin = CASES[name]
    assert np.array_equal(P.vertex_clusters(_mesh(v, t), float(cell), origin).cpu().numpy(), want[3])
    counted = P.count_faces(_mesh(v, t), float(cell), origin)
    assert counted == {k: want[4][k] for k in STAT_KEYS if k != "vertices"}
    b = P.mesh_bounds(_t(v))
    assert np.array_equal(b[0], O.bounds(v)[0]) and np.array_equal(b[1], O.bounds(v)[1])


def test_scan_edge_cases_hold_what_they_are_there_for():
    """conditions on the inputs of lattice-one-tile and one-triangle, and the one count they cannot reach: a single vertex"""
    import surfel_simplify as P
    v, t, _, cell, origin = CASES["lattice-one-tile"]
    w = _want("lattice-one-tile")[4]
    assert len(v) == len(t) == 4096 and w["clusters"] == 4096 and w["dropped"] == w["collapsed"] == w["duplicates"] == 0 and w["triangles"] == 4096
    w = _want("one-triangle")[4]
    assert w["clusters"] == 3 and w["triangles"] == 1
    got = P.vertex_clusters(_mesh(v[:1], np.zeros((0, 3), np.int32)), float(cell), origin)
    assert got.cpu().numpy().tolist() == [0]


# ------------------------------------------------------------------------------------------------ 2: the same bytes
@pytest.mark.parametrize("name", ["cube-2", "sphere-13", "special-8"])
def test_two_runs_give_identical_bytes(name):
    timings = {}
    a, sa = _run(name, timings=timings)
    torch.empty(1 << 24, dtype=torch.uint8, device=_dev()).fill_(0xA5)      # (a different history of the allocator's memory)
    junk = [torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=_dev()) for n in (1 << 12, 1 << 16, 1 << 20)]
    del junk
    b, sb = _run(name)
    for x, y in ((a.vertices, b.vertices), (a.triangles, b.triangles), (sa["cluster"], sb["cluster"]), (sa["cluster_vertex"], sb["cluster_vertex"])):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    if a.vertex_colors is not None:
        assert a.vertex_colors.cpu().numpy().tobytes() == b.vertex_colors.cpu().numpy().tobytes()
    import surfel_simplify as P
    assert set(timings) == set(P.STAGES) | {"bisection_ms"} and all(v >= 0 for v in timings.values()) and timings["sorts_ms"] > 0
    _same(a, sa, _want(name))      # (the timed call computes the same)


# ------------------------------------------------------------------------------------------------ 3: skipped inputs
@pytest.mark.parametrize("n", S.CUBE_GRIDS)
def test_special_inputs_change_nothing(n):
    plain, ps = _run("cube-%d" % n)
    special, ss = _run("special-%d" % n)
    assert _bits(plain.vertices).tobytes() == _bits(special.vertices).tobytes() and torch.equal(plain.triangles, special.triangles)
    assert torch.equal(ss["cluster"][:-1], ps["cluster"]) and int(ss["cluster"][-1]) == -1
    assert ss["dropped"] == ps["dropped"] + 3 and ss["collapsed"] == ps["collapsed"] + 2 and ss["duplicates"] == ps["duplicates"]


# ------------------------------------------------------------------------------------------------ 4: empty cases
def test_empty_meshes():
    import surfel_simplify as P
    v, t = S.cube()
    none, stats = P.simplify_mesh(_mesh(v, np.zeros((0, 3), np.int32)), cell=0.5)
    assert tuple(none.vertices.shape) == (0, 3) and tuple(none.triangles.shape) == (0, 3)
    assert stats["clusters"] == 98 and stats["vertices"] == stats["triangles"] == 0      # 5^3 - 3^3 surface cells
    assert int(stats["cluster"].min()) == 0 and int(stats["cluster"].max()) == 97 and bool((stats["cluster_vertex"] == -1).all())
    nan = np.full((300, 3), np.nan, np.float32)
    nan[::3, 1] = np.inf
    nan[1::3, 0] = 1.0      # (finite in one coordinate only)
    gone, stats = P.simplify_mesh(_mesh(nan, t[:500] % 300, nan), cell=0.5)
    assert tuple(gone.vertices.shape) == (0, 3) and tuple(gone.triangles.shape) == (0, 3) and tuple(gone.vertex_colors.shape) == (0, 3)
    assert stats["clusters"] == 0 and stats["dropped"] == 500 and bool((stats["cluster"] == -1).all())
    assert P.mesh_bounds(_t(nan)) is None and bool((P.vertex_clusters(_mesh(nan, t[:1]), 0.5) == -1).all())
    assert P.count_faces(_mesh(nan, t[:500] % 300), 0.5)["triangles"] == 0
    nothing, stats = P.simplify_mesh(_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), cell=0.5)
    assert tuple(nothing.vertices.shape) == (0, 3) and stats["clusters"] == 0
    same, stats = P.simplify_mesh(_mesh(nan, t[:4] % 300), target_faces=2)      # the bisection has nothing to bracket
    assert tuple(same.triangles.shape) == (0, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5: the limit, 6: buffers respected
def _carve(sizes, pad=4096):
    total = pad + sum(s + pad + 8 for s in sizes.values())
    big = torch.empty(total, dtype=torch.uint8, device=_dev())
    pattern = (torch.arange(total, device=_dev()) * 37 + 11).to(torch.uint8)
    big.copy_(pattern)
    off, at = {}, pad
    for name, s in sizes.items():
        at = (at + 7) // 8 * 8
        off[name] = at
        at += s + pad
    inside = torch.zeros(total, dtype=torch.bool, device=_dev())
    for name, s in sizes.items():
        inside[off[name]:off[name] + s] = True
    view = lambda name, dtype: big[off[name]:off[name] + sizes[name]].view(dtype)
    return big, pattern, inside, view


def _raw_call(v, t, c, cell, origin, view, counts):
    import ctypes as C
    import surfel_native as N
    alloc = N.TorchAllocator(_dev())
    org = None if origin is None else (C.c_float * 3)(*[float(x) for x in origin])
    return N.call(_dev(), "surfel_simplify_mesh", alloc.cb, None, len(v), len(t), _t(v), _t(c) if c is not None else None, _t(t), None, org, float(cell),
                  S.LAM, view("cluster", torch.int32), view("cluster_vertex", torch.int32), view("verts", torch.float32),
                  view("colors", torch.float32) if c is not None else None, view("tris", torch.int32), counts, None)


def test_an_index_past_21_bits_is_refused_before_anything_is_written():
    import ctypes as C
    import surfel_native as N
    import surfel_simplify as P
    v, t = S.cube()
    sizes = {"cluster": 4 * len(v), "cluster_vertex": 4 * len(v), "verts": 12 * len(v), "colors": 12 * len(v), "tris": 12 * len(t)}
    big, pattern, inside, view = _carve(sizes)
    counts = (C.c_int64 * 6)(*([-7] * 6))
    with pytest.raises(N.LimitError, match=r"\(-4\): .*cell index"):
        _raw_call(v, t, v, np.float32(2.0 / (1 << 21)), None, view, counts)
    with pytest.raises(N.LimitError, match=r"\(-4\): .*below the origin"):
        _raw_call(v, t, v, np.float32(0.5), [0.0, -1.0, -1.0], view, counts)
    torch.cuda.synchronize()
    assert torch.equal(big, pattern) and list(counts) == [-7] * 6
    for call in (lambda: P.simplify_mesh(_mesh(v, t), cell=2.0 / (1 << 21)), lambda: P.vertex_clusters(_mesh(v, t), 2.0 / (1 << 21)),
                 lambda: P.count_faces(_mesh(v, t), 2.0 / (1 << 21))):
        with pytest.raises(P.MeshLimitError):
            call()
    # the largest index that fits is accepted: the cube's extent in 2^21 - 1 cells and the maximum in the last one
    cell = np.float32(2.0 / ((1 << 21) - 1.5))
    assert int(np.floor(np.float32(2.0) / cell)) == (1 << 21) - 2
    got = P.vertex_clusters(_mesh(v, t), float(cell))
    assert np.array_equal(got.cpu().numpy(), O.clusters(v, cell)[0])


@pytest.mark.parametrize("name", ["special-8", "sphere-5", "plates"])
def test_canaries_around_every_output_buffer(name):
    """cluster, cluster_vertex, vertices, colours and triangles carved out of one allocation filled with a pattern: the pattern on both sides
    of each is intact after the call, and what lies inside is the result"""
    import ctypes as C
    v, t, c, cell, origin = CASES[name]
    sizes = {"cluster": 4 * len(v), "cluster_vertex": 4 * len(v), "verts": 12 * len(v), "colors": 12 * len(v), "tris": 12 * len(t)}
    big, pattern, inside, view = _carve(sizes)
    counts = (C.c_int64 * 6)()
    _raw_call(v, t, c, cell, origin, view, counts)
    torch.cuda.synchronize()
    assert torch.equal(big[~inside], pattern[~inside]) and int((~inside).sum()) >= 6 * 4096
    verts, tris, cols, cluster, stats, full = _want(name)
    assert list(counts) == [stats[k] for k in STAT_KEYS]
    nc, nv, nf = counts[0], counts[1], counts[2]
    assert np.array_equal(view("cluster", torch.int32).cpu().numpy(), cluster)
    assert np.array_equal(view("cluster_vertex", torch.int32)[:nc].cpu().numpy(), full["newid"])
    assert np.array_equal(_bits(view("verts", torch.float32)[:3 * nv]), _bits(verts).reshape(-1))
    assert np.array_equal(view("tris", torch.int32)[:3 * nf].cpu().numpy(), tris.reshape(-1))
    if cols is not None:
        assert np.array_equal(_bits(view("colors", torch.float32)[:3 * nv]), _bits(cols).reshape(-1))
    # behind the rows the library reports, the buffers keep the pattern too (a mesh without colours leaves the colour rows alone)
    for nm, used in (("verts", 12 * nv), ("tris", 12 * nf), ("cluster_vertex", 4 * nc), ("colors", 12 * nv if cols is not None else 0)):
        lo = int(view(nm, torch.uint8).data_ptr() - big.data_ptr())
        assert torch.equal(big[lo + used:lo + sizes[nm]], pattern[lo + used:lo + sizes[nm]]), nm


# ------------------------------------------------------------------------------------------------ 7: the bisection
@pytest.mark.parametrize("target", [100, 1000, 5000])
def test_target_faces_meets_the_bisection_condition(target):
    import surfel_simplify as P
    v, t = S.cube()
    timings = {}
    got, stats = P.simplify_mesh(_mesh(v, t), target_faces=target, timings=timings)
    want = O.simplify_target(v, t, target)
    n = stats["n"]
    assert n == want[4]["n"] and stats["probes"] == want[4]["probes"] and timings["bisection_ms"] > 0
    b = P.mesh_bounds(_t(v))
    faces = lambda k: P.count_faces(_mesh(v, t), P.grid_cell(b, k))["triangles"]
    assert faces(n) == got.triangles.shape[0] <= target < faces(n + 1)
    assert np.float32(P.grid_cell(b, n)) == O.grid_cell(v, n) == np.float32(stats["cell"])
    assert np.array_equal(_bits(got.vertices), _bits(want[0])) and np.array_equal(got.triangles.cpu().numpy(), want[1])
    if target == 100:
        mesh = _mesh(v, t, v)
        same, stats = P.simplify_mesh(mesh, target_faces=len(t))
        assert same.vertices is mesh.vertices and same.triangles is mesh.triangles and stats["n"] == 0 and stats["triangles"] == len(t)


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_mesh_cli_writes_a_simplified_mesh(tmp_path):
    """surfel_mesh.py --simplify_cell 4 on a sphere of surfels: fuse_post.ply as before, fuse_post_simplified.ply beside it with fewer
    triangles, every vertex within a cell diagonal of an input vertex, and a mesh the viewer renders"""
    import surfel_eval as E
    import surfel_io
    import surfel_mesh
    import surfel_meshview as MV
    import surfel_trainer as TR
    import test_gpu_mesh as TM
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import mesh_bench
    dev = _dev()
    model = TM._sphere_model(dev)
    cams = TR.orbit_cameras(22, 256, 192, device=dev)
    mesh_bench.write_model_dir(model, cams, str(tmp_path), 7)
    res, k = 256, 4
    assert surfel_mesh.main(["-m", str(tmp_path), "--mesh_res", str(res), "--simplify_cell", str(k), "--num_cluster", "1"]) == 0
    out = tmp_path / "train" / "ours_7"
    assert sorted(os.listdir(out)) == ["fuse.ply", "fuse_post.ply", "fuse_post_simplified.ply"]
    v, t, c = surfel_io.read_triangle_mesh(str(out / "fuse_post.ply"))
    sv, st, sc = surfel_io.read_triangle_mesh(str(out / "fuse_post_simplified.ply"))
    radius = surfel_mesh.bounding_sphere(np.stack([np.linalg.inv(np.asarray(cm.world_view_transform.T.cpu().numpy(), np.float64)) for cm in cams]))[1]
    cell = k * (2.0 * radius / res)
    print("end to end: %d -> %d vertices, %d -> %d triangles, cell %.4f" % (len(v), len(sv), len(t), len(st), cell))
    assert len(t) > 2000 and 100 < len(st) < len(t) / 4 and st.min() == 0 and st.max() == len(sv) - 1
    dist = E.nearest(torch.from_numpy(sv).to(dev), torch.from_numpy(v).to(dev)).cpu().numpy()      # exact search; the input is its reference set
    assert np.isfinite(dist).all() and dist.max() <= np.sqrt(3.0) * cell * (1 + 1e-5)
    assert np.abs(np.linalg.norm(sv, axis=1) - 1.0).max() < 0.15 and sc.min() >= 0 and sc.max() <= 1
    mesh = _mesh(sv, st, sc)
    frame = MV.render_mesh(mesh, cams[:1])
    assert tuple(frame.shape) == (1, 192, 256, 3) and len(np.unique(frame.cpu().numpy().reshape(-1, 3), axis=0)) > 20
