"""GPU checks of the mesh smoothing (include/surfel_smooth.h, SMOOTH.md): on every fixture the adjacency arrays, flags and counts equal
the numpy restatement (tests/smooth_oracle.py) exactly and the filtered positions equal it as bit patterns — both schedules, all three
boundary modes, rows on both sides of every length at which the step kernel takes another path — colours, the NaN vertex, run-to-run
identity, untouched inputs, canaries around every output buffer, a passed-in adjacency, and both CLIs end to end."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import simplify_scenes as S  # noqa: E402
import smooth_oracle as O  # noqa: E402
import smooth_scenes as M  # noqa: E402
from device_mesh import dev as _dev, mesh as _mesh, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = M.meshes()
_ADJ = {}


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _adj(name):
    """the oracle's adjacency of a fixture, computed once and never written"""
    if name not in _ADJ:
        _ADJ[name] = O.adjacency(*MESHES[name])
    return _ADJ[name]


def _same_adjacency(got, want):
    assert got.offsets.dtype == got.neighbors.dtype == got.multiplicity.dtype == torch.int32 and got.flags.dtype == torch.uint8
    for key in ("offsets", "neighbors", "multiplicity", "flags"):
        g = getattr(got, key).cpu().numpy()
        assert g.shape == want[key].shape and np.array_equal(g, want[key]), key
    assert got.stats == want["stats"]


def _same_bits(got, want, what):
    diff = np.argwhere(_bits(got) != _bits(want))
    assert not len(diff), (what, len(diff), diff[:5], got.cpu().numpy()[diff[0][0]], want[diff[0][0]])


# ------------------------------------------------------------------------------------------------ 1: the adjacency, exactly
@pytest.mark.parametrize("name", sorted(MESHES))
def test_adjacency_equals_the_restatement(name):
    import surfel_smooth as P
    v, t = MESHES[name]
    got = P.mesh_adjacency(_mesh(v, t))
    print("%s: V %d, F %d, %s" % (name, len(v), len(t), got.stats))
    _same_adjacency(got, _adj(name))


# ------------------------------------------------------------------------------------------------ 2: positions, bit for bit
POSITION_CASES = [(name, method, n, "free") for name in ("cube", "sphere") for method in ("taubin", "laplacian") for n in (1, 10)] + \
                 [("plates", "taubin", 3, b) for b in O.BOUNDARY] + \
                 [("clustered", "taubin", 4, b) for b in O.BOUNDARY] + \
                 [("umbrellas", "taubin", 2, b) for b in O.BOUNDARY] + \
                 [("fan", "taubin", 2, "free"), ("fan", "laplacian", 3, "curve"), ("special", "taubin", 3, "free"), ("special", "laplacian", 2, "fixed"),
                  ("all-dropped", "taubin", 2, "free"), ("no-triangle", "laplacian", 1, "free")]


@pytest.mark.parametrize("name,method,n,boundary", POSITION_CASES)
def test_positions_equal_the_restatement_bit_for_bit(name, method, n, boundary):
    import surfel_smooth as P
    v, t = MESHES[name]
    mesh = _mesh(v, t)
    got, stats = P.smooth_mesh(mesh, iterations=n, method=method, boundary=boundary)
    want = O.smooth(v, _adj(name), n, method, boundary=boundary)
    assert got.vertices.dtype == torch.float32 and tuple(got.vertices.shape) == v.shape
    _same_bits(got.vertices, want, (name, method, n, boundary))
    assert got.triangles is mesh.triangles and got.vertex_colors is None
    assert stats["steps"] == (2 * n if method == "taubin" else n) and {k: stats[k] for k in O.COUNTS} == _adj(name)["stats"]
    assert np.array_equal(_bits(mesh.vertices), _bits(v)) and torch.equal(mesh.triangles, _t(t))      # the input is not written
    if len(v) and _adj(name)["stats"]["directed_edges"] and boundary != "fixed":
        assert (_bits(got.vertices) != _bits(v)).any()


def test_other_parameters_and_no_iteration():
    import surfel_smooth as P
    v, t, _ = M.noisy_sphere()
    mesh = _mesh(v, t)
    got, _ = P.smooth_mesh(mesh, iterations=3, lam=0.33, mu=-0.34)
    _same_bits(got.vertices, O.smooth(v, _adj("sphere"), 3, lam=0.33, mu=-0.34), "lam 0.33")
    got, _ = P.smooth_mesh(mesh, iterations=2, method="laplacian", lam=1.0)
    _same_bits(got.vertices, O.smooth(v, _adj("sphere"), 2, "laplacian", lam=1.0), "lam 1")
    same, stats = P.smooth_mesh(mesh, iterations=0)
    assert stats["steps"] == 0 and same.vertices is not mesh.vertices and np.array_equal(_bits(same.vertices), _bits(v))
    empty, stats = P.smooth_mesh(_mesh(*MESHES["no-vertex"]), iterations=2)
    assert tuple(empty.vertices.shape) == (0, 3) and stats["directed_edges"] == 0
    with pytest.raises(ValueError, match="rows"):
        P.filter_steps(P.mesh_adjacency(mesh), _t(v[:-1]), [0.5])


# ------------------------------------------------------------------------------------------------ 3: colours, the NaN vertex
def test_colours_filtered_only_on_request():
    import surfel_smooth as P
    v, t, c = M.noisy_sphere()
    mesh = _mesh(v, t, c)
    plain, _ = P.smooth_mesh(mesh, iterations=2)
    assert plain.vertex_colors is mesh.vertex_colors and np.array_equal(_bits(plain.vertex_colors), _bits(c))
    both, _ = P.smooth_mesh(mesh, iterations=2, colors=True)
    _same_bits(both.vertex_colors, O.smooth(c, _adj("sphere"), 2), "colours")
    assert np.array_equal(_bits(both.vertices), _bits(plain.vertices)) and np.array_equal(_bits(mesh.vertex_colors), _bits(c))


def test_nan_vertex_passes_through_with_its_bits():
    import surfel_smooth as P
    v, t = S.special_cube()
    v = v.copy()
    v.view(np.uint32)[-1] = (0x7FC12345, 0xFFC00001, 0x7F800000)      # two NaN payloads and an infinity
    got, stats = P.smooth_mesh(_mesh(v, t), iterations=2)
    assert _bits(got.vertices)[-1].tolist() == [0x7FC12345, 0xFFC00001, 0x7F800000] and stats["isolated_vertices"] == 1
    _same_bits(got.vertices, O.smooth(v, O.adjacency(v, t), 2), "special with payloads")
    assert bool(torch.isfinite(got.vertices[:-1]).all())


# ------------------------------------------------------------------------------------------------ 4: the same bytes, a passed-in adjacency
@pytest.mark.parametrize("name", ["sphere", "clustered", "fan"])
def test_two_runs_give_identical_bytes(name):
    import surfel_smooth as P
    v, t = MESHES[name]
    mesh = _mesh(v, t)
    timings = {}
    a, sa = P.smooth_mesh(mesh, iterations=3, boundary="curve", timings=timings)
    torch.empty(1 << 24, dtype=torch.uint8, device=_dev()).fill_(0xA5)      # (a different history of the allocator's memory)
    junk = [torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=_dev()) for n in (1 << 12, 1 << 16, 1 << 20)]
    del junk
    b, sb = P.smooth_mesh(mesh, iterations=3, boundary="curve")
    assert a.vertices.cpu().numpy().tobytes() == b.vertices.cpu().numpy().tobytes()
    for key in ("offsets", "neighbors", "multiplicity", "flags"):
        assert getattr(sa["adjacency"], key).cpu().numpy().tobytes() == getattr(sb["adjacency"], key).cpu().numpy().tobytes()
    assert sa["adjacency"].stats == sb["adjacency"].stats
    assert set(timings) == {"adjacency_ms", "steps_ms"} and timings["adjacency_ms"] > 0 and timings["steps_ms"] > 0
    adj = P.mesh_adjacency(mesh)
    c, sc = P.smooth_mesh(mesh, iterations=3, boundary="curve", adjacency=adj)
    assert sc["adjacency"] is adj and c.vertices.cpu().numpy().tobytes() == a.vertices.cpu().numpy().tobytes()
    _same_adjacency(adj, _adj(name))      # (the steps read the adjacency only)


# ------------------------------------------------------------------------------------------------ 5: buffers respected
def _carve(sizes, pad=4096):
    total = pad + sum(s + pad + 16 for s in sizes.values())
    big = torch.empty(total, dtype=torch.uint8, device=_dev())
    pattern = (torch.arange(total, device=_dev()) * 37 + 11).to(torch.uint8)
    big.copy_(pattern)
    off, at = {}, pad
    for name, s in sizes.items():
        at = (at + 15) // 16 * 16
        off[name] = at
        at += s + pad
    inside = torch.zeros(total, dtype=torch.bool, device=_dev())
    for name, s in sizes.items():
        inside[off[name]:off[name] + s] = True
    view = lambda name, dtype: big[off[name]:off[name] + sizes[name]].view(dtype)
    return big, pattern, inside, view, off


@pytest.mark.parametrize("name,boundary", [("special", "free"), ("plates", "curve"), ("umbrellas", "fixed")])
def test_canaries_around_every_output_buffer(name, boundary):
    """offsets, neighbours, multiplicities, flags, the steps' scratch and the output carved out of one allocation filled with a pattern:
    the pattern on both sides of each is intact after the two calls, and behind the E2 entries the library reports"""
    import ctypes as C
    import surfel_native as N
    v, t = MESHES[name]
    V, F = len(v), len(t)
    sizes = {"offsets": 4 * (V + 1), "neighbors": 24 * F, "multiplicity": 24 * F, "flags": V, "scratch": 12 * V, "out": 12 * V}
    big, pattern, inside, view, off = _carve(sizes)
    assert big.data_ptr() % 16 == 0
    counts = (C.c_int64 * 8)()
    alloc = N.TorchAllocator(_dev())
    dv, dt = _t(v), _t(t)
    e2 = N.call(_dev(), "surfel_smooth_adjacency", alloc.cb, None, V, F, dv, dt, view("offsets", torch.int32), view("neighbors", torch.int32),
                view("multiplicity", torch.int32), view("flags", torch.uint8), counts)
    factors = [0.5, -0.53, 0.5]
    N.call(_dev(), "surfel_smooth_steps", V, view("offsets", torch.int32), view("neighbors", torch.int32), view("multiplicity", torch.int32),
           view("flags", torch.uint8), O.BOUNDARY.index(boundary), len(factors), (C.c_double * 3)(*factors), dv, view("scratch", torch.float32),
           view("out", torch.float32))
    torch.cuda.synchronize()
    assert torch.equal(big[~inside], pattern[~inside]) and int((~inside).sum()) >= 7 * 4096
    want = _adj(name)
    assert e2 == want["stats"]["directed_edges"] and list(counts) == [want["stats"][k] for k in O.COUNTS]
    assert np.array_equal(view("offsets", torch.int32).cpu().numpy(), want["offsets"])
    assert np.array_equal(view("neighbors", torch.int32)[:e2].cpu().numpy(), want["neighbors"])
    assert np.array_equal(view("multiplicity", torch.int32)[:e2].cpu().numpy(), want["multiplicity"])
    assert np.array_equal(view("flags", torch.uint8).cpu().numpy(), want["flags"])
    for nm in ("neighbors", "multiplicity"):
        lo = off[nm]
        assert torch.equal(big[lo + 4 * e2:lo + sizes[nm]], pattern[lo + 4 * e2:lo + sizes[nm]]), nm
    the_plan = O.plan(want, boundary)
    out = np.asarray(v, np.float32)
    for f in factors:
        out = O.step(out, the_plan, f)
    assert np.array_equal(_bits(view("out", torch.float32)).reshape(-1, 3), _bits(out))
    assert np.array_equal(_bits(dv), _bits(v)) and torch.equal(dt, _t(t))


# ------------------------------------------------------------------------------------------------ 6: end to end
def test_smooth_cli_writes_a_smoothed_ply(tmp_path):
    import surfel_io
    import surfel_smooth as P
    v, t, c = M.noisy_sphere()
    path = str(tmp_path / "ball.ply")
    surfel_io.write_triangle_mesh(path, _mesh(v, t, c).numpy())
    out = P.main(["--ply-path", path, "--iterations", "4", "--boundary", "fixed", "--colors"])
    assert sorted(os.listdir(tmp_path)) == ["ball.ply", "ball_smoothed.ply"]
    rv, rt, rc = surfel_io.read_triangle_mesh(path)      # (the file holds 8-bit colours: the CLI smooths what it read)
    sv, st, sc = surfel_io.read_triangle_mesh(str(tmp_path / "ball_smoothed.ply"))
    adj = O.adjacency(rv, rt)
    assert np.array_equal(_bits(sv), _bits(O.smooth(rv, adj, 4, boundary="fixed"))) and np.array_equal(st, rt)
    assert np.array_equal(_bits(out.vertex_colors), _bits(O.smooth(rc, adj, 4, boundary="fixed")))
    assert np.array_equal(sc, np.round(np.clip(out.vertex_colors.cpu().numpy(), 0, 1) * 255).astype(np.uint8).astype(np.float32) / 255)
    assert M.radial_stats(sv)[0] < 0.8 * M.radial_stats(rv)[0]


def test_mesh_cli_writes_a_smoothed_mesh(tmp_path):
    """surfel_mesh.py --smooth_iterations 2 on a sphere of surfels: fuse_post.ply byte for byte what a run without the flag writes,
    fuse_post_smoothed.ply beside it equal to smooth_mesh of that file's mesh; a --simplify_cell in the same run still writes its file"""
    import surfel_io
    import surfel_mesh
    import surfel_smooth as P
    import surfel_trainer as TR
    import test_gpu_mesh as TM
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import mesh_bench
    dev = _dev()
    model = TM._sphere_model(dev)
    cams = TR.orbit_cameras(22, 256, 192, device=dev)
    mesh_bench.write_model_dir(model, cams, str(tmp_path), 7)
    res = 128
    out = tmp_path / "train" / "ours_7"
    assert surfel_mesh.main(["-m", str(tmp_path), "--mesh_res", str(res), "--num_cluster", "1"]) == 0
    assert sorted(os.listdir(out)) == ["fuse.ply", "fuse_post.ply"]
    before = open(out / "fuse_post.ply", "rb").read()
    assert surfel_mesh.main(["-m", str(tmp_path), "--mesh_res", str(res), "--num_cluster", "1", "--smooth_iterations", "2", "--smooth_boundary", "curve",
                             "--simplify_cell", "3"]) == 0
    assert sorted(os.listdir(out)) == ["fuse.ply", "fuse_post.ply", "fuse_post_simplified.ply", "fuse_post_smoothed.ply"]
    assert open(out / "fuse_post.ply", "rb").read() == before
    v, t, c = surfel_io.read_triangle_mesh(str(out / "fuse_post.ply"))
    sv, st, sc = surfel_io.read_triangle_mesh(str(out / "fuse_post_smoothed.ply"))
    assert len(t) > 1000 and np.array_equal(st, t) and np.array_equal(sc, c)
    want, stats = P.smooth_mesh(_mesh(v, t, c), iterations=2, boundary="curve")
    print("end to end: %d vertices, %d triangles, %s" % (len(v), len(t), {k: stats[k] for k in O.COUNTS}))
    assert np.array_equal(_bits(sv), _bits(want.vertices)) and (sv != v).any()
    _same_bits(want.vertices, O.smooth(v, O.adjacency(v, t), 2, boundary="curve"), "extracted mesh")
    qv, qt, _ = surfel_io.read_triangle_mesh(str(out / "fuse_post_simplified.ply"))      # (the later steps still run)
    assert 100 < len(qt) < len(t) / 2 and qt.min() == 0 and qt.max() == len(qv) - 1
