"""GPU checks of the mesh repair (include/surfel_repair.h, REPAIR.md): on every fixture and cap all integer outputs and the counts equal
the numpy restatement (tests/repair_oracle.py) exactly, positions and colours equal it as bit patterns; the vertex adjacency of the
output (mesh_smooth.hip, which shares rule 1 and the sort's helper with the repair, nothing else) finds no non-manifold edge and the
border the counts name; one mesh that fails rule 1 in every way, on which both modules keep the same triangles; run-to-run
identity, untouched inputs, canaries around every output buffer, border_loops against repair_mesh(max_hole_edges=0), and both CLIs end
to end."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import repair_oracle as O  # noqa: E402
import repair_scenes as R  # noqa: E402
import test_repair_cpu as TC  # noqa: E402  (the restatement's results, computed once for both files)
from device_mesh import dev as _dev, mesh as _mesh, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = TC.CASES


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _same(got, stats, want, what):
    for key, g in (("triangles", got.triangles), ("vertex_source", stats["vertex_source"]), ("triangle_source", stats["triangle_source"]),
                   ("loop_lengths", stats["loop_lengths"])):
        assert g.dtype == torch.int32 and tuple(g.shape) == want[key].shape, (what, key, tuple(g.shape), want[key].shape)
        assert np.array_equal(g.cpu().numpy(), want[key]), (what, key)
    assert {k: stats[k] for k in O.COUNTS} == want["stats"], what
    assert got.vertices.dtype == torch.float32 and tuple(got.vertices.shape) == want["vertices"].shape
    assert np.array_equal(_bits(got.vertices), _bits(want["vertices"])), (what, "vertices")
    if want["colors"] is None:
        assert got.vertex_colors is None
    else:
        assert np.array_equal(_bits(got.vertex_colors), _bits(want["colors"])), (what, "colors")


# ------------------------------------------------------------------------------------------------ 1: every output, exactly
@pytest.mark.parametrize("name,cap", TC.RUNS)
def test_repair_equals_the_restatement(name, cap):
    import surfel_repair as P
    import surfel_smooth
    v, t, c, _ = CASES[name]
    mesh = _mesh(v, t, c)
    got, stats = P.repair_mesh(mesh, max_hole_edges=cap)
    want = TC.result(name, cap)
    print("%s, cap %d: V %d, F %d, %s" % (name, cap, len(v), len(t), {k: stats[k] for k in O.COUNTS}))
    _same(got, stats, want, (name, cap))
    assert stats["label_rounds"] <= math.ceil(math.log2(max(stats["longest_loop"], 2))) + 1
    assert np.array_equal(_bits(mesh.vertices), _bits(np.asarray(v, np.float32))) and torch.equal(mesh.triangles, _t(np.asarray(t, np.int32)))
    if c is not None:
        assert np.array_equal(_bits(mesh.vertex_colors), _bits(c))      # the input is not written
    adj = surfel_smooth.mesh_adjacency(got).stats      # an independent device check
    assert adj["nonmanifold_edges"] == 0 and adj["border_edges"] == stats["border_edges_after"] and adj["dropped"] == 0
    assert adj["kept"] == stats["kept"] - stats["cut_triangles"] + stats["fill_triangles"]


def test_default_cap_and_a_cap_given_as_a_float():
    import surfel_repair as P
    v, t, c, _ = CASES["punched"]
    got, stats = P.repair_mesh(_mesh(v, t, c))
    _same(got, stats, TC.result("punched", 32), "default")
    got, stats = P.repair_mesh(_mesh(v, t, c), max_hole_edges=4.0)
    _same(got, stats, TC.result("punched", 4), "4.0")


def test_smooth_and_repair_keep_the_same_triangles():
    """rule 1 has one kernel for both modules (csrc/mesh_topology.h): on a mesh with a triangle for each way to fail it — an index below
    0, an index V, a repeated index, a NaN, a +inf and a -inf vertex, each in another coordinate — the adjacency and the repair keep the
    same two triangles, and both equal their restatements"""
    import smooth_oracle as SO
    import surfel_repair as P
    import surfel_smooth
    nan, inf = float("nan"), float("inf")
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, nan, 2], [3, 3, inf], [-inf, 4, 4]], np.float32)
    t = np.array([[0, 1, 3], [0, 1, 2], [-1, 1, 2], [1, 2, 4], [0, 1, 6], [0, 2, 1], [2, 1, 1], [2, 0, 5]], np.int32)
    V, F = len(v), len(t)
    assert (V, F) == (6, 8) and SO.kept_triangles(v, t).tolist() == [False, True, False, False, False, True, False, False]
    want_adj, want_rep = SO.adjacency(v, t)["stats"], O.repair(v, t, None, 0)["stats"]
    assert (want_adj["kept"], want_adj["dropped"]) == (want_rep["kept"], want_rep["dropped"]) == (2, 6)      # the two restatements agree
    mesh = _mesh(v, t)
    adj = surfel_smooth.mesh_adjacency(mesh).stats
    rep = P.repair_mesh(mesh, 0)[1]
    print("adjacency %s, repair %s" % (adj, {k: rep[k] for k in O.COUNTS}))
    assert (adj["kept"], adj["dropped"]) == (2, 6) and (rep["kept"], rep["dropped"]) == (2, 6)
    assert adj == want_adj and {k: rep[k] for k in O.COUNTS} == want_rep


# ------------------------------------------------------------------------------------------------ 2: border_loops
@pytest.mark.parametrize("name", ["punched", "relabelled", "clustered", "fan", "umbrellas", "cube", "no-triangle"])
def test_border_loops_agree_with_a_repair_that_fills_nothing(name):
    import surfel_repair as P
    v, t, c, _ = CASES[name]
    mesh = _mesh(v, t, c)
    loops = P.border_loops(mesh)
    want = TC.result(name, 0)
    for key in ("half_edge", "loop", "position"):
        g = getattr(loops, key)
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), want[key]), key
    assert np.array_equal(loops.lengths.cpu().numpy(), want["loop_lengths"]) and loops.stats == want["stats"]
    got, stats = P.repair_mesh(mesh, max_hole_edges=0)
    assert {k: stats[k] for k in O.COUNTS} == loops.stats and torch.equal(stats["loop_lengths"], loops.lengths)
    assert stats["filled_loops"] == 0 and stats["border_edges_after"] == stats["border_edges"] == loops.half_edge.shape[0]
    if loops.half_edge.shape[0]:      # the half-edges are those of the repaired mesh's triangles: each loop closes on itself
        he = loops.half_edge.long()
        tris = got.triangles.long()
        src, dst = tris.reshape(-1)[he], tris[he // 3, (he % 3 + 1) % 3]
        key = loops.loop.long() * (int(loops.lengths.max()) + 1)
        order = torch.argsort(key + loops.position.long())
        nxt = torch.argsort(key + (loops.position.long() + 1) % loops.lengths.long()[loops.loop.long()])
        assert torch.equal(dst[nxt], src[order])      # (nxt[i]: the half-edge one position before order[i] in its loop)


# ------------------------------------------------------------------------------------------------ 3: the same bytes
@pytest.mark.parametrize("name,cap", [("punched", 200), ("clustered", 100), ("fan", 6000)])
def test_two_runs_give_identical_bytes(name, cap):
    import surfel_repair as P
    v, t, c, _ = CASES[name]
    mesh = _mesh(v, t, c)
    timings = {}
    a, sa = P.repair_mesh(mesh, max_hole_edges=cap, timings=timings)
    torch.empty(1 << 24, dtype=torch.uint8, device=_dev()).fill_(0xA5)      # (a different history of the allocator's memory)
    junk = [torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=_dev()) for n in (1 << 12, 1 << 16, 1 << 20)]
    del junk
    b, sb = P.repair_mesh(mesh, max_hole_edges=cap)
    for x, y in ((a.vertices, b.vertices), (a.triangles, b.triangles), (a.vertex_colors, b.vertex_colors)) + \
            tuple((sa[k], sb[k]) for k in ("vertex_source", "triangle_source", "loop_lengths")):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert {k: sa[k] for k in O.COUNTS} == {k: sb[k] for k in O.COUNTS}
    assert set(timings) == {"%s_ms" % s for s in P.STAGES} and all(ms > 0 for ms in timings.values())


# ------------------------------------------------------------------------------------------------ 4: buffers respected
@pytest.mark.parametrize("name,cap", [("special", 32), ("clustered", 100), ("umbrellas", 600), ("punched", 4)])
def test_canaries_around_every_output_buffer(name, cap):
    """the six outputs of the emit entry and the four of the loops entry carved out of one allocation filled with a pattern: the pattern
    on both sides of each is intact after the calls"""
    import ctypes as C
    import surfel_native as N
    import test_gpu_smooth as TS
    v, t, c, _ = CASES[name]
    want = TC.result(name, cap)
    V, F = len(v), len(t)
    dv, dt, dc = _t(np.asarray(v, np.float32)), _t(np.asarray(t, np.int32)), (_t(c) if c is not None else None)
    plan, counts = N.RepairPlan(), (C.c_int64 * len(O.COUNTS))()
    alloc = N.TorchAllocator(_dev())
    N.call(_dev(), "surfel_repair_analyze", alloc.cb, None, V, F, dv, dt, cap, C.byref(plan), counts, None)
    assert list(counts) == [want["stats"][k] for k in O.COUNTS]
    nv, nt = plan.V + plan.split + plan.fill_vertices, plan.survivors + plan.fill_triangles
    assert (nv, nt, plan.loops, plan.border) == (len(want["vertices"]), len(want["triangles"]), len(want["loop_lengths"]), len(want["half_edge"]))
    sizes = {"verts": 12 * nv, "colors": 12 * nv, "tris": 12 * nt, "vsrc": 4 * nv, "tsrc": 4 * nt, "lengths": 4 * plan.loops,
             "half_edge": 4 * plan.border, "loop": 4 * plan.border, "position": 4 * plan.border, "lengths2": 4 * plan.loops}
    big, pattern, inside, view, off = TS._carve(sizes)
    i32, f32 = torch.int32, torch.float32
    N.call(_dev(), "surfel_repair_emit", C.byref(plan), dv, dc, view("verts", f32), view("colors", f32) if c is not None else None, view("tris", i32),
           view("vsrc", i32), view("tsrc", i32), view("lengths", i32))
    N.call(_dev(), "surfel_repair_loops", C.byref(plan), view("half_edge", i32), view("loop", i32), view("position", i32), view("lengths2", i32))
    torch.cuda.synchronize()
    if c is None:
        inside[off["colors"]:off["colors"] + sizes["colors"]] = False      # (not passed: must stay untouched)
    assert torch.equal(big[~inside], pattern[~inside]) and int((~inside).sum()) >= 11 * 4096
    assert np.array_equal(_bits(view("verts", f32)).reshape(-1, 3), _bits(want["vertices"]))
    if c is not None:
        assert np.array_equal(_bits(view("colors", f32)).reshape(-1, 3), _bits(want["colors"]))
    for key, nm in (("triangles", "tris"), ("vertex_source", "vsrc"), ("triangle_source", "tsrc"), ("loop_lengths", "lengths"),
                    ("half_edge", "half_edge"), ("loop", "loop"), ("position", "position"), ("loop_lengths", "lengths2")):
        assert np.array_equal(view(nm, i32).cpu().numpy(), want[key].reshape(-1)), key
    assert np.array_equal(_bits(dv), _bits(np.asarray(v, np.float32))) and torch.equal(dt, _t(np.asarray(t, np.int32)))


# ------------------------------------------------------------------------------------------------ 5: end to end
def test_repair_cli_writes_a_repaired_ply(tmp_path, capsys):
    import surfel_io
    import surfel_repair as P
    v, t, c, _ = CASES["punched"]
    path = str(tmp_path / "ball.ply")
    surfel_io.write_triangle_mesh(path, _mesh(v, t, c).numpy())
    loops = P.main(["--ply-path", path, "--report"])
    assert sorted(os.listdir(tmp_path)) == ["ball.ply"] and sorted(loops.lengths.cpu().tolist()) == R.punched_sphere()[3]
    text = capsys.readouterr().out
    assert "loops 5" in text and "loops of 3..3 edges: 1 (3 edges)" in text and "loops of 4..7 edges: 3 (16 edges)" in text
    assert "loops of 128..255 edges: 1 (140 edges)" in text
    out = P.main(["--ply-path", path, "--max_hole_edges", "6"])
    assert sorted(os.listdir(tmp_path)) == ["ball.ply", "ball_repaired.ply"]
    rv, rt, rc = surfel_io.read_triangle_mesh(path)      # (the file holds 8-bit colours: the CLI repairs what it read)
    sv, st, sc = surfel_io.read_triangle_mesh(str(tmp_path / "ball_repaired.ply"))
    want = O.repair(rv, rt, rc, 6)
    assert np.array_equal(_bits(sv), _bits(want["vertices"])) and np.array_equal(st, want["triangles"])
    assert np.array_equal(_bits(out.vertex_colors), _bits(want["colors"])) and want["stats"]["filled_loops"] == 4
    assert "4 of 5 loops filled" in capsys.readouterr().out


def test_mesh_cli_writes_a_repaired_mesh(tmp_path, capsys):
    """surfel_mesh.py --repair on a sphere of surfels: without the flag the file list of a run is what it was; with it fuse_post.ply is
    byte for byte the same, fuse_post_repaired.ply beside it equals repair_mesh of that file's mesh, and --smooth_iterations in the same
    run smooths the repaired mesh"""
    import surfel_io
    import surfel_mesh
    import surfel_repair as P
    import surfel_smooth
    import surfel_trainer as TR
    import test_gpu_mesh as TM
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import mesh_bench
    dev = _dev()
    model = TM._sphere_model(dev)
    cams = TR.orbit_cameras(22, 256, 192, device=dev)
    mesh_bench.write_model_dir(model, cams, str(tmp_path), 7)
    out = tmp_path / "train" / "ours_7"
    common = ["-m", str(tmp_path), "--mesh_res", "128", "--num_cluster", "1"]
    assert surfel_mesh.main(common) == 0
    assert sorted(os.listdir(out)) == ["fuse.ply", "fuse_post.ply"]
    before = open(out / "fuse_post.ply", "rb").read()
    capsys.readouterr()
    assert surfel_mesh.main(common + ["--repair", "--repair_max_hole", "40", "--smooth_iterations", "2"]) == 0
    assert sorted(os.listdir(out)) == ["fuse.ply", "fuse_post.ply", "fuse_post_repaired.ply", "fuse_post_smoothed.ply"]
    assert open(out / "fuse_post.ply", "rb").read() == before
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("mesh repaired (")]
    assert len(line) == 1 and "fuse_post_repaired.ply" in line[0]
    v, t, c = surfel_io.read_triangle_mesh(str(out / "fuse_post.ply"))
    rv, rt, rc = surfel_io.read_triangle_mesh(str(out / "fuse_post_repaired.ply"))
    want, stats = P.repair_mesh(_mesh(v, t, c), max_hole_edges=40)
    print("end to end: %d vertices, %d triangles, %s" % (len(v), len(t), {k: stats[k] for k in O.COUNTS}))
    assert len(t) > 1000 and np.array_equal(_bits(rv), _bits(want.vertices)) and np.array_equal(rt, want.triangles.cpu().numpy())
    ref = O.repair(v, t, c, 40)
    assert np.array_equal(_bits(want.vertices), _bits(ref["vertices"])) and np.array_equal(rt, ref["triangles"]) and ref["stats"] == {k: stats[k] for k in O.COUNTS}
    sv, st, _ = surfel_io.read_triangle_mesh(str(out / "fuse_post_smoothed.ply"))      # the filter ran on the repaired mesh
    smooth, _ = surfel_smooth.smooth_mesh(_mesh(rv, rt, rc), iterations=2)
    assert np.array_equal(st, rt) and np.array_equal(_bits(sv), _bits(smooth.vertices))
