"""GPU checks of the view culling (include/surfel_cull.h, CULL.md): the depth images against the fp64 ray / triangle oracle
(tests/cull_oracle.py) and against a plane in closed form, run-to-run and class-to-class identity, the visibility kernel on the depth
images of the fixture against what the reference's own point_masks computed on them (tests/golden/ref_tnt_cull.npz), cull_mesh_views end
to end, the inputs a rasteriser must skip, and guard pages.

The depth bar is not fixed here: it is four times the largest relative deviation of the oracle's fp32 twin from the fp64 oracle over the
decided pixels of the same scene (cull_oracle.twin_deviation; 2.5e-4 at 67 x 45 and 2.6e-4 at 96 x 64, so about 1e-3) — the kernel
evaluates the same fp32 formula with the division by fx, fy folded into per-triangle coefficients and with fused multiply-adds, which
reorders roundings but adds none of another size.  Undecided pixels and vertices (cull_oracle) are exempt; their shares are printed and
capped."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cull_oracle as O  # noqa: E402
import cull_scenes as S  # noqa: E402
import device_mesh  # noqa: E402
from device_mesh import dev as _dev, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ZN, ZF, EPS = S.SCENE["znear"], S.SCENE["zfar"], S.SCENE["eps"]


def _mesh(v, t, c=None):      # (a mesh without colours carries zeros here)
    return device_mesh.mesh(v, t, np.zeros((len(v), 3), np.float32) if c is None else c)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_tnt_cull.npz"))
    assert json.loads(str(z["scene"])) == json.loads(S.fingerprint())
    return z


def _depth(ref, **kw):
    import surfel_cull as P
    return P.mesh_depth(_mesh(ref["verts"], ref["tris"]), ref["w2c"], ref["intr"], ref["H"], ref["W"], ZN, ZF, **kw)


# ------------------------------------------------------------------------------------------------ 1: depth
@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_depth_matches_the_oracle(size):
    ref = O.scene_reference(size)
    got = _depth(ref).cpu().numpy()
    d64, und = ref["d64"], ref["und"]
    bar = 4 * ref["deviation"]
    ok = ~und
    wrong = ((got > 0) != (d64 > 0)) & ok
    hit = ok & (d64 > 0) & (got > 0)
    dev = np.abs(got[hit].astype(np.float64) - d64[hit]) / d64[hit]
    print("%s: coverage differs on %d decided pixels; max relative deviation %.3g (bar %.3g = 4 x %.3g); undecided share per image max %.4f %%, "
          "of which differ %d" % (size, wrong.sum(), dev.max(), bar, ref["deviation"], 100 * und.mean((1, 2)).max(), int((((got > 0) != (d64 > 0)) & und).sum())))
    assert und.mean((1, 2)).max() <= 5e-3
    assert not wrong.any(), np.argwhere(wrong)[:5]
    assert dev.max() <= bar
    assert np.isfinite(got).all() and (got >= 0).all() and ((got == 0) | ((got >= ZN) & (got <= ZF))).all()


def test_depth_matches_a_plane_in_closed_form():
    """A quad in the plane n . p = d under an identity camera: z = d / (n . ray) at every pixel; no code shared with the oracle.  The bar:
    four times the fp32 twin's deviation on this quad, plus 1e-6 for the fp32 rounding of the quad's corners (test_cull_cpu measures the
    closed form against the fp64 oracle on the rounded corners below that)."""
    import surfel_cull as P
    v, t, n, d = S.quad_anchor()
    H, W = S.SIZES["large"][:2]
    k = S.intrinsics("large")
    eye = np.eye(4, dtype=np.float32)[None]
    a64, _, u64 = O.depth_image(v, t, eye[0], k, H, W, ZN, ZF, np.float64)
    a32 = O.depth_image(v, t, eye[0], k, H, W, ZN, ZF, np.float32)[0]
    twin = O.twin_deviation(a64, a32, u64)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    want = d / (n[0] * (xs - np.float64(np.float32(k[2]))) / np.float32(k[0]) + n[1] * (ys - np.float64(np.float32(k[3]))) / np.float32(k[1]) + n[2])
    for per_view in (False, True):      # shared and per-view intrinsics
        kk = np.tile(np.asarray(k, np.float32), (2, 1)) if per_view else k
        got = P.mesh_depth(_mesh(v, t), np.concatenate([eye, eye]) if per_view else eye, kk, H, W, ZN, ZF).cpu().numpy()
        dev = np.abs(got.astype(np.float64) - want[None]) / want[None]
        print("plane: max relative deviation %.3g (bar %.3g)" % (dev.max(), 4 * twin + 1e-6))
        assert (got > 0).all() and dev.max() <= 4 * twin + 1e-6
    assert want.min() > 2 and want.max() < 5


def test_same_bits_on_two_runs_and_through_either_class():
    ref = O.scene_reference(S.FIXTURE_SIZE)
    stats = {}
    first = _depth(ref, timings=stats)
    assert stats["large_pairs"] > 100
    torch.empty(1 << 22, dtype=torch.uint8, device=_dev()).fill_(0x5A)      # (a different history of the allocator's memory)
    assert torch.equal(_depth(ref), first)
    all_large, all_small = {}, {}
    assert torch.equal(_depth(ref, small_pixels=0, timings=all_large), first)
    assert torch.equal(_depth(ref, small_pixels=1 << 30, timings=all_small), first)
    small, large = O.size_classes(ref["verts"], ref["tris"], ref["w2c"], ref["intr"], ref["H"], ref["W"], ZN, ZF)
    print("large-class pairs: %d by default (the box rule in numpy: %d), %d with the threshold 0, %d with the threshold 2^30" %
          (stats["large_pairs"], large, all_large["large_pairs"], all_small["large_pairs"]))
    assert all_small["large_pairs"] == 0 and all_large["large_pairs"] >= stats["large_pairs"] + 1000
    assert abs(stats["large_pairs"] - large) <= 0.02 * large      # (a box edge within rounding of a pixel may fall either way)


def test_skipped_inputs_change_nothing():
    """degenerate triangles, indices outside the vertices, a NaN vertex and a camera that looks away: the call completes and the images
    are those of the scene without them"""
    a, b = O.scene_reference(S.FIXTURE_SIZE), O.scene_reference(S.FIXTURE_SIZE, special=False)
    da, db = _depth(a), _depth(b)
    assert torch.equal(da, db)
    assert float(da[-1].abs().max()) == 0.0 and float(da[-2].min()) > 0.0      # looks away: nothing; the filler: every pixel
    # an empty mesh, and a mesh of skipped triangles only
    import surfel_cull as P
    none = P.mesh_depth(_mesh(a["verts"], np.zeros((0, 3), np.int32)), a["w2c"][:2], a["intr"], a["H"], a["W"])
    bad = P.mesh_depth(_mesh(a["verts"], a["tris"][-5:]), a["w2c"][:2], a["intr"], a["H"], a["W"])
    assert float(none.abs().max()) == 0.0 and float(bad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2: visibility
def test_visibility_on_the_fixture_depth(golden):
    import surfel_cull as P
    ref = O.scene_reference(S.FIXTURE_SIZE)
    v = ref["verts"]
    r = O.point_masks(v, golden["depth"], ref["w2c"], ref["intr"], 0.005, 20)
    depth = _t(golden["depth"])
    counts = P.view_counts(_t(v), depth, ref["w2c"], ref["intr"], 0.005)
    got = counts.cpu().numpy()
    clear = ~r["undecided_pairs"].any(0)
    print("fixture: counts differ on %d of %d vertices without an undecided pair; %d vertices have one (%.3f %%), %d are undecided for the mask"
          % ((got != golden["counts"])[clear].sum(), clear.sum(), (~clear).sum(), 100 * (~clear).mean(), r["undecided"].sum()))
    assert (~clear).mean() <= 5e-3 and r["undecided"].mean() <= 5e-3
    assert np.array_equal(got[clear], golden["counts"][clear])
    assert np.array_equal((got >= 20)[~r["undecided"]], golden["mask"][~r["undecided"]])
    # batches accumulate into the same array; per-view intrinsics give the same counts
    acc = torch.zeros_like(counts)
    kk = np.tile(np.asarray(ref["intr"], np.float32), (len(ref["w2c"]), 1))
    for b in range(0, len(ref["w2c"]), 7):
        P.view_counts(_t(v), depth[b:b + 7], ref["w2c"][b:b + 7], kk[b:b + 7], 0.005, acc)
    assert torch.equal(acc, counts)
    assert int(counts[-1]) == 0      # the NaN vertex counts nowhere


# ------------------------------------------------------------------------------------------------ 3: end to end
def _expected_mesh(ref, mv):
    m = ref["masks"][mv]
    v, t, c = O.compact(ref["verts"], ref["tris"], m["mask"], ref["colors"])
    return m, v, t, c


@pytest.mark.parametrize("min_views", S.MIN_VIEWS)
def test_cull_mesh_views_end_to_end(min_views):
    """oracle depth -> oracle masks -> numpy compaction against cull_mesh_views.  Triangles that touch an undecided vertex are exempt; the
    others must be the same list (compared through the original vertex ids, which the vertex order lets both sides recover)."""
    import surfel_cull as P
    ref = O.scene_reference(S.FIXTURE_SIZE)
    m, wv, wt, wc = _expected_mesh(ref, min_views)
    mesh = _mesh(ref["verts"], ref["tris"], ref["colors"])
    H, W = ref["H"], ref["W"]
    one, counts = P.cull_mesh_views(mesh, S.cameras(), ref["intr"], H, W, "opencv", min_views, EPS, ZN, ZF, return_counts=True)
    five = P.cull_mesh_views(mesh, S.cameras()[:24], ref["intr"], H, W, "opencv", min_views, EPS, ZN, ZF, budget_bytes=5 * 4 * H * W + 100)
    whole = P.cull_mesh_views(mesh, S.cameras()[:24], ref["intr"], H, W, "opencv", min_views, EPS, ZN, ZF)
    gl = P.cull_mesh_views(mesh, S.cameras_opengl(), ref["intr"], H, W, "opengl", min_views, EPS, ZN, ZF)
    for a, b in ((five, whole), (gl, one)):      # 5 + 5 + 5 + 5 + 4 views as one batch of 24; OpenGL poses as their OpenCV twins
        assert torch.equal(a.vertices, b.vertices, ) and torch.equal(a.triangles, b.triangles) and torch.equal(a.vertex_colors, b.vertex_colors)
    got_counts = counts.cpu().numpy()
    clear = ~m["undecided_pairs"].any(0)
    und = m["undecided"]
    print("min_views %d: kept %d of %d vertices, %d of %d triangles; %d undecided vertices, %d with an undecided pair; counts differ on %d clear ones"
          % (min_views, one.vertices.shape[0], len(ref["verts"]), one.triangles.shape[0], len(ref["tris"]), und.sum(), (~clear).sum(),
             (got_counts != m["counts"])[clear].sum()))
    assert und.mean() <= 5e-3
    # The kernel's depth differs from the oracle's within the depth bar, so a pair may flip where that moves z - (sample + eps) across 0:
    # the oracle's 1e-4 margin covers a bar of 1e-3 times the eps-scale differences only in part, hence the comparison is on the mask.
    keep = (got_counts >= min_views)
    assert np.array_equal(keep[~und], m["mask"][~und])
    # the triangle list through original ids
    tt = ref["tris"].astype(np.int64)
    inside = ((tt >= 0) & (tt < len(ref["verts"]))).all(1)
    touched = np.zeros(len(tt), bool)
    touched[inside] = und[tt[inside]].any(1)
    want_ids = np.nonzero(inside & ~touched)[0]
    want_ids = want_ids[m["mask"][tt[want_ids]].all(1)]
    got_v, got_t, got_c = one.vertices.cpu().numpy(), one.triangles.cpu().numpy(), one.vertex_colors.cpu().numpy()
    used = np.zeros(len(ref["verts"]), bool)
    kept_t = tt[inside][keep[tt[inside]].all(1)]
    used[kept_t.reshape(-1)] = True
    orig = np.nonzero(used)[0]      # the original id of every output vertex: order is kept
    assert len(orig) == len(got_v) and np.array_equal(got_v, ref["verts"][orig], equal_nan=True) and np.array_equal(got_c, ref["colors"][orig])
    got_orig = orig[got_t]
    got_clear = got_orig[~und[got_orig].any(1)]
    assert np.array_equal(got_clear, tt[want_ids])
    if not und.any():
        assert np.array_equal(got_t, wt) and np.array_equal(got_v, wv, equal_nan=True) and np.array_equal(got_c, wc)


def test_cameras_of_two_sizes_share_one_count():
    """cull_mesh_cameras (the -m path): views grouped by size give the counts of the two sizes added"""
    import surfel_cull as P
    a, b = O.scene_reference("small"), O.scene_reference("large")
    mesh = _mesh(a["verts"], a["tris"], a["colors"])
    cams = [(c, a["intr"], a["H"], a["W"]) for c in S.cameras()[:6]] + [(c, b["intr"], b["H"], b["W"]) for c in S.cameras()[6:12]]
    out = P.cull_mesh_cameras(mesh, cams, min_views=8)
    ca = P.view_counts(mesh.vertices, P.mesh_depth(mesh, a["w2c"][:6], a["intr"], a["H"], a["W"]), a["w2c"][:6], a["intr"])
    cb = P.view_counts(mesh.vertices, P.mesh_depth(mesh, b["w2c"][6:12], b["intr"], b["H"], b["W"]), b["w2c"][6:12], b["intr"])
    inside = ((mesh.triangles >= 0) & (mesh.triangles < mesh.vertices.shape[0])).all(1)
    want = P.TriangleMesh(*P._e.compact_kept(mesh.vertices, mesh.triangles.long()[inside], (ca + cb) >= 8, mesh.vertex_colors))
    assert torch.equal(out.triangles, want.triangles) and torch.equal(out.vertices, want.vertices) and 0 < out.triangles.shape[0] < inside.sum()


# ------------------------------------------------------------------------------------------------ 4: guard pages
def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "cull_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "cull_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 4, p.stdout


# ------------------------------------------------------------------------------------------------ 5: the command line
def test_command_line_from_npy_and_json(tmp_path):
    """python surfel_cull.py on the fixture mesh: a .npy trajectory gives cull_mesh_views' mesh; a transforms .json is read, oriented and
    used (its poses are not this scene's, so only the file it writes is checked)."""
    import surfel_cull as P
    import surfel_io
    ref = O.scene_reference(S.FIXTURE_SIZE)
    mesh = _mesh(ref["verts"], ref["tris"], ref["colors"])
    ply = str(tmp_path / "mesh.ply")
    surfel_io.write_triangle_mesh(ply, mesh)
    np.save(str(tmp_path / "traj.npy"), S.cameras_opengl())
    with open(str(tmp_path / "transforms.json"), "w") as f:
        json.dump(S.transforms_json(), f)
    H, W = ref["H"], ref["W"]
    fx, fy, cx, cy = ref["intr"]
    size = ["--height", str(H), "--width", str(W), "--fx", repr(fx), "--fy", repr(fy), "--cx", repr(cx), "--cy", repr(cy)]
    out = P.main(["--traj-path", str(tmp_path / "traj.npy"), "--ply-path", ply, "--min_views", "3"] + size)
    v, t, c = surfel_io.read_triangle_mesh(str(tmp_path / "mesh_cull.ply"))
    # the .ply stores 8-bit colours and drops nothing else; the mesh that went in had its bad triangles written out as they were
    v0, t0, _ = surfel_io.read_triangle_mesh(ply)
    want = P.cull_mesh_views(_mesh(v0, t0), S.cameras_opengl(), ref["intr"], H, W, "opengl", 3)
    assert np.array_equal(t, want.triangles.cpu().numpy()) and np.array_equal(v, want.vertices.cpu().numpy(), equal_nan=True)
    assert 0 < len(t) == out.triangles.shape[0] < len(t0)
    os.remove(str(tmp_path / "mesh_cull.ply"))
    P.main(["--traj-path", str(tmp_path / "transforms.json"), "--ply-path", ply, "--min_views", "1", "--convention", "opengl"] + size)
    v, t, c = surfel_io.read_triangle_mesh(str(tmp_path / "mesh_cull.ply"))
    assert len(t) <= len(t0) and (len(t) == 0 or t.max() == len(v) - 1)
    with pytest.raises(SystemExit):
        P.main(["--ply-path", ply])
