"""GPU checks of the Tanks-and-Temples-style evaluation (include/surfel_eval_tnt.h, TNT.md) against the numpy oracle
(tests/tnt_oracle.py) and against what the reference's run.py computed on the fixture scene (tests/golden/ref_tnt.npz).
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import tnt_oracle as O  # noqa: E402
import tnt_scenes as S  # noqa: E402
import device_mesh  # noqa: E402
from device_mesh import dev as _dev, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = S.FIXTURE["tau"]
# Bar on max |T_ours q - T_ref q| over the ground-truth points of the fixture, ours against the golden's final transform.  The hard
# condition is tau / 100 = 1e-4, one histogram bin.  Measured on an MI355X: 7.3e-10 with the default criteria (one, one and three updates)
# and 5.9e-7 with relative_rmse = 1e-6 (12, 9 and 2 updates); the bar is ten times the larger.
MEASURED_DISPLACEMENT = 5.9e-7
DISPLACEMENT_BAR = 10 * MEASURED_DISPLACEMENT


def _mesh(v, t):      # (zeros for colours)
    return device_mesh.mesh(v, t, np.zeros((len(v), 3), np.float32))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_tnt.npz"))
    assert json.loads(str(z["scene"])) == json.loads(json.dumps(S.FIXTURE)) and json.loads(str(z["cases"])) == json.loads(json.dumps(S.CASES))
    return z


# ------------------------------------------------------------------------------------------------ 1: crop
def test_crop_matches_the_oracle_exactly():
    """Both sides decide in fp64 on the same fp32 coordinates in the same operation order: the masks are identical, no exemption."""
    import surfel_eval_tnt as P
    for axis in ("X", "Y", "Z"):
        fields, pts = S.crop_case(axis)
        assert len(pts) > 50000
        want = O.crop_mask(pts, O.CropVolume(**fields))
        vol = P.CropVolume(**fields)
        got = P.crop(_t(pts), vol, return_mask=True).cpu().numpy()
        assert np.array_equal(got, want), (axis, int((got != want).sum()))
        assert 0.15 < want.mean() < 0.6 and want[50000:].any() and not want[50000:].all()
        kept = P.crop(_t(pts), vol).cpu().numpy()
        assert np.array_equal(kept, pts[want])
    big = P.CropVolume("Z", 0, 1, np.concatenate([np.stack([np.cos(a := np.linspace(0, 6.28, 1025)), np.sin(a)], 1), np.zeros((1025, 1))], 1))
    with pytest.raises(P.MeshLimitError):
        P.crop(_t(pts), big)
    ok = P.CropVolume("Z", -1, 1, big.bounding_polygon[:1024])
    assert np.array_equal(P.crop(_t(pts), ok, return_mask=True).cpu().numpy(), O.crop_mask(pts, O.CropVolume("Z", -1, 1, ok.bounding_polygon)))


# ------------------------------------------------------------------------------------------------ 2: voxel down-sampling
def _lattice_cloud():
    """399 points in the 300 cells (x, y, z), x, y < 10, z < 2, and (x, y + 2048, 0) at voxel 1 (a third of the cells holds two points;
    the first point is the minimum corner, so the origin is 0)."""
    rng = np.random.default_rng(22)
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    cells = np.concatenate([g, g[g[:, 2] == 0] + [0, 2048, 0]])
    cells = np.concatenate([cells, cells[::3][1:]])
    pts = cells + rng.uniform(0.5, 0.95, size=cells.shape)
    pts[0] = 0.5
    return np.concatenate([pts[:1], pts[1:][rng.permutation(len(pts) - 1)]]).astype(np.float32)


def _voxel_cases():
    rng = np.random.default_rng(21)
    yield "random, negative coordinates", rng.uniform(-3, 2, size=(20000, 3)).astype(np.float32), 0.1
    # voxel 2^-6, the cloud's minimum corner at 0: odd multiples of 2^-7 lie exactly on cell faces ((p - origin) / voxel is an integer)
    faces = np.concatenate([np.zeros((1, 3)), rng.integers(0, 200, size=(6000, 3)) * 2.0 ** -7]).astype(np.float32)
    yield "points on cell faces", faces, 2.0 ** -6
    # two clusters 1500 apart along every axis at voxel 2^-10: 1.5 M cells per axis, a key far beyond 32 bits
    far = np.concatenate([rng.uniform(0, 0.5, size=(3000, 3)), rng.uniform(0, 0.5, size=(3000, 3)) + 1500.0]).astype(np.float32)
    yield "two clusters, 63-bit keys", far[rng.permutation(len(far))], 2.0 ** -10
    # cells (x, y, z), (x, y, z + 1) and (x, y + 2048, z) share the key's low word (x and the low 11 bits of y) and differ in every part
    # of its high word: the second sort pass alone orders them, and it has to keep the first pass's order inside a cell
    yield "lattice, equal low words", _lattice_cloud(), 1.0
    yield "one point", np.array([[1.5, -2.0, 3.0]], np.float32), 0.25
    yield "empty", np.zeros((0, 3), np.float32), 0.25
    yield "100 000 points in one cell", (rng.uniform(0, 1, size=(100000, 3)) * 0.01 + [5.0, 6.0, -7.0]).astype(np.float32), 1.0
    # the run heads are scanned over n + 1 elements (the last one holds the cell count): one full scan tile of 4 096, and one element more
    yield "4 095 points", rng.uniform(-1, 1, size=(4095, 3)).astype(np.float32), 0.1
    yield "4 096 points", rng.uniform(-1, 1, size=(4096, 3)).astype(np.float32), 0.1


def test_voxel_down_sample_matches_the_oracle():
    """Occupied cells, their order and the counts per cell are the oracle's exactly; the means differ by the one rounding of the fp32 store,
    2^-24 max|coordinate|; two runs give the same bits."""
    import surfel_eval_tnt as P
    for name, pts, voxel in _voxel_cases():
        want, wcounts, wcells = O.voxel_down_sample(pts, voxel)
        got, counts, cells = P.voxel_down_sample(_t(pts), voxel, return_counts=True, return_cells=True)
        again = P.voxel_down_sample(_t(pts), voxel)
        assert got.shape[0] == len(want), (name, got.shape[0], len(want))
        assert np.array_equal(cells.cpu().numpy(), wcells) and np.array_equal(counts.cpu().numpy(), wcounts), name
        assert torch.equal(got, again), name
        if len(pts):
            err, bound = np.abs(got.cpu().numpy().astype(np.float64) - want).max(), 2.0 ** -24 * np.abs(pts).max()
            print("voxel (%s): %d points -> %d cells, max |dmean| = %.3g (bound %.3g)" % (name, len(pts), len(want), err, bound))
            assert err <= bound, name
            key = (wcells[:, 2].astype(object) << 42) | (wcells[:, 1].astype(object) << 21) | wcells[:, 0].astype(object)
            assert all(key[i] < key[i + 1] for i in range(len(key) - 1))
            if "63-bit" in name:
                assert max(key) >= 1 << 32 and wcells.max() > 1 << 20
            if "low words" in name:
                assert len(want) == 300 and len({int(k) & 0xFFFFFFFF for k in key}) == 100 and wcells[:, 1].max() >= 2048 and wcounts.max() == 2
            if "one cell" in name:
                assert len(want) == 1 and wcounts[0] == 100000
            if "faces" in name:
                onface = ((pts.astype(np.float64) + voxel / 2) / voxel % 1 == 0).any(axis=1)
                assert onface.mean() > 0.5
    # two clusters 4000 apart at voxel 2^-10 (the case first asked for) need 4.1 M cells along an axis: beyond the 21 bits an axis has, a SURFEL_E_LIMIT
    far = np.array([[0, 0, 0], [4000, 0, 0]], np.float32)
    with pytest.raises(P.MeshLimitError, match="SURFEL_TNT_VOXEL_AXIS_BITS"):
        P.voxel_down_sample(_t(far), 2.0 ** -10)
    with pytest.raises(P.MeshLimitError, match="budget"):
        P.voxel_down_sample(_t(np.zeros((1000, 3), np.float32)), 1.0, budget_bytes=1000)


# ------------------------------------------------------------------------------------------------ 3: the cloud of a mesh
def test_mesh_cloud_matches_the_oracle():
    import surfel_eval_tnt as P
    rng = np.random.default_rng(22)
    v = (rng.normal(size=(1203, 3)) * 3 + [10, -20, 5]).astype(np.float32)
    t = rng.integers(0, 1200, size=(2000, 3)).astype(np.int32)       # vertices 1200 .. 1202 are referenced by no triangle
    t[7] = [5, 5, 9]                                                  # zero area
    t[8] = [4, 4, 4]
    want = O.mesh_cloud(v, t)
    got = P.mesh_cloud(_mesh(v, t)).cpu().numpy()
    assert got.shape == (1203 + 2000, 3) and np.array_equal(got[:1203], v)
    err = np.abs(got.astype(np.float64) - want).max()
    print("mesh cloud: max |dp| = %.3g (bound %.3g)" % (err, 2.0 ** -24 * np.abs(want).max()))
    assert err <= 2.0 ** -24 * np.abs(want).max()
    assert np.array_equal(got[1203 + 8], v[4])
    bad = t.copy()
    bad[3, 1] = 5000
    assert np.isnan(P.mesh_cloud(_mesh(v, bad)).cpu().numpy()[1203 + 3]).all()
    assert P.mesh_cloud(_mesh(v[:0], t[:0])).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 4: one ICP evaluation and one update
def test_icp_evaluation_and_update():
    import surfel_eval_tnt as P
    src, tgt, T, thr = S.icp_pair()
    fit, rmse, sums, moved, index = P.icp_evaluate(_t(src), _t(tgt), T, thr, return_index=True)
    fit2, rmse2, sums2 = P.icp_evaluate(_t(src), _t(tgt), T, thr)
    assert (fit, rmse) == (fit2, rmse2) and np.array_equal(sums, sums2)                      # the same bits on every run
    mv = moved.cpu().numpy()
    exact = O.transform(src, T)
    assert np.abs(mv.astype(np.float64) - exact).max() <= 2.0 ** -24 * np.abs(exact).max()
    # the correspondence set, for the queries the kernel saw (the fp32 moved source)
    d, i = O.nearest(mv, tgt, k=2)
    margin = 2.0 ** -22 * np.ptp(tgt.astype(np.float64), axis=0).max()
    exempt = (d[:, 1] - d[:, 0] < margin) | (np.abs(d[:, 0] - thr) < margin)
    want = np.where(d[:, 0] < thr, i[:, 0], -1)
    got = index.cpu().numpy()
    print("icp evaluation: fitness %.4f, %d of %d queries exempt (%.4f %%), %d of them differ" % (fit, exempt.sum(), len(src), 100.0 * exempt.mean(),
                                                                                                 (got != want)[exempt].sum()))
    assert exempt.mean() <= 1e-3
    assert np.array_equal(got[~exempt], want[~exempt])
    assert 0.5 < fit < 0.999 and abs(fit - (want >= 0).mean()) <= exempt.mean()
    # the sums, on the oracle's own correspondence set
    osums = O.correspondence_sums(mv, want, tgt)
    gsums = P.correspondence_sums(moved, _t(want.astype(np.int32)), _t(tgt))
    rel = np.abs(gsums - osums) / np.abs(osums)
    print("icp sums: max relative difference %.3g" % rel.max())
    assert gsums[0] == osums[0] and rel.max() < 1e-12
    assert np.array_equal(gsums, P.correspondence_sums(moved, _t(want.astype(np.int32)), _t(tgt)))
    # one update from them
    assert np.abs(P.umeyama_from_sums(gsums) - O.umeyama_from_sums(osums)).max() < 1e-9
    # index -1 everywhere and an empty source
    none = P.correspondence_sums(moved, torch.full((len(src),), -1, dtype=torch.int32, device=_dev()), _t(tgt))
    assert np.array_equal(none, np.zeros(18))
    r = P.icp_similarity(_t(src[:0]), _t(tgt), thr)
    assert r["fitness"] == 0 and r["iterations"] == 0 and np.array_equal(r["transformation"], np.eye(4))
    far = P.icp_similarity(_t(src[:100] + 50), _t(tgt), thr, S.truth())
    assert far["fitness"] == 0 and far["iterations"] == 0 and np.array_equal(far["transformation"], S.truth())


# ------------------------------------------------------------------------------------------------ 5: the ICP loop
@pytest.fixture(scope="module")
def fixture_runs(golden):
    import surfel_eval_tnt as P
    v, t = S.mesh()
    mesh, gt, vol = _mesh(v, t), _t(S.ground_truth()), P.CropVolume(**S.crop_fields())
    return [P.evaluate_tnt(mesh, gt, vol, TAU, init_transform=golden["trajectory"][k], **case) for k, case in enumerate(S.CASES)]


def test_icp_loop_on_the_fixture(golden, fixture_runs):
    gt = S.ground_truth().astype(np.float64)
    for k, r in enumerate(fixture_runs):
        its = [s["iterations"] for s in r["stages"]]
        disp = np.abs(O.transform(gt, r["transformation"]) - O.transform(gt, golden["final"][k])).max()
        print("case %d: iterations %s (golden %s), max displacement against the golden %.3g, sizes %s (golden %s)"
              % (k, its, golden["stage_sizes"][k, :, 2].tolist(), disp, [(s["source"], s["target"]) for s in r["stages"]], golden["stage_sizes"][k, :, :2].tolist()))
        assert its == golden["stage_sizes"][k, :, 2].tolist()
        assert disp < TAU / 100
        assert disp < DISPLACEMENT_BAR
        assert [s["target"] for s in r["stages"]] == golden["stage_sizes"][k, :, 1].tolist()      # the ground truth is not moved: exact


def test_scores_on_the_fixture(golden, fixture_runs):
    """Precision and recall against the golden.  Our transform lies within tau / 100 of the golden's (the test above), so a distance moves
    by less than one histogram bin and can change sides of tau only from the bins next to it: |dP| is at most the golden curve's rise over
    the three bins around tau (and the same for R).  The curves are compared with one bin of slack in the same way."""
    for k, r in enumerate(fixture_runs):
        gp, gr, gf = golden["prf"][k][:3]
        cs, ct = golden["cum_source"][k], golden["cum_target"][k]
        bp, br = cs[101] - cs[98], ct[101] - ct[98]
        print("case %d: P %.5f R %.5f F %.5f (golden %.5f %.5f %.5f; bounds %.4f %.4f)" % (k, r["precision"], r["recall"], r["fscore"], gp, gr, gf, bp, br))
        assert abs(r["precision"] - gp) <= bp and abs(r["recall"] - gr) <= br
        assert abs(r["fscore"] - 2 * r["precision"] * r["recall"] / (r["precision"] + r["recall"])) < 1e-15
        assert r["cum_source"].shape == (499,) and r["edges"].shape == (500,)
        for ours, ref in ((r["cum_source"], cs), (r["cum_target"], ct)):
            assert np.all(ours[1:-1] <= ref[2:] + 1e-3) and np.all(ours[1:-1] >= ref[:-2] - 1e-3)
        assert abs(r["source"] - golden["scored"][k][0]) <= golden["scored"][k][0] // 100 and r["target"] == golden["scored"][k][1]


def test_icp_analytic_anchor():
    """A source that is an exact subset of the target, moved by a known similarity and started 1 degree / 0.01 away: with
    relative_rmse = 1e-6 the loop recovers the similarity to within tau / 100."""
    import surfel_eval_tnt as P
    src, tgt, init, T = S.anchor_pair()
    r = P.icp_similarity(_t(src), _t(tgt), 2 * TAU, init, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30)
    q = tgt.astype(np.float64)
    err = np.abs(O.transform(q, r["transformation"]) - O.transform(q, T)).max()
    start = np.abs(O.transform(q, init) - O.transform(q, T)).max()
    print("anchor: %d updates, fitness %.4f, rmse %.3g, error %.3g (start %.3g)" % (r["iterations"], r["fitness"], r["inlier_rmse"], err, start))
    assert start > 0.01 and r["iterations"] >= 2 and r["fitness"] == 1.0
    assert err < TAU / 100


# ------------------------------------------------------------------------------------------------ 6: the histogram
def test_histogram_matches_numpy():
    import surfel_eval_tnt as P
    rng = np.random.default_rng(23)
    for tau in (0.01, 0.003):
        edges = np.arange(0, 5 * tau, tau / 100)
        e32 = edges.astype(np.float32)
        d = np.concatenate([rng.uniform(0, 6 * tau, 200000 - 6 * len(edges) - 8), e32, np.nextafter(e32, np.float32(0)), np.nextafter(e32, np.float32(1)),
                            e32, e32, e32, [edges[-1], np.inf, np.inf, 0.0, 7 * tau, tau, np.nextafter(np.float32(tau), np.float32(0)), np.nan]]).astype(np.float32)
        assert len(d) == 200000
        fin = d[~np.isnan(d)]
        want = np.histogram(fin, edges)[0]
        hist, below = P.histogram(_t(d), edges, tau)
        assert np.array_equal(hist, want) and np.array_equal(hist, O.histogram(fin, edges))
        assert below == int((fin.astype(np.float64) < tau).sum()) and hist.sum() < len(d) - 30000
    s = P.score(_t(d[:0]), _t(d), 0.01)
    assert (s["precision"], s["recall"], s["fscore"]) == (0.0, 0.0, 0.0)
    with pytest.raises(P.MeshLimitError):
        P.histogram(_t(d), np.arange(2049.0), 1.0)


# ------------------------------------------------------------------------------------------------ 7: the command line
def test_cli_end_to_end(tmp_path, golden):
    """The CLI on the fixture written out as a Tanks-and-Temples directory: the trajectory alignment reproduces the golden's, the files the
    reference writes are there, and the coloured clouds carry hot_r."""
    import surfel_eval_tnt as P
    import surfel_io
    from types import SimpleNamespace
    d = tmp_path / "Barn"
    d.mkdir()
    surfel_io.write_ply(str(d / "Barn.ply"), ["x", "y", "z"], S.ground_truth())
    P.write_crop_volume(str(d / "Barn.json"), P.CropVolume(**S.crop_fields()))
    est, col = S.cameras()
    P.write_trajectory_log(str(d / "Barn_COLMAP_SfM.log"), col)
    np.savetxt(str(d / "Barn_trans.txt"), S.alignment())
    np.save(str(tmp_path / "traj.npy"), est)
    v, t = S.mesh()
    surfel_io.write_triangle_mesh(str(tmp_path / "mesh.ply"), SimpleNamespace(vertices=v, triangles=t, vertex_colors=np.zeros_like(v)))
    out = tmp_path / "out"
    res = P.main(["--dataset-dir", str(d), "--traj-path", str(tmp_path / "traj.npy"), "--ply-path", str(tmp_path / "mesh.ply"), "--out-dir", str(out)])
    assert np.abs(np.asarray(res["trajectory"]["transformation"]) - golden["trajectory"][0]).max() < 1e-9
    assert [s["iterations"] for s in res["stages"]] == golden["stage_sizes"][0, :, 2].tolist()
    prf = np.loadtxt(str(out / "Barn.prf_tau_plotstr.txt"))
    assert prf.tolist() == [res["precision"], res["recall"], res["fscore"], 0.01, 5.0]
    assert np.array_equal(np.loadtxt(str(out / "Barn.precision.txt")), res["cum_source"]) and np.loadtxt(str(out / "Barn.recall.txt")).shape == (499,)
    js = json.load(open(str(out / "results.json")))
    assert js["fscore"] == res["fscore"] and np.array(js["transformation"]).shape == (4, 4) and len(js["stages"]) == 3
    pv, _, pc = surfel_io.read_triangle_mesh(str(out / "Barn.precision.ply"))
    assert len(pv) == res["source"] and np.array_equal(pv, res["source_cloud"].cpu().numpy())
    x = (res["distance1"].clamp(max=0.03) / 0.03).cpu().numpy()
    assert np.abs(pc - P.hot_r(x)).max() <= 0.5 / 255 + 1e-6                                  # the 8-bit store of a .ply
    assert np.abs(pc - O.hot(1 - x.astype(np.float64))).max() <= 0.5 / 255 + (1 / (1 - 0.746032)) / 256 + 1e-6      # the ramps, up to the table's step
    assert len(surfel_io.read_triangle_mesh(str(out / "Barn.recall.ply"))[0]) == res["target"]
