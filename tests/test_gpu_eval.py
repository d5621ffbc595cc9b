"""GPU checks of the mesh evaluation (include/surfel_eval.h, EVAL.md) against the numpy oracle (tests/eval_oracle.py), against what the
reference's eval.py computed on the fixture scene (tests/golden/ref_eval.npz) and end to end on the project's own mesh.
"""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import eval_oracle as O  # noqa: E402
import eval_scenes as S  # noqa: E402
import device_mesh  # noqa: E402
from device_mesh import dev as _dev, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Bar on the same-seed |ours - reference| of a mean on the fixture.  The first bar is the reference against itself: its seed-to-seed
# spread, 7.8e-5 .. 1.3e-4 (checked below to lie above this bar).  Measured on an MI355X: 1.2e-9 .. 1.6e-8 with max_dist = 20, and
# 7.0e-7 once with max_dist = 0.4, where one fp32 distance of 44 524 crossed the cut-off.  That is two orders below the spread, so the
# bar is ten times the largest measured difference.
SAME_SEED_BAR = 7e-6


def _mesh(v, t):      # (zeros for colours)
    return device_mesh.mesh(v, t, np.zeros((len(v), 3), np.float32))


@pytest.fixture(scope="module")
def fixture_scene():
    import surfel_eval
    v, t = S.fixture_mesh()
    pts, counts = surfel_eval.sample_mesh(_mesh(v, t), S.PARAMS[0]["density"], return_counts=True)
    return v, t, pts, counts


@pytest.fixture(scope="module")
def sphere_extraction():
    import surfel_mesh
    import test_gpu_mesh as TM
    ext, mesh, voxel = TM._extract_sphere()
    return surfel_mesh.post_process_mesh(mesh, 1), voxel


# ------------------------------------------------------------------------------------------------ sampling
def _check_sampling(v, t, density, pts, counts):
    opts, ocounts = O.sample_mesh(v, t, density)
    assert np.array_equal(counts.cpu().numpy(), ocounts)
    assert pts.shape[0] == len(opts) == len(v) + ocounts.sum()
    got = pts.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:len(v)], v.astype(np.float64))
    # the kernel repeats the oracle's fp64 operations one for one (no contraction; IEEE division and square root), so the positions
    # differ by the one rounding of the fp64 result to fp32: half an ulp, 2^-24 relative, of a value no larger than max|coordinate|
    err = np.abs(got - opts).max()
    print("sampling: %d triangles, %d samples, max |dp| = %.3g (bound %.3g)" % (len(t), ocounts.sum(), err, 2.0 ** -24 * np.abs(opts).max()))
    assert err <= 2.0 ** -24 * np.abs(opts).max()


def test_sampling_fixture(fixture_scene):
    v, t, pts, counts = fixture_scene
    _check_sampling(v, t, S.PARAMS[0]["density"], pts, counts)
    c = counts.cpu().numpy()
    assert c[-4] == 0 and c[-3] == 0 and c[-2] > 1000 and c[-1] > 30      # zero area, sliver, n = 51, n = 10


def test_sampling_extracted_sphere(sphere_extraction):
    import surfel_eval
    mesh, voxel = sphere_extraction
    pts, counts = surfel_eval.sample_mesh(mesh, voxel / 2, return_counts=True)
    _check_sampling(mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), voxel / 2, pts, counts)


# ------------------------------------------------------------------------------------------------ thinning
def _check_thinning(pts, density, seeds):
    import surfel_eval
    p = pts.cpu().numpy()
    pairs = O.radius_pairs(p, density, f32=True)
    out = {}
    for seed in seeds:
        keep, rounds = surfel_eval.thin(pts, density, seed, return_rounds=True)
        want = O.thin_sequential(len(p), pairs, O.shuffle_order(len(p), seed))
        k = keep.cpu().numpy()
        print("thinning: seed %s: %d of %d kept, %d rounds" % (seed, k.sum(), len(p), rounds))
        assert np.array_equal(k, want), (seed, int((k != want).sum()))
        again = surfel_eval.thin(pts, density, seed)
        assert again.cpu().numpy().tobytes() == k.tobytes()
        out[seed] = (k, rounds)
    return out


def test_thinning_fixture(fixture_scene):
    v, t, pts, counts = fixture_scene
    r = _check_thinning(pts, S.PARAMS[0]["density"], (0, 1, 2))
    assert all(0.5 * len(pts) < k.sum() < 0.8 * len(pts) for k, _ in r.values())


def test_thinning_clusters():
    density = 0.2
    cloud = S.cluster_cloud(density)
    r = _check_thinning(_t(cloud), density, (0, 1, 2, None))
    k, rounds = r[None]
    assert k[:1000].sum() == 1 and k[0]                       # the blob: its first point
    assert np.array_equal(k[1000:1200], np.arange(200) % 2 == 0)      # the chain in input order: every other point
    assert rounds <= 202                                      # one decision per round at worst, plus the round that finds nothing
    for seed in (0, 1, 2):
        assert r[seed][0][:1000].sum() == 1


# ------------------------------------------------------------------------------------------------ nearest neighbour
def test_nearest_against_brute_force():
    import surfel_eval
    L, max_dist = 100.0, 5.0
    rng = np.random.default_rng(0)
    q = rng.uniform(0, L, size=(20000, 3)).astype(np.float32)
    c = (rng.uniform(0, L, size=(30000, 3)) * [1.0, 1.0, 0.6]).astype(np.float32)      # nothing above z = 60: queries beyond 65 find none
    want = O.nearest(q, c)
    assert np.array_equal(want[:300], O.nearest_exact(q[:300], c))
    # fp32 on re-based coordinates: the re-basing rounds every coordinate of query and point once (<= 2^-24 L each), the difference
    # once (2^-24 d): the vector moves by sqrt(3) 2^-24 (2 L + d); three products, two sums (relative 3 x 2^-24 on d^2 = 1.5 x 2^-24 on d)
    # and the root (2^-24): 2.5 x 2^-24 d.  Together below 4.5 x 2^-24 (L + d).
    bound = 4.5 * 2.0 ** -24 * (L + want)
    edge = np.abs(want - max_dist) <= bound
    assert edge.sum() <= 2, edge.sum()                        # the fp64 brute force itself puts (far) fewer than 0.1 % there
    got, idx = surfel_eval.nearest(_t(q), _t(c), max_dist, return_index=True)
    got, idx = got.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    none = np.isinf(got)
    assert np.array_equal(none[~edge], (want >= max_dist)[~edge])
    assert 0.2 < none.mean() < 0.5
    hit = ~none
    err = np.abs(got[hit] - want[hit])
    print("nearest: %d hits, max |dd| / bound = %.3f" % (hit.sum(), (err / bound[hit]).max()))
    assert np.all(err <= bound[hit])
    assert np.all(idx[none] == -1) and np.all(idx[hit] >= 0)
    assert np.all(np.abs(np.linalg.norm(q[hit].astype(np.float64) - c[idx[hit]], axis=1) - want[hit]) <= 2 * bound[hit])
    full = surfel_eval.nearest(_t(q[:2000]), _t(c)).cpu().numpy()     # no cut-off: every query has a neighbour
    assert np.all(np.abs(full - want[:2000]) <= bound[:2000])
    assert surfel_eval.nearest(_t(q), _t(c), max_dist).cpu().numpy().tobytes() == got.astype(np.float32).tobytes()


def test_nearest_edge_cases():
    import surfel_eval
    q = _t(np.random.default_rng(1).uniform(-1, 1, size=(500, 3)).astype(np.float32))
    empty = torch.zeros((0, 3), device=_dev())
    assert surfel_eval.nearest(empty, q).shape == (0,)
    d, i = surfel_eval.nearest(q, empty, return_index=True)
    assert torch.isinf(d).all() and (i == -1).all()
    one = _t(np.array([[0.25, -0.5, 2.0]], np.float32))
    d = surfel_eval.nearest(q, one).cpu().numpy()
    assert np.allclose(d, np.linalg.norm(q.cpu().numpy() - one.cpu().numpy(), axis=1), rtol=1e-6)
    same = one.repeat(300, 1)
    d2, i2 = surfel_eval.nearest(q, same, return_index=True)
    assert np.array_equal(d2.cpu().numpy(), d) and (i2 >= 0).all()
    assert surfel_eval.nearest(one, same).item() == 0.0
    f = surfel_eval.fscore(d2, torch.full((4,), math.inf, device=_dev()), 10.0)
    assert f == dict(precision=1.0, recall=0.0, fscore=0.0)
    assert math.isnan(surfel_eval.mean_below(torch.full((4,), math.inf, device=_dev()), 1.0))


# ------------------------------------------------------------------------------------------------ end to end against the reference
def test_end_to_end_against_reference(fixture_scene):
    import surfel_eval
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_eval.npz"))
    assert json.loads(str(z["scene"])) == json.loads(json.dumps(S.FIXTURE))
    names = [str(x) for x in z["size_names"]]
    v, t, _, _ = fixture_scene
    mesh, stl = _mesh(v, t), _t(S.fixture_ground_truth())
    mask, bb, res, plane = S.fixture_obs()
    mask = _t(mask)
    worst = 0.0
    for a, p in enumerate(S.PARAMS):
        spread = np.ptp(z["means"][a], axis=0)                 # the largest |ref(seed a) - ref(seed b)|
        bar = SAME_SEED_BAR
        assert np.all(bar < spread)
        for b, seed in enumerate(S.SEEDS):
            r = surfel_eval.evaluate_dtu(mesh, stl, mask, bb, res, plane, mode="mesh", seed=int(seed), **p)
            ref = dict(zip(names, z["sizes"][a, b]))
            assert r["data_pcd"] == ref["data_pcd"] and r["stl_above"] == ref["stl_above"]
            for k in ("data_down", "data_in", "data_in_obs"):
                assert abs(r[k] - ref[k]) <= ref[k] // 1000, (p, seed, k, r[k], ref[k])
            got = np.array([r["mean_d2s"], r["mean_s2d"], r["overall"]])
            diff = np.abs(got - z["means"][a, b])
            worst = max(worst, diff.max())
            print("set %d seed %d: sizes %s (reference %s), |ours - ref| = %s, reference seed spread = %s, rounds %d"
                  % (a, seed, [r[k] for k in names], list(z["sizes"][a, b]), diff, spread, r["rounds"]))
            assert np.all(diff <= bar), (p, seed, diff)
    print("largest same-seed difference: %.3g" % worst)


def test_pcd_mode_and_distances(fixture_scene):
    """mode "pcd" on the sampled cloud gives the mesh mode's result; the per-point outputs agree with the counts."""
    import surfel_eval
    v, t, pts, _ = fixture_scene
    stl = _t(S.fixture_ground_truth())
    mask, bb, res, plane = S.fixture_obs()
    p = S.PARAMS[1]
    a = surfel_eval.evaluate_dtu(_mesh(v, t), stl, _t(mask), bb, res, plane, mode="mesh", seed=3, **p)
    b = surfel_eval.evaluate_dtu(pts, stl, _t(mask), bb, res, plane, mode="pcd", seed=3, return_distances=True, **p)
    assert all(a[k] == b[k] for k in a)
    assert b["dist_d2s"].shape[0] == b["data_in_obs"] == int(b["in_obs"].sum()) and b["dist_s2d"].shape[0] == b["stl_above"]
    assert int(b["inbound"].sum()) == b["data_in"] < b["data_down"] and bool((b["inbound"] | ~b["in_obs"]).all())
    assert torch.isinf(b["dist_d2s"]).any() and float(b["dist_d2s"][~torch.isinf(b["dist_d2s"])].max()) < p["max_dist"]


# ------------------------------------------------------------------------------------------------ culling
def test_culling():
    import surfel_eval
    v, f, K, poses, masks = S.cull_scene()
    proj = surfel_eval.projections(K, poses)
    dil = surfel_eval.dilate_masks(_t(masks), 6)
    odil = np.stack([O.dilate(m, 6) for m in masks])
    assert np.array_equal(dil.cpu().numpy().astype(bool), odil)
    big = surfel_eval.dilate_masks(_t(masks[:1]), 24).cpu().numpy().astype(bool)
    assert np.array_equal(big[0], O.dilate(masks[0], 24))
    keep = surfel_eval.cull_vertices(_t(v), proj, dil).cpu().numpy()
    want, near = O.cull_vertices(v, proj.astype(np.float64), odil, margins=True)
    print("culling: %d of %d kept, %d exempt" % (want.sum(), len(v), near.sum()))
    assert near.sum() <= len(v) // 200
    assert np.array_equal(keep[~near], want[~near])
    assert 0.05 < keep.mean() < 0.95
    out = surfel_eval.cull_mesh(_mesh(v, f), K, poses, _t(masks), dilate=6, scale=2.0, offset=(1.0, 2.0, 3.0))
    ov, ot = O.cull_mesh(v, f, keep, 2.0, np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(out.triangles.cpu().numpy(), ot) and len(ot) > 100
    assert np.allclose(out.vertices.cpu().numpy(), ov, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the project's own mesh
def test_end_to_end_extracted_sphere(sphere_extraction):
    """tests/test_gpu_mesh.py holds 99 % of this mesh's vertices within 1.5 voxels of the unit sphere on a closed manifold."""
    import surfel_eval
    mesh, voxel = sphere_extraction
    n = 200000
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), math.pi * (1 + 5 ** 0.5) * k
    gt = _t(np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1).astype(np.float32))
    pts = surfel_eval.sample_mesh(mesh, voxel / 2)
    down = pts[surfel_eval.thin(pts, voxel / 2, 0)]
    d2s, s2d = surfel_eval.nearest(down, gt), surfel_eval.nearest(gt, down)
    m1, m2 = surfel_eval.mean_below(d2s, math.inf), surfel_eval.mean_below(s2d, math.inf)
    f = surfel_eval.fscore(d2s, s2d, 2 * voxel)
    print("extracted sphere: %d samples, %d kept, mean_d2s %.4f voxel, mean_s2d %.4f voxel, %s" % (pts.shape[0], down.shape[0], m1 / voxel, m2 / voxel, f))
    assert m1 < 1.5 * voxel and m2 < 1.5 * voxel
    assert f["fscore"] >= 0.98
    assert abs(m1 - float(d2s.double().mean())) < 1e-6 * voxel and abs(m2 - float(s2d.double().mean())) < 1e-6 * voxel


# ------------------------------------------------------------------------------------------------ limits and the command line
def test_point_budget(fixture_scene):
    import surfel_eval
    v, t, pts, _ = fixture_scene
    mesh = _mesh(v, t)
    with pytest.raises(surfel_eval.MeshLimitError) as e:
        surfel_eval.sample_mesh(mesh, 0.001, budget_bytes=1 << 20)      # the large triangle alone wants 10 300 samples along an edge
    assert "SURFEL_EVAL_MAX_N" in str(e.value)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with pytest.raises(surfel_eval.MeshLimitError) as e:
        surfel_eval.sample_mesh(mesh, S.PARAMS[0]["density"], budget_bytes=12 * (pts.shape[0] - 1))
    assert "budget" in str(e.value)
    assert torch.cuda.max_memory_allocated() - base < 12 * pts.shape[0]      # the cloud was never allocated
    assert surfel_eval.sample_mesh(mesh, S.PARAMS[0]["density"], budget_bytes=12 * pts.shape[0]).shape == pts.shape


def test_cli(tmp_path, fixture_scene):
    import surfel_eval
    import surfel_io
    v, t, _, _ = fixture_scene
    mask, bb, res, plane = S.fixture_obs()
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "ObsMask")); os.makedirs(os.path.join(root, "Points", "stl"))
    np.savez(os.path.join(root, "ObsMask", "ObsMask1_10.npz"), ObsMask=mask, BB=bb, Res=np.array([[res]]))
    np.savez(os.path.join(root, "ObsMask", "Plane1.npz"), P=plane.reshape(4, 1))
    surfel_io.write_ply(os.path.join(root, "Points", "stl", "stl001_total.ply"), ["x", "y", "z"], S.fixture_ground_truth())
    surfel_io.write_triangle_mesh(os.path.join(root, "mesh.ply"), _mesh(v, t))
    out = os.path.join(root, "out")
    surfel_eval.main(["--data", os.path.join(root, "mesh.ply"), "--scan", "1", "--dataset_dir", root, "--vis_out_dir", out, "--seed", "2"])
    res_json = json.load(open(os.path.join(out, "results.json")))
    assert sorted(res_json) == ["mean_d2s", "mean_s2d", "overall"]
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_eval.npz"))
    assert abs(res_json["overall"] - z["means"][0, 2, 2]) <= SAME_SEED_BAR
    dv, _, dc = surfel_io.read_triangle_mesh(os.path.join(out, "vis_001_d2s.ply"))
    sv, _, sc = surfel_io.read_triangle_mesh(os.path.join(out, "vis_001_s2d.ply"))
    assert len(sv) == S.FIXTURE["gt_points"] and abs(len(dv) - z["sizes"][0, 2, 1]) <= 21
    assert np.all(sc[sv[:, 2] <= 44.0] == [0, 0, 1]) and np.all(sc[sv[:, 2] > 44.0][:, 0] == 1.0)      # below the plane: blue; above: white..red
    assert np.all(dc[dv[:, 0] >= 38.3] == [0, 0, 1])
    with pytest.raises(FileNotFoundError) as e:
        surfel_eval.main(["--data", os.path.join(root, "mesh.ply"), "--scan", "7", "--dataset_dir", root, "--vis_out_dir", out])
    assert "npz" in str(e.value)
