"""CPU checks of the Tanks-and-Temples-style evaluation (TNT.md): the numpy oracle (tests/tnt_oracle.py) against what the reference's own
run.py computed on the fixture scene (tests/golden/ref_tnt.npz, minted by tests/golden/make_golden_tnt.py), the conditions the scene has
to meet, each rule against a literal restatement, the host-side parts of surfel_eval_tnt and the library surface (header, exports, kernel
resources)."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tnt_oracle as O
import tnt_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_eval_tnt.h"


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_tnt.npz"))
    assert json.loads(str(z["scene"])) == json.loads(json.dumps(S.FIXTURE)), "the fixture was minted from another scene: run make_golden_tnt.py"
    assert json.loads(str(z["cases"])) == json.loads(json.dumps(S.CASES)) and int(z["ransac_seed"]) == S.RANSAC_SEED
    return z


@pytest.fixture(scope="module")
def oracle_runs(golden):
    """The oracle's own protocol on the fixture, once per recorded case, from the recorded trajectory transform."""
    v, t = S.mesh()
    pcd, gt, vol = O.mesh_cloud(v, t), S.ground_truth(), O.CropVolume(**S.crop_fields())
    return [O.evaluate_tnt(pcd, gt, vol, S.FIXTURE["tau"], golden["trajectory"][k], **case, return_clouds=True) for k, case in enumerate(S.CASES)]


# ------------------------------------------------------------------------------------------------ the oracle against the reference
def test_oracle_reproduces_reference(golden, oracle_runs):
    """Sizes and iterations exactly, P / R / F and the curves to 1e-12, the transform to 1e-9: both sides are fp64 on identical inputs; the
    reference's Python decides the stage order, the thresholds, the voxel sizes, T_icp . T_init, the centroids and the histogram."""
    tau = S.FIXTURE["tau"]
    assert np.array_equal(golden["stage_fit"][:, :, 2], np.tile([80 * tau, 20 * tau, 2 * tau], (len(S.CASES), 1)))
    for k, r in enumerate(oracle_runs):
        assert [[s["source"], s["target"], s["iterations"]] for s in r["stages"]] == golden["stage_sizes"][k].tolist(), k
        assert [r["source"], r["target"]] == golden["scored"][k].tolist()
        assert golden["crops"][k][-2:].tolist()[0][0] == len(S.mesh()[0]) + len(S.mesh()[1])
        got = np.array([r["precision"], r["recall"], r["fscore"]])
        assert np.max(np.abs(got - golden["prf"][k][:3])) < 1e-12 and golden["prf"][k][3] == tau and golden["prf"][k][4] == 5
        assert r["cum_source"].shape == golden["cum_source"][k].shape == (499,)
        assert np.max(np.abs(r["cum_source"] - golden["cum_source"][k])) < 1e-12 and np.max(np.abs(r["cum_target"] - golden["cum_target"][k])) < 1e-12
        assert np.max(np.abs(r["transformation"] - golden["final"][k])) < 1e-9
        fit = np.array([[s["fitness"], s["inlier_rmse"]] for s in r["stages"]])
        assert np.max(np.abs(fit - golden["stage_fit"][k][:, :2])) < 1e-9
    assert golden["stage_sizes"][0, :, 2].tolist() != golden["stage_sizes"][1, :, 2].tolist()      # the second case exercises the loop
    assert golden["stage_sizes"][1, :, 2].max() > 5


def test_scene_conditions(golden, oracle_runs):
    """What TNT.md §Pinning asks of the scene, on the oracle alone."""
    f = S.FIXTURE
    assert len(set(f["axes"])) == 3 and f["bump"] > 0 and f["scene"] == "Barn" and f["tau"] == 0.01      # not rotationally symmetric
    assert len(f["polygon"]) == 6 and abs(f["scale"] - 1.03) < 0.011 and 35 <= f["cameras"] <= 45
    v, t = S.mesh()
    gt = S.ground_truth()
    assert len(gt) == 120000 and 55000 <= len(v) + len(t) <= 65000
    # the polygon is concave and cuts the object, and so do the axis bounds
    poly = np.asarray(f["polygon"])
    e1, e2 = np.roll(poly, -1, 0) - poly, np.roll(poly, -2, 0) - np.roll(poly, -1, 0)
    turn = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert (turn > 0).any() and (turn < 0).any()
    vol = O.CropVolume(**S.crop_fields())
    m = O.crop_mask(gt, vol)
    band = (gt[:, 2] >= f["axis_min"]) & (gt[:, 2] <= f["axis_max"])
    assert 0.3 < m.mean() < 0.8 and 0.5 < band.mean() < 0.98 and m.sum() < band.sum() * 0.9
    for k, r in enumerate(oracle_runs):
        assert 0.2 < r["precision"] < 0.9 and 0.2 < r["recall"] < 0.9, (r["precision"], r["recall"])
        d = np.concatenate([r["distance1"], r["distance2"]])
        near = int((np.abs(d - f["tau"]) < 1e-6).sum())
        print("case %d: P %.4f R %.4f, %d of %d final distances within 1e-6 of tau" % (k, r["precision"], r["recall"], near, len(d)))
        assert near <= len(d) * 1e-4
        # Where the loop stops.  TNT.md asks for | |dfitness| - relative_fitness | >= 10 / n_source at every iteration, so that a few
        # correspondences flipped by fp32 rounding cannot move the stop.  A loop that stops does so with dfitness = 0 exactly (any change
        # of the count is at least 1 / n_source > relative_fitness for n_source < 10^6), where that margin is relative_fitness itself; there
        # the condition that carries the same meaning is that no pair can flip at all: none within NEAR_MARGIN (1e-6, four times the fp32
        # resolution at this scene's coordinates) of the threshold at either of the two evaluations.
        for s in r["stages"]:
            h = np.array(s["history"])
            for i in range(1, len(h)):
                margin = abs(abs(h[i, 0] - h[i - 1, 0]) - S.CASES[k]["relative_fitness"])
                assert margin >= 10 / s["source"] or (h[i, 2] == 0 and h[i - 1, 2] == 0), (k, s["source"], i, h[i - 1], h[i])


def test_icp_scene_exempt_share():
    """The GPU test of one ICP evaluation exempts queries whose two nearest target points differ by less than 2^-22 extent in distance, or
    whose distance is that close to the threshold; on its scene that share is below the 0.1 % cap (here: below half of it)."""
    src, tgt, T, thr = S.icp_pair()
    assert src.shape == (30000, 3) and tgt.shape == (60000, 3)
    moved = O.transform(src, T)
    d, _ = O.nearest(moved, tgt, k=2)
    margin = 2.0 ** -22 * np.ptp(tgt.astype(np.float64), axis=0).max()
    exempt = (d[:, 1] - d[:, 0] < margin) | (np.abs(d[:, 0] - thr) < margin)
    hit = (d[:, 0] < thr).mean()
    print("icp scene: fitness %.4f, %d of %d queries exempt (cap %d)" % (hit, exempt.sum(), len(src), len(src) // 1000))
    assert 0.5 < hit < 0.999 and exempt.sum() <= len(src) // 2000


# ------------------------------------------------------------------------------------------------ each rule against a literal restatement
def _sorted_pairs(p, vol):
    """Open3D's crop test written out: the nodes of the crossing edges, sorted, taken in pairs."""
    u, v, w = vol.uvw()
    poly = vol.bounding_polygon
    out = np.zeros(len(p), bool)
    for n, q in enumerate(np.asarray(p, np.float64)):
        if not (vol.axis_min <= q[w] <= vol.axis_max):
            continue
        nodes = []
        for k in range(len(poly)):
            a, b = poly[k], poly[(k + 1) % len(poly)]
            if (a[v] < q[v] and b[v] >= q[v]) or (b[v] < q[v] and a[v] >= q[v]):
                nodes.append(a[u] + (q[v] - a[v]) / (b[v] - a[v]) * (b[u] - a[u]))
        nodes.sort()
        for k in range(0, len(nodes) - 1, 2):
            if nodes[k] < q[u] < nodes[k + 1]:
                out[n] = True
    return out


def test_crossing_rule_equals_sorted_pairs():
    for axis in ("X", "Y", "Z"):
        fields, pts = S.crop_case(axis, n=100000 if axis == "Z" else 5000)
        vol = O.CropVolume(**fields)
        got, want = O.crop_mask(pts, vol), _sorted_pairs(pts, vol)
        assert np.array_equal(got, want), axis
        special = got[-(len(pts) - (100000 if axis == "Z" else 5000)):]
        assert 0.15 < got.mean() < 0.6 and special.any() and not special.all()
    # by hand, on the unit square seen along Z: inside, on the left edge (a node equals p.u), on a vertex, level with the top edge, outside
    sq = O.CropVolume("Z", 0, 1, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    pts = np.array([[0.5, 0.5, 0.5], [0, 0.5, 0.5], [1, 0.5, 0.5], [0, 0, 0.5], [0.5, 1, 0.5], [0.5, 0, 0.5], [2, 0.5, 0.5], [0.5, 0.5, 1], [0.5, 0.5, 1.5]])
    assert O.crop_mask(pts, sq).tolist() == [True, False, False, False, True, False, False, True, False]
    assert np.array_equal(O.crop_mask(pts, sq), _sorted_pairs(pts, sq))


def test_voxel_rule_against_a_dict_of_lists():
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(-3, 2, size=(5000, 3)), np.round(rng.uniform(-3, 2, size=(500, 3)) * 4) / 4]).astype(np.float32)
    for voxel in (0.25, 0.37):
        means, counts, cells = O.voxel_down_sample(pts, voxel)
        origin = pts.astype(np.float64).min(0) - voxel / 2
        d = {}
        for p in pts.astype(np.float64):
            d.setdefault(tuple(np.floor((p - origin) / voxel).astype(int)), []).append(p)
        keys = sorted(d, key=lambda c: (c[2], c[1], c[0]))
        assert [tuple(c) for c in cells] == keys and counts.tolist() == [len(d[k]) for k in keys]
        want = []
        for k in keys:
            s = np.zeros(3)
            for p in d[k]:
                s = s + p
            want.append(s / len(d[k]))
        assert np.array_equal(means, np.array(want)) and 500 < len(keys) < 5500


def test_histogram_rule_against_numpy():
    rng = np.random.default_rng(2)
    for tau in (0.01, 0.005, 0.025, 0.003):
        edges = np.arange(0, 5 * tau, tau / 100)
        assert len(edges) == 500
        d = np.concatenate([rng.uniform(0, 6 * tau, 20000), edges, edges[1:] - 1e-12, [edges[-1], np.inf, 0.0, np.nextafter(edges[-1], 1)]]).astype(np.float32)
        assert np.array_equal(O.histogram(d, edges), np.histogram(d, edges)[0])
        assert np.array_equal(O.histogram(d.astype(np.float64), edges), np.histogram(d.astype(np.float64), edges)[0])


def _random_similarity(rng, scale):
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    q = q * np.sign(np.linalg.det(q))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * q, rng.normal(size=3)
    return T


def test_umeyama_recovers_a_similarity():
    sys.path.insert(0, PKG)
    import surfel_eval_tnt as P
    rng = np.random.default_rng(3)
    for flat in (1.0, 1e-7):      # a cloud, and a nearly planar one, whose covariance's smallest singular value is noise: the reflection case
        for trial in range(20):
            T = _random_similarity(rng, rng.uniform(0.5, 2.0))
            x = rng.normal(size=(50, 3)) * [1.0, 1.0, flat] + rng.normal(size=3)
            y = O.transform(x, T)
            idx = np.arange(50)
            for got in (O.umeyama(x, y), O.umeyama_from_sums(O.correspondence_sums(x, idx, y)), P.umeyama(x, y), P.umeyama_from_sums(O.correspondence_sums(x, idx, y))):
                assert np.linalg.det(got[:3, :3]) > 0
                assert np.max(np.abs(O.transform(x, got) - y)) < 1e-7, (flat, trial)
    # exactly planar, mirrored target: a proper rotation comes back, never the reflection
    x = np.concatenate([rng.normal(size=(30, 2)), np.zeros((30, 1))], 1)
    got = O.umeyama(x, x * [1, -1, 1])
    assert abs(np.linalg.det(got[:3, :3]) - 1) < 1e-9


def test_ransac_recovers_the_similarity_and_is_seeded(golden):
    sys.path.insert(0, PKG)
    import surfel_eval_tnt as P
    rng = np.random.default_rng(4)
    T = S.similarity([5, -3, 8], 1.07, [0.2, 0.1, -0.3])
    n = 40
    est = rng.uniform(-2, 2, size=(n, 3))
    gt = O.transform(est, T) + rng.normal(0, 0.002, size=(n, 3))
    bad = rng.permutation(n)[:n * 3 // 10]
    gt[bad] += rng.choice([-1, 1], size=(len(bad), 3)) * rng.uniform(0.3, 1.0, size=(len(bad), 3))      # 30 % displaced by more than 0.2
    a = P.trajectory_alignment(est, gt, None, seed=5, draws=3000)
    b = P.trajectory_alignment(est, gt, None, seed=5, draws=3000, batch=700)
    c = O.trajectory_alignment(est, gt, None, seed=5, draws=3000)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert abs(a[1] - 0.7) < 1e-12 and a[1] == c[1] and abs(a[2] - c[2]) < 1e-12 and np.max(np.abs(a[0] - c[0])) < 1e-9
    assert np.max(np.abs(O.transform(est, a[0]) - O.transform(est, T))) < 0.02
    assert not np.array_equal(P.trajectory_alignment(est, gt, None, seed=6, draws=3000)[0], a[0])
    # the fixture's trajectory transform, through the .log format's 12 decimals as the reference read it
    est_p, col_p = S.cameras()
    col_p = np.round(col_p, 12)
    got = P.trajectory_alignment(est_p[:, :3, 3], col_p[:, :3, 3], S.alignment(), seed=S.RANSAC_SEED)
    assert got[1] == golden["trajectory_fit"][0, 0] and np.max(np.abs(got[0] - golden["trajectory"][0])) < 1e-9


def test_readers_round_trip(tmp_path):
    sys.path.insert(0, PKG)
    import surfel_eval_tnt as P
    est, col = S.cameras()
    P.write_trajectory_log(str(tmp_path / "a.log"), col)
    back, meta = P.read_trajectory_log(str(tmp_path / "a.log"))
    assert back.shape == col.shape and np.max(np.abs(back - col)) <= 0.5e-12 and meta[3] == [3, 3, 0]
    assert np.array_equal(P.read_trajectory(str(tmp_path / "a.log")), back)
    np.save(str(tmp_path / "a.npy"), est.astype(np.float32))
    assert np.array_equal(P.read_trajectory(str(tmp_path / "a.npy")), est.astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError):
        P.read_trajectory("poses.json")
    vol = P.CropVolume(**S.crop_fields())
    P.write_crop_volume(str(tmp_path / "c.json"), vol)
    v2 = P.read_crop_volume(str(tmp_path / "c.json"))
    assert (v2.orthogonal_axis, v2.axis_min, v2.axis_max) == ("Z", S.FIXTURE["axis_min"], S.FIXTURE["axis_max"]) and np.array_equal(v2.bounding_polygon, vol.bounding_polygon)
    assert np.array_equal(v2.uv(), np.asarray(S.FIXTURE["polygon"])) and v2.axis == 2
    assert P.CropVolume("X", 0, 1, [[9, 1, 2]]).uv().tolist() == [[1, 2]] and P.CropVolume("Y", 0, 1, [[1, 9, 2]]).uv().tolist() == [[1, 2]]
    np.savetxt(str(tmp_path / "t.txt"), S.alignment())
    assert np.array_equal(P.read_alignment(str(tmp_path / "t.txt")), S.alignment())
    assert P.SCENES_TAU == {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01, "Truck": 0.005}


def test_colormap_against_matplotlib():
    """hot_r without matplotlib, to 1 / 255 per channel: the step of the 8-bit colour a .ply stores."""
    cm = pytest.importorskip("matplotlib.cm")
    import matplotlib
    sys.path.insert(0, PKG)
    import surfel_eval_tnt as P
    x = np.concatenate([np.linspace(0, 1, 4097), [0.365079, 0.746032, 1 - 0.365079, 1 - 0.746032]])
    want = matplotlib.colormaps["hot_r"](x)[:, :3]
    got = P.hot_r(x)
    print("hot_r: max |ours - matplotlib| = %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1 / 255
    import torch
    assert np.abs(P.hot_r(torch.from_numpy(x)).numpy() - want).max() <= 1 / 255
    assert np.abs(O.hot(1 - x) - want).max() <= (1 / (1 - 0.746032)) / 256 + 1e-12      # the continuous ramps, up to the table's step on the steepest


# ------------------------------------------------------------------------------------------------ library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_tnt_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", HEADER)).read(), re.M)
    assert len(decl) == 6
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.TNT_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    assert not set(decl) & set(surfel_native.EXPORTS + surfel_native.MESH_EXPORTS + surfel_native.UNBOUNDED_EXPORTS + surfel_native.EVAL_EXPORTS)
    lib = surfel_native.load()
    for name in surfel_native.TNT_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name


def test_tnt_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_eval_tnt.h."""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    old = A.REPO
    protos, mentions = A._prototypes(HEADER)
    assert old == REPO and len(protos) == mentions == 6
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
                host = pname in ("T", "origin", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_tnt_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("eval_tnt.hip"))
    names = [k for k in ks if "tnt_" in k or "rekey_kernel" in k]      # (the voxel sort's high word: rekey_kernel<VoxelKey>, side_util.h)
    assert len(names) == 10 and sum("rekey_kernel" in k for k in names) == 1, names
    for k in names:
        assert int(ks[k][1].get("private_segment_fixed_size", 0)) == 0, k
    sums = [k for k in names if "corr_sums_kernel" in k][0]
    print("tnt_corr_sums_kernel: %d VGPRs, %d B LDS" % (ks[sums][1].get("next_free_vgpr", 0), ks[sums][1].get("group_segment_fixed_size", 0)))
    assert ks[sums][1].get("next_free_vgpr", 0) <= 128


def test_tnt_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    sys.path.insert(0, PKG)
    import surfel_eval_tnt as P
    from surfel_mesh import TriangleMesh
    p = torch.zeros((8, 3))
    vol = P.CropVolume(**S.crop_fields())
    mesh = TriangleMesh(p, torch.zeros((1, 3), dtype=torch.int32), p)
    for call in (lambda: P.mesh_cloud(mesh), lambda: P.transform(p, np.eye(4)), lambda: P.crop(p, vol), lambda: P.voxel_down_sample(p, 0.1),
                 lambda: P.uniform_down_sample(p), lambda: P.icp_similarity(p, p, 0.1), lambda: P.icp_evaluate(p, p, np.eye(4), 0.1),
                 lambda: P.correspondence_sums(p, torch.zeros(8, dtype=torch.int32), p), lambda: P.histogram(p[:, 0], np.arange(3.0), 1.0),
                 lambda: P.score(p[:, 0], p[:, 0], 0.01), lambda: P.evaluate_tnt(p, p, vol, 0.01, init_transform=np.eye(4)),
                 lambda: P.evaluate_tnt(mesh, p, vol, 0.01, init_transform=np.eye(4))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "tensors must live on a HIP device" in str(e.value)


def test_tnt_budget_is_checked_before_allocating():
    """The pattern of test_call_maps_error_codes_without_a_device: the calls fail before the library touches a device or the allocator."""
    import ctypes as C
    import surfel_eval_tnt as P
    import surfel_native as n
    assert P.MeshLimitError is n.LimitError
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    origin = (C.c_double * 3)(0, 0, 0)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*budget"):
        n.call(None, "surfel_tnt_voxel_down_sample", cb, None, 1000, C.c_void_p(256), 0.01, origin, 24000, C.c_void_p(256), None, None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*2\^30"):
        n.call(None, "surfel_tnt_voxel_down_sample", cb, None, 1 << 30, C.c_void_p(256), 0.01, origin, 1 << 62, C.c_void_p(256), None, None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*SURFEL_TNT_MAX_POLYGON"):
        n.call(None, "surfel_tnt_crop", 10, C.c_void_p(256), 2, 0.0, 1.0, 1025, C.c_void_p(256), C.c_void_p(256))
    with pytest.raises(n.LimitError, match=r"\(-4\): .*SURFEL_TNT_MAX_EDGES"):
        n.call(None, "surfel_tnt_histogram", 10, C.c_void_p(256), 2049, C.c_void_p(256), 1.0, C.c_void_p(256))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
        n.call(None, "surfel_tnt_crop", 10, C.c_void_p(256), 3, 0.0, 1.0, 4, C.c_void_p(256), C.c_void_p(256))
    assert not taken
