"""CPU checks of the mesh evaluation (EVAL.md): the numpy oracle (tests/eval_oracle.py) against what the reference's own eval.py
computed on the fixture scene (tests/golden/ref_eval.npz, minted by tests/golden/make_golden_eval.py), against hand-derived cases, and
the library surface (header, exports, kernel resources)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import eval_oracle as O
import eval_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_eval.npz"))
    assert json.loads(str(z["scene"])) == json.loads(json.dumps(S.FIXTURE)), "the fixture was minted from another scene: run make_golden_eval.py"
    assert json.loads(str(z["params"])) == json.loads(json.dumps(S.PARAMS))
    assert tuple(z["seeds"]) == S.SEEDS
    return z


@pytest.fixture(scope="module")
def fixture_cloud():
    v, t = S.fixture_mesh()
    pts, counts = O.sample_mesh(v, t, S.PARAMS[0]["density"])
    return v, t, pts, counts, O.radius_pairs(pts, S.PARAMS[0]["density"])


# ------------------------------------------------------------------------------------------------ the oracle against the reference
def test_oracle_reproduces_reference(golden, fixture_cloud):
    """Stage sizes exactly and the three means to 1e-9 relative, per parameter set and seed: both sides are fp64 on identical inputs
    in identical order."""
    v, t, pts, counts, pairs = fixture_cloud
    stl = S.fixture_ground_truth()
    mask, bb, res, plane = S.fixture_obs()
    names = [str(x) for x in golden["size_names"]]
    assert names == ["data_pcd", "data_down", "data_in", "data_in_obs", "stl_above"]
    for b, seed in enumerate(S.SEEDS):
        keep = O.thin_sequential(len(pts), pairs, O.shuffle_order(len(pts), seed))
        for a, p in enumerate(S.PARAMS):
            assert p["density"] == S.PARAMS[0]["density"]
            r = O.evaluate_dtu(pts, stl, mask, bb, res, plane, p["density"], p["patch"], p["max_dist"], seed, keep=keep)
            assert [r[k] for k in names] == list(golden["sizes"][a, b]), (p, seed)
            got = np.array([r["mean_d2s"], r["mean_s2d"], r["overall"]])
            assert np.max(np.abs(got / golden["means"][a, b] - 1)) < 1e-9, (p, seed, got, golden["means"][a, b])


def test_fixture_bites(golden):
    """The second parameter set must cut: fewer points inside its bounding box, a smaller mean under its max_dist."""
    s, m = golden["sizes"], golden["means"]
    assert np.all(s[1, :, 2] < s[0, :, 2]) and np.all(s[0, :, 2] == s[0, :, 1])      # data_in < data_down only with patch = 1
    assert np.all(s[:, :, 3] < s[:, :, 2])                                            # the observation mask drops points
    assert np.all(s[:, :, 4] < S.FIXTURE["gt_points"])                                # the plane drops ground truth
    assert np.all(m[1] < m[0])
    spread = np.ptp(m[0], axis=0)
    print("reference seed spread (max |ref(a) - ref(b)|) of mean_d2s, mean_s2d, overall:", spread)
    assert np.all(spread > 0)


def test_analytic_anchor(golden):
    """The mesh is inscribed in the sphere of radius 12 (sagitta of a 0.4 edge: 0.002), the ground truth lies on radius 12.35: both
    means are 0.35 up to the lateral offset to the nearest sample, which the sampling density (0.2) bounds."""
    gap = S.FIXTURE["gt_radius"] - S.FIXTURE["radius"]
    assert np.all(np.abs(golden["means"][0, :, :2] - gap) <= S.PARAMS[0]["density"])
    assert np.all(golden["means"][0, :, :2] >= gap - 0.01)


def test_pairs_near_the_threshold(fixture_cloud):
    """How many point pairs of the fixture an fp32 pair test could flip: those within 1e-5 of density in fp64 (the GPU end-to-end test
    caps the size difference this causes at 0.1 %)."""
    v, t, pts, counts, pairs = fixture_cloud
    d = S.PARAMS[0]["density"]
    i, j = O.radius_pairs(pts, d + 1e-5)
    dist = np.linalg.norm(pts[i] - pts[j], axis=1)
    close = int((np.abs(dist - d) < 1e-5).sum()) // 2
    print("pairs within 1e-5 of density: %d of %d points (cap: %d)" % (close, len(pts), len(pts) // 1000))
    assert close <= len(pts) // 1000


# ------------------------------------------------------------------------------------------------ hand-derived cases
def _count_by_hand(n1, n2):
    return sum(1 for i in range(n1 + 1) for j in range(n2 + 1) if (i + 0.5) / n1 + (j + 0.5) / n2 < 1)


def test_sampling_by_hand():
    # right triangle, legs 3, density 1: |v1 x v2| = |v1| |v2|, thr = 1, n1 = n2 = 3.  The lattice (i + 0.5) / 3 + (j + 0.5) / 3 < 1 holds
    # strictly for i + j <= 1 (3 points); i + j = 2 lies on the hypotenuse and is decided by fp64 rounding: 0.5/3 + 2.5/3 and
    # 2.5/3 + 0.5/3 give exactly 1.0 (excluded), 1.5/3 + 1.5/3 = 1.0 (excluded)
    v = np.array([(0, 0, 0), (3, 0, 0), (0, 3, 0), (4, 0, 0), (0, 2, 0), (1, 1, 0), (2, 2, 0), (1e-3, 0, 1)], np.float32)
    t = np.array([(0, 1, 2), (0, 3, 4), (0, 5, 6), (0, 1, 7)], np.int32)
    pts, counts = O.sample_mesh(v, t, 1.0)
    assert 0.5 / 3 + 2.5 / 3 == 1.0 and 1.5 / 3 + 1.5 / 3 == 1.0
    assert counts[0] == 3 == _count_by_hand(3, 3)
    assert np.allclose(pts[len(v):len(v) + 3], [(0.5, 0.5, 0), (0.5, 1.5, 0), (1.5, 0.5, 0)])      # i outer, j inner
    # legs 4 and 2: thr = 1, n1 = 4, n2 = 2: c0 in {1/8, 3/8, 5/8, 7/8, 9/8}, c1 in {1/4, 3/4, 5/4}: (1/8, 1/4), (1/8, 3/4), (3/8, 1/4),
    # (5/8, 1/4) are inside; (3/8, 3/4) and (7/8, 1/4) are 1.125 > 1
    assert counts[1] == 4 == _count_by_hand(4, 2)
    assert counts[2] == 0                       # collinear: zero area
    # the fourth: l1 = 3, l2 ~ 1, area2 ~ 3: thr = 1, n1 = 3, n2 = floor(1.0000005) = 1
    assert counts[3] == _count_by_hand(3, 1) == 1
    assert len(pts) == len(v) + counts.sum()
    half = O.sample_mesh(v, t, 0.5)[1]
    assert half[0] == _count_by_hand(6, 6) == 15 and half[1] == _count_by_hand(8, 4)


def test_thinning_is_the_first_independent_set():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 3, size=(2000, 3))
    for f32 in (False, True):
        p = pts.astype(np.float32) if f32 else pts
        brute = O.radius_pairs_brute(p, 0.2, f32)
        fast = O.radius_pairs(p, 0.2, f32)
        assert sorted(zip(*brute)) == sorted(zip(*fast)) and len(brute[0]) > 2000
        for seed in (None, 0, 1):
            order = O.shuffle_order(len(p), seed)
            seq = O.thin_sequential(len(p), fast, order)
            # the literal loop once more, without the adjacency lists
            lit = np.ones(len(p), bool)
            nb = {}
            for i, j in zip(*brute):
                nb.setdefault(int(i), []).append(int(j))
            for cur in order:
                if lit[cur]:
                    lit[nb.get(int(cur), [])] = False
                    lit[cur] = True
            mis, rounds = O.thin_rounds(len(p), fast, order)
            assert np.array_equal(seq, lit) and np.array_equal(seq, mis)
            assert 500 < seq.sum() < 2000 and rounds > 2
            kept = np.nonzero(seq)[0]                                 # independent and maximal
            assert not np.isin(fast[0], kept)[np.isin(fast[1], kept)].any()
            covered = np.zeros(len(p), bool); covered[kept] = True
            covered[fast[0][np.isin(fast[1], kept)]] = True
            assert covered.all()


def test_shuffle_matches_the_reference_shuffle():
    """eval.py shuffles the rows in place with an unseeded generator; rule 2 states the order as permutation(n) of a seeded one: the same
    draws."""
    x = np.arange(30, dtype=np.float64).reshape(10, 3)
    y = x.copy()
    np.random.default_rng(3).shuffle(y, axis=0)
    assert np.array_equal(y, x[np.random.default_rng(3).permutation(10)])


def test_fscore_edges():
    inf = np.inf
    assert O.fscore(np.array([0.1, 0.3, inf]), np.array([0.1, 0.1, 0.1, 0.5]), 0.2) == dict(precision=1 / 3, recall=0.75, fscore=2 * (1 / 3) * 0.75 / (1 / 3 + 0.75))
    assert O.fscore(np.array([0.2]), np.array([0.2]), 0.2)["fscore"] == 0.0          # strict <
    assert O.fscore(np.array([inf]), np.array([inf]), 1.0) == dict(precision=0.0, recall=0.0, fscore=0.0)
    assert O.fscore(np.zeros(0), np.zeros(0), 1.0)["fscore"] == 0.0
    assert O.fscore(np.array([0.0]), np.array([0.0]), 1e-9)["fscore"] == 1.0


def test_nearest_forms_agree():
    rng = np.random.default_rng(2)
    q, c = rng.uniform(0, 10, size=(700, 3)), rng.uniform(0, 10, size=(900, 3)) + 1e3      # far from the origin: centring matters
    assert np.array_equal(O.nearest(q + 1e3, c), O.nearest_exact(q + 1e3, c))
    assert np.all(np.isinf(O.nearest(q, np.zeros((0, 3)))))


def test_dilation_and_culling_brute_force():
    rng = np.random.default_rng(4)
    H, W, r = 48, 64, 5
    mask = (rng.random((H, W)) < 0.01).astype(np.uint8) * 200
    mask[10:14, 50:64] = 1
    ref = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if dx * dx + dy * dy <= r * r and 0 <= y + dy < H and 0 <= x + dx < W and mask[y + dy, x + dx]:
                        ref[y, x] = True
    dil = O.dilate(mask, r)
    assert np.array_equal(dil, ref) and ref.sum() > mask.astype(bool).sum() * 10
    # one view, identity pose, K with focal 40: a vertex survives iff it projects onto the dilated mask or outside (-1, 1)
    K = np.array([[40, 0, (W - 1) / 2, 0], [0, 40, (H - 1) / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    proj = (K @ np.eye(4))[:3].reshape(1, 12)
    v = np.concatenate([rng.uniform(-1, 1, size=(400, 2)) * [1.2, 0.9], np.full((400, 1), 1.0)], 1)
    keep = O.cull_vertices(v, proj, dil[None])
    want = np.zeros(len(v), bool)
    for k, (x, y, z) in enumerate(v):
        px, py = (40 * x + (W - 1) / 2 * z) / (z + 1e-6), (40 * y + (H - 1) / 2 * z) / (z + 1e-6)
        nx, ny = (px / (W - 1) - 0.5) * 2, (py / (H - 1) - 0.5) * 2
        if not (-1 < nx < 1 and -1 < ny < 1):
            want[k] = True
            continue
        ix, iy = int(np.around((nx + 1) / 2 * (W - 1))), int(np.around((ny + 1) / 2 * (H - 1)))
        want[k] = bool(ref[iy, ix])
    assert np.array_equal(keep, want) and 0 < keep.sum() < len(v)
    vv, tt = O.cull_mesh(v, np.array([(0, 1, 2), (3, 4, 5)]), np.array([True] * 3 + [True, False, True] + [True] * 394), 2.0, 1.0)
    assert len(vv) == 3 and np.array_equal(tt, [(0, 1, 2)]) and np.allclose(vv, v[:3] * 2 + 1)


def test_culling_margins_are_rare():
    """The GPU culling test exempts vertices whose ndc lies within 1e-5 of +-1, or whose pixel coordinate lies within 1e-3 of a
    half-integer where that changes the sampled value; on its scene that is far below its 0.5 % cap."""
    sys.path.insert(0, PKG)
    v, f, K, poses, masks = S.cull_scene()
    proj = np.stack([(K[i] @ np.linalg.inv(poses[i]))[:3].reshape(-1) for i in range(6)])
    dil = np.stack([O.dilate(m, 6) for m in masks])
    keep, near = O.cull_vertices(v, proj, dil, margins=True)
    print("culling: %d of %d kept, %d within the margins (cap %d)" % (keep.sum(), len(v), near.sum(), len(v) // 200))
    assert 0.05 < keep.mean() < 0.95
    assert near.sum() <= len(v) // 200 // 2


# ------------------------------------------------------------------------------------------------ library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_eval_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", "surfel_eval.h")).read(), re.M)
    assert len(decl) == 10
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.EVAL_EXPORTS) == sorted(decl)
    lib = surfel_native.load()
    for name in surfel_native.EVAL_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name


def test_eval_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("eval_geometry.hip"))
    names = [k for k in ks if "eval_" in k]
    assert len(names) >= 15, names
    for k in names:
        assert int(ks[k][1].get("private_segment_fixed_size", 0)) == 0, k


def test_eval_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    sys.path.insert(0, PKG)
    import surfel_eval
    from surfel_mesh import TriangleMesh
    p = torch.zeros((4, 3))
    for call in (lambda: surfel_eval.thin(p, 0.2), lambda: surfel_eval.nearest(p, p), lambda: surfel_eval.fscore(p[:, 0], p[:, 0], 1.0),
                 lambda: surfel_eval.sample_mesh(TriangleMesh(p, torch.zeros((1, 3), dtype=torch.int32), p), 0.2),
                 lambda: surfel_eval.evaluate_dtu(p, p, torch.zeros((2, 2, 2), dtype=torch.uint8), np.zeros((2, 3)), 1.0, np.zeros(4), mode="pcd"),
                 lambda: surfel_eval.dilate_masks(torch.zeros((1, 4, 4), dtype=torch.uint8))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "tensors must live on a HIP device" in str(e.value)
