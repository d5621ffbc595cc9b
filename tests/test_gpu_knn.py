"""-m gpu tests of csrc/knn.hip (simple_knn._C.distCUDA2: mean squared distance to the three nearest neighbours) at the sizes and inputs
where its structure sits: search workgroups and LDS chunks of 256 points, boxes of 1024, 2^10 Morton cells per axis, the degenerate-axis
branch of the quantiser (extent 0), and the pruning rule `box distance <= b2` at b2 == 0 (duplicates) and b2 == FLT_MAX (fewer than three
candidates seen so far).  The result initialises every scene's scales.

Reference: Oracle("f64").knn_dist2 — brute force in fp64 on the same fp32 inputs.  Tolerance: rtol 1e-5, atol 1e-9, that of
test_gpu_parity.py::test_knn_exact; an fp32 squared distance from exact (or exactly rounded) differences carries ~2e-7 relative."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-9


def _device(pts):
    import torch
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.tensor(np.ascontiguousarray(pts, np.float32), device="cuda:0")).cpu().numpy()


def _oracle(pts):
    from oracle.surfel_oracle import Oracle
    return Oracle("f64").knn_dist2(np.ascontiguousarray(pts, np.float32))


def _check(pts, what):
    got = _device(pts); ref = _oracle(pts)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - ref) - (ATOL + RTOL * np.abs(ref))
    assert np.allclose(got, ref, rtol=RTOL, atol=ATOL), "%s: %d of %d points off, worst at %d: %.9g against %.9g" % (
        what, int((err > 0).sum()), len(ref), int(err.argmax()), got[err.argmax()], ref[err.argmax()])
    return got, ref


def _cloud(kind, P, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=(P, 3)).astype(np.float32)
    assert kind == "mixed"      # three scales mixed: points of the wide component have their neighbours many boxes away in Morton order
    return (rng.normal(size=(P, 3)) * rng.choice([0.05, 1.0, 5.0], size=(P, 1))).astype(np.float32)


@pytest.mark.parametrize("kind", ["normal", "mixed"])
@pytest.mark.parametrize("P", [4, 5, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2047, 2049, 4097])
def test_size_edges(P, kind):
    """one point more and one fewer than a search workgroup / LDS chunk (256), a box (1024) and their multiples; P = 4 is the smallest
    cloud in which every point has three neighbours"""
    got, ref = _check(_cloud(kind, P, seed=P), "%s cloud of %d" % (kind, P))
    assert (ref > 0).all()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_fewer_than_three_neighbours(P):
    """The kernel keeps its three best distances in fp32 from FLT_MAX seeds: with fewer than three neighbours a seed is left and the mean
    of three is +inf.  The fp64 oracle's sum of the same seeds does not overflow and stays finite, so it is no reference here: the
    device's value is asserted directly to be +inf.

    P = 3 found a defect: the kernel returned 1.1342745e+38 = FLT_MAX / 3 for every point.  With two neighbours one seed is left,
    (b0 + b1) + FLT_MAX rounds back to FLT_MAX in fp32 (its ulp is 2e31) and the division by 3 is finite; only two seeds (P = 1, 2:
    FLT_MAX + FLT_MAX) overflow by themselves.  The kernel now returns +inf whenever a seed is left in b2."""
    got = _device(_cloud("normal", P, seed=P))
    assert got.shape == (P,)
    assert np.isposinf(got).all(), got


def test_no_points():
    import torch
    from simple_knn._C import distCUDA2
    got = distCUDA2(torch.empty((0, 3), device="cuda:0"))
    assert got.shape == (0,) and got.dtype == torch.float32 and got.device.type == "cuda"


@pytest.mark.parametrize("kind", ["plane", "line", "point"])
def test_degenerate_extents(kind):
    """1500 points (two boxes) with one, two or all three axes constant: the quantiser's `ext > 0 ? ... : 0` branch.  All points
    identical: every distance is exactly 0 and so is the result."""
    P = 1500
    rng = np.random.default_rng(11)
    pts = rng.normal(size=(P, 3)).astype(np.float32)
    const = {"plane": [1], "line": [0, 2], "point": [0, 1, 2]}[kind]
    pts[:, const] = np.array([0.37, -2.5, 11.0], np.float32)[const]
    got, ref = _check(pts, kind)
    if kind == "point":
        assert not got.any() and not ref.any()
    else:
        assert (ref > 0).all()


def test_duplicates_across_chunks_and_boxes():
    """3000 points of which 1500 are copies of one point, shuffled: after the Morton sort the copies fill six 256-chunks across two
    boxes with b2 == 0 (the pruning rule must still let the other points' searches through).  The copies' result is exactly 0."""
    rng = np.random.default_rng(12)
    pts = rng.normal(size=(3000, 3)).astype(np.float32)
    copy = np.zeros(3000, bool); copy[rng.permutation(3000)[:1500]] = True
    pts[copy] = np.array([0.3, -0.2, 0.1], np.float32)
    got, ref = _check(pts, "duplicates")
    assert not got[copy].any() and not ref[copy].any()
    assert (ref[~copy] > 0).all()


def test_one_morton_cell():
    """A cluster of 3000 points with spread 1e-4 and 8 outliers at (+-1e3, +-1e3, +-1e3): the extent is 2e3, a cell 2 wide, the whole
    cluster falls into ONE Morton cell and the sort leaves it in input order — no spatial order inside three boxes.  Still exact."""
    rng = np.random.default_rng(13)
    cluster = (rng.normal(size=(3000, 3)) * 1e-4).astype(np.float32)
    far = np.array([[sx, sy, sz] for sx in (-1e3, 1e3) for sy in (-1e3, 1e3) for sz in (-1e3, 1e3)], np.float32)
    pts = np.concatenate([cluster, far])[rng.permutation(3008)]
    q = np.floor((pts - pts.min(0)) / (pts.max(0) - pts.min(0)) * 1023.0)
    assert len(np.unique(q[np.abs(pts).max(1) < 1.0], axis=0)) == 1      # (the case is what it says)
    got, ref = _check(pts, "one cell")
    assert (ref > 0).all()


def test_large_offset():
    """A normal cloud translated by (1e4, -1e4, 1e4): coordinates carry ~1e-3 absolute resolution, but the reference reads the SAME fp32
    inputs, differences of fp32 numbers this close are exact in fp32, and only the squares and their sum round.  Measured on this input:
    the oracle run in fp32 (-DORACLE_F32) deviates from fp64 by at most 4.0e-8 relative — the existing rtol of 1e-5 holds as it is."""
    from oracle.surfel_oracle import Oracle
    rng = np.random.default_rng(14)
    pts = (rng.normal(size=(5000, 3)) + np.array([1e4, -1e4, 1e4])).astype(np.float32)
    ref32 = Oracle("f32").knn_dist2(pts); ref = _oracle(pts)
    print("large offset: oracle fp32 against fp64, worst relative deviation %.3e" % np.max(np.abs(ref32 - ref) / ref))
    got, _ = _check(pts, "large offset")
    assert (ref > 0).all()


def test_order_invariance():
    """The result for a permuted input is the permuted result, bit for bit: a point meets the same candidates in another order, every
    distance is computed from the same pair by the same expression ((p - q)^2 is symmetric in fp32), and update3 keeps the three smallest
    whatever the order they arrive in."""
    rng = np.random.default_rng(15)
    pts = _cloud("mixed", 5000, seed=15)
    perm = rng.permutation(5000)
    got = _device(pts); got_perm = _device(pts[perm])
    assert np.array_equal(got_perm, got[perm]), "%d of 5000 results differ" % int((got_perm != got[perm]).sum())
    assert np.allclose(got, _oracle(pts), rtol=RTOL, atol=ATOL) and (got > 0).all()
