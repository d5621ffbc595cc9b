"""CPU half of the input-setting parity cases (tests/input_cases.py): every case compares something, and the oracle run in plain
fp32 meets the bars tests/test_gpu_inputs.py holds the device to.

The all-element bar of helpers.check_grads (>= 99.9 % of the elements within tolerance, or at most 3 surfels off) is a fair bar for
the device only where any fp32 implementation of the algorithm meets it.  So the same algorithm in fp32 (oracle -DORACLE_F32) is held
against the fp64 run here, on the same fp32 depth keys, with the same helpers and the same cotangents as the GPU test.  Run with -s,
the test prints each case's figures."""
import functools

import numpy as np
import pytest

import input_cases as IC
from helpers import check_grads, check_image_arrays, grad_figures, image_figures, oracle_forward, oracle_grads


def cotangents(a):
    rng = np.random.default_rng(5)
    return rng.normal(size=(3, a["H"], a["W"])).astype(np.float32), rng.normal(size=(7, a["H"], a["W"])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _runs(name, size):
    """(arguments, fp64 forward, fp64 gradients, fp32 forward, fp32 gradients) of one case, both on the fp32 run's own depths as keys"""
    from oracle.surfel_oracle import Oracle
    a = IC.case(name, size)
    o64, o32 = Oracle("f64"), Oracle("f32")
    dk = oracle_forward(o32, a)[4].depths.astype(np.float32)
    f64 = oracle_forward(o64, a, depth_key=dk)
    f32 = oracle_forward(o32, a, depth_key=dk)
    gC, gO = cotangents(a)
    return a, f64, o64.rasterize_backward(f64[4], gC, gO), f32, o32.rasterize_backward(f32[4], gC, gO)


@pytest.mark.parametrize("name,size", IC.PAIRS)
def test_case_compares_something(name, size):
    a, (R, col, oth, radii, st), og, _, _ = _runs(name, size)
    P = a["means3D"].shape[0]
    M, D = IC.sh_shape(name)
    nb = (D + 1) * (D + 1)
    assert a["shs"].shape == (P, M, 3) and a["shs"].flags["C_CONTIGUOUS"] and a["sh_degree"] == D
    assert a["scale_modifier"] == IC.modifier(name)
    assert R > 0
    assert (radii > 0).mean() >= 0.9, "only %.3f of the surfels are visible" % (radii > 0).mean()
    assert (radii[(P - 1) // 64 * 64:] > 0).any(), "no visible surfel in the last wave"
    assert og.dL_dsh.shape == (P, M, 3) and np.abs(og.dL_dsh[:, 0]).max() > 0
    assert np.abs(og.dL_dscales).max() > 0 and np.abs(og.dL_dmeans3D).max() > 0
    if D > 0:
        assert np.abs(og.dL_dsh[:, 1:nb]).max() > 0
    if M > nb:
        assert not og.dL_dsh[:, nb:].any()


@pytest.mark.parametrize("name,size", IC.PAIRS)
def test_plain_fp32_meets_the_bars(name, size):
    a, (R, col, oth, radii, st), og, (R32, col32, oth32, radii32, st32), og32 = _runs(name, size)
    g32 = oracle_grads(og32)
    print("%s-%s fp32 reference: images min %.5f | %s" % (name, size, min(f for _, f in image_figures(col32, oth32, col, oth)),
          ", ".join("%s %.5f / %d off" % (k, f, bad) for k, f, bad, _ in grad_figures(g32, og))))
    assert np.array_equal(radii32, radii) and R32 == R
    check_image_arrays(col32, oth32, col, oth)
    check_grads(g32, og)


def test_the_unit_changes_change_nothing():
    """k = 1 rebuilds the scene's own projection bit for bit, so the aniso cases differ from the tested scenes by k alone; a store
    cut to 16 coefficients and scale_modifier 1 are the scene itself."""
    import synthetic
    from helpers import scene_args
    for s in IC.SIZES.values():
        sc = synthetic.make_scene(s["P"], s["W"], s["H"], seed=s["seed"], px_radius=s["px_radius"])
        a = scene_args(sc)
        IC.anisotropic(a, 1.0)
        assert a["tanfovy"] == float(sc["tanfovy"]) and np.array_equal(a["projmatrix"], sc["projmatrix"])
    a = IC.case("aniso1.25", "s64")
    b = IC.case("mod2", "s64")
    assert a["tanfovy"] * 1.25 == pytest.approx(b["tanfovy"], rel=1e-12) and a["tanfovx"] == b["tanfovx"]
    # (row-vector convention: column 1 of the full projection carries fy; every other column is the square camera's)
    assert np.allclose(a["projmatrix"][:, 1], 1.25 * b["projmatrix"][:, 1], rtol=1e-6, atol=0)
    assert np.array_equal(np.delete(a["projmatrix"], 1, 1), np.delete(b["projmatrix"], 1, 1))


def test_offcentre_moves_the_principal_point():
    """Pm[0, 2], Pm[1, 2] shift every projected centre by 0.15 W / 2 and -0.10 H / 2 pixels (7.5 % and 5 % of the frame)"""
    a, b = IC.case("offcentre", "s300"), IC.case("mod2", "s300")
    hom = np.concatenate([a["means3D"].astype(np.float64), np.ones((a["means3D"].shape[0], 1))], 1)
    pa, pb = hom @ a["projmatrix"].astype(np.float64), hom @ b["projmatrix"].astype(np.float64)
    d = pa[:, :2] / pa[:, 3:] - pb[:, :2] / pb[:, 3:]
    assert np.allclose(d, [IC.OFFCENTRE], atol=1e-5)


def test_stress_cases_share_the_parity_scenes():
    a = IC.stress_case("huge", 11, "all")
    base = IC._stress_scene("huge", 11)
    assert a["means3D"].shape == (1500, 3) and (a["W"], a["H"]) == (208, 136)
    assert np.array_equal(a["scales"], base["scales"]) and a["scale_modifier"] == 2.0
    assert a["shs"].shape == (1500, 4, 3) and a["sh_degree"] == 1 and a["tanfovy"] == pytest.approx(float(base["tanfovy"]) / 1.25)
    import test_gpu_parity
    assert test_gpu_parity._stress_scene is IC._stress_scene
