"""-m gpu parity tests on the input settings no other test varies (tests/input_cases.py): scale_modifier != 1, cameras with
fx != fy or an off-centre principal point, SH stores of 1, 4 and 9 coefficients.

Tolerances and bars are those of tests/test_gpu_parity.py (constants in tests/determinacy.py, checks in tests/helpers.py); this file
adds no number of its own.  tests/test_inputs_cpu.py shows on the CPU that the oracle run in plain fp32 meets the same bars on every
case, so a case that fails here is a kernel or wrapper fault, not a tolerance question.  Run with -s, each case prints the device's
figures in the format of the CPU test's."""
from types import SimpleNamespace

import numpy as np
import pytest

import input_cases as IC
from helpers import HipRun, check_binning, check_grads, check_images, grad_figures, image_figures, oracle_forward
from test_gpu_preprocess_dma import _assert_compared_something, _assert_identical, _cotangents, _frame

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,size", IC.PAIRS)
def test_inputs_match_the_oracle(name, size):
    """test_forward_backward_small on one case: binning, images, gradients against the fp64 oracle on the device's depth keys.  Twice,
    under preprocess_dma 0 and 2, bit-identical (a store of M != 16 coefficients falls back to direct loads inside the DMA kernel), and
    the backward twice, on the forward's d(colour) / d(direction) rows and on the re-read SH block (SURFEL_OPT_PBWD_NO_JAC)."""
    from oracle.surfel_oracle import Oracle
    a = IC.case(name, size)
    P = a["means3D"].shape[0]
    M, D = IC.sh_shape(name)
    nb = (D + 1) * (D + 1)
    direct, _ = _frame(a, 0)
    dma, run = _frame(a, 2)
    _assert_compared_something(P, dma)
    _assert_identical(direct, dma, "%s-%s" % (name, size))
    o = Oracle("f64")
    R, col, oth, radii, st = oracle_forward(o, a, depth_key=dma["depths"])
    check_binning(run, R, radii)
    print("%s-%s device: images min %.5f" % (name, size, min(f for _, f in image_figures(dma["color"], dma["others"], col, oth))), end="")
    check_images(run, col, oth, st)
    gC, gO = _cotangents(a)
    og = o.rasterize_backward(st, gC, gO)
    for tag in ("rows", "reread"):
        g = dma[tag]
        print(" | %s: %s" % (tag, ", ".join("%s %.5f / %d off" % (k, f, bad) for k, f, bad, _ in grad_figures(g, og))), end="")
        check_grads(g, og)
        assert g["sh"].shape == (P, M, 3)
        if D > 0:
            assert np.abs(g["sh"][:, 1:nb]).max() > 0
        if M > nb:      # coefficients above the active degree: written, and exactly zero
            assert np.array_equal(g["sh"][:, nb:], np.zeros((P, M - nb, 3), np.float32))
        mod = a["scale_modifier"]
        if mod != 1.0:      # d/d(scale) of (modifier x scale): the factor is in the gradient exactly once
            og_m = SimpleNamespace(**vars(og)); og_m.dL_dscales = og.dL_dscales / mod
            check_grads(dict(g, scales=g["scales"] / np.float32(mod)), og_m)
    print()
    # the two readings of the SH data: every gradient has the same bits, except dL/dmeans3D where the forward left its rows (M = 16
    # only) — there test_preprocess_bwd_sh_direction_rows's bound.  A short store leaves no rows: both backwards take the same branch.
    for k in dma["rows"]:
        x, ref = dma["reread"][k], dma["rows"][k]
        if k == "means3D" and M == 16:
            assert np.abs(x.astype(np.float64) - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-12
        else:
            assert np.array_equal(x, ref), "dL/d%s differs between the Jacobian rows and the re-read SH block" % k


@pytest.mark.parametrize("variant", IC.STRESS_VARIANTS)
@pytest.mark.parametrize("kind", ["plain", "huge", "needles"])
def test_culls_and_walks_hold_under_the_variants(kind, variant):
    """The bit-identity checks of test_culling_is_exact, test_backward_variants_are_identical and test_binning_paths_are_identical with
    scaled axes, non-square pixels and a short SH store: a footprint bound that assumed square pixels or unscaled axes would remove a
    contributing (pixel, surfel) pair, and that changes bits."""
    import surfel_native as n
    from oracle.surfel_oracle import Oracle
    a = IC.stress_case(kind, 11, variant)
    rng = np.random.default_rng(11)
    gC = rng.normal(size=(3, a["H"], a["W"])).astype(np.float32); gO = rng.normal(size=(7, a["H"], a["W"])).astype(np.float32)

    def frame(fwd_flags, bwd_flags=None):
        run = HipRun(a, debug=fwd_flags).forward()
        if bwd_flags is not None:
            run.debug = bwd_flags
        g = run.backward(gC, gO)
        return run, (run.R, run.color.cpu().numpy(), run.others.cpu().numpy(), run.radii.cpu().numpy(), g)

    def same(x, y, what, count=True):
        assert not count or x[0] == y[0], (what, x[0], y[0])
        assert np.array_equal(x[3], y[3]), "%s: radii differ" % what
        assert np.array_equal(x[1], y[1]), "%s: colour differs" % what
        assert np.array_equal(x[2], y[2]), "%s: allmap differs" % what
        for k in x[4]:
            assert np.isfinite(x[4][k]).all(), "%s: dL/d%s has non-finite entries" % (what, k)
            assert np.array_equal(x[4][k], y[4][k]), "%s: dL/d%s differs (max |d| %.3e)" % (what, k, np.abs(x[4][k].astype(np.float64) - y[4][k]).max())

    tag = "%s-%s" % (kind, variant)
    run, cull = frame(0, n.OPT_BWD_ROWS)
    _, nocull = frame(n.OPT_NO_CULL, n.OPT_BWD_ROWS)
    assert 0 < cull[0] <= nocull[0]
    same(cull, nocull, tag + " culling", count=False)
    Rref, _, _, radii, _ = oracle_forward(Oracle("f64"), a, depth_key=None)
    if np.array_equal(nocull[3], radii):
        assert nocull[0] == Rref, (nocull[0], Rref)
    run.debug = n.OPT_BWD_QUAD
    same(cull, cull[:4] + (run.backward(gC, gO),), tag + " rows / quad walk")
    _, presorted = frame(n.opt_tile_sort(0))
    _, per_tile = frame(n.opt_tile_sort(2))
    same(presorted, per_tile, tag + " binning paths")
    assert presorted[0] == cull[0] and np.array_equal(presorted[1], cull[1]) and np.array_equal(presorted[2], cull[2])


def test_dropin_passes_the_settings_to_both_directions():
    """GaussianRasterizer with scale_modifier 2, fy = 1.25 fx and a [P, 4, 3] SH tensor at degree 1 calls the same library on the same
    inputs as HipRun on case `all`: outputs and gradients bit for bit — a wrapper that dropped a setting on the way to the forward or
    the backward would not."""
    import torch
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    a = IC.case("all", "s300")
    P = a["means3D"].shape[0]
    assert a["scale_modifier"] == 2.0 and a["shs"].shape == (P, 4, 3) and a["sh_degree"] == 1
    gC, gO = _cotangents(a)
    run = HipRun(a).forward()
    g = run.backward(gC, gO)
    dev = torch.device("cuda:0")
    t = lambda x: torch.tensor(x, device=dev)
    rs = GaussianRasterizationSettings(image_height=a["H"], image_width=a["W"], tanfovx=a["tanfovx"], tanfovy=a["tanfovy"], bg=t(a["bg"]),
                                       scale_modifier=2.0, viewmatrix=t(a["viewmatrix"]), projmatrix=t(a["projmatrix"]), sh_degree=1,
                                       campos=t(a["campos"]), prefiltered=False, debug=False)
    p = {k: t(a[k]).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    means2D = torch.zeros_like(p["means3D"], requires_grad=True)
    color, radii, others = GaussianRasterizer(raster_settings=rs)(means3D=p["means3D"], means2D=means2D, shs=p["shs"], colors_precomp=None,
                                                                   opacities=p["opacities"], scales=p["scales"], rotations=p["rotations"], cov3D_precomp=None)
    ((color * t(gC)).sum() + (others * t(gO)).sum()).backward()
    torch.cuda.synchronize()
    assert run.R > 0 and np.array_equal(radii.cpu().numpy(), run.radii.cpu().numpy())
    assert np.array_equal(color.detach().cpu().numpy(), run.color.cpu().numpy())
    assert np.array_equal(others.detach().cpu().numpy(), run.others.cpu().numpy())
    assert p["shs"].grad.shape == (P, 4, 3)
    for k, ref in (("means3D", "means3D"), ("opacities", "opacity"), ("scales", "scales"), ("rotations", "rots"), ("shs", "sh")):
        x = p[k].grad.cpu().numpy()
        assert np.abs(x).max() > 0 and np.array_equal(x, g[ref].reshape(x.shape)), "dL/d%s differs between the drop-in module and the C ABI" % k
    assert np.array_equal(means2D.grad.cpu().numpy(), g["means2D"])


def test_sh_store_argument_errors():
    """A store too short for the degree (4 coefficients at degree 2; none at all behind a non-NULL pointer) is SURFEL_E_INVALID in the
    forward and in the backward (which the forward's check used to stand in for); the message names degree and count."""
    import surfel_native as n
    a = IC.case("M4_D1", "s64")
    gC, gO = _cotangents(a)
    run = HipRun(a); run.D = 2
    with pytest.raises(AssertionError, match="degree 2, 4 coefficients"):
        run.forward()
    assert run.rc == n.E_INVALID
    run = HipRun(IC.case("M1_D0", "s64")); run.M = 0
    with pytest.raises(AssertionError, match="degree 0, 0 coefficients"):
        run.forward()
    assert run.rc == n.E_INVALID
    run = HipRun(a).forward()
    good = run.backward(gC, gO)
    run.D = 2
    with pytest.raises(AssertionError, match="degree 2, 4 coefficients"):
        run.backward(gC, gO)
    assert run.rc == n.E_INVALID
    assert all(bool(v.isnan().all()) for v in run.g.values())      # refused before any kernel ran: the poisoned outputs are untouched
    run.D = 1
    again = run.backward(gC, gO)
    assert run.rc == 0 and all(np.array_equal(good[k], again[k]) for k in good)
