"""-m gpu tests of preprocess_fwd_kernel<true>, the preprocess that fetches a wave's SH block (64 surfels x 192 B, contiguous) by LDS-DMA.

By size it runs on frames of >= 2^19 surfels only, which the suite reaches with two scenes whose counts are multiples of 64, at SH
degree 3 with 16 coefficients.  surfel_set_option("preprocess_dma", 2) forces it at any size, 0 forbids it: here it is held
BIT-IDENTICAL to the direct-load kernel and within the parity tolerances of the fp64 oracle (tests/test_gpu_parity.py states them,
tests/determinacy.py holds the constants) at the sizes where a wave or a workgroup is partly filled — the `p < npieces` guard of the
DMA, behind which lanes would read another surfel's LDS slot — and on the inputs for which the <true> instantiation falls back to
direct loads inside the kernel (degree < 3, a coefficient count other than 16, colors_precomp).  The same LDS data feeds the colour
and the d(colour) / d(direction) rows preprocess_bwd reads, so images AND every gradient are compared, with the backward once on the
rows and once on the re-read SH block (SURFEL_OPT_PBWD_NO_JAC).  Every test restores the option's default (1) in a `finally`."""
import functools

import numpy as np
import pytest

import determinacy as D
from helpers import HipRun, check_binning, check_grads, check_images, cosine, frac_close, oracle_forward, scene_args

pytestmark = pytest.mark.gpu

W, H, PX_RADIUS = 96, 80, 4.0
SIZES = (1, 63, 64, 65, 127, 191, 192, 193, 255, 256, 257, 300, 4099)
# (seed = P: counted on the CPU with the oracle, every one of these scenes has a surfel of the last, partly filled wave that reaches the
# image with a non-zero colour gradient — which every test below asserts on the device's own results)
SWITCH = 1 << 19            # launch_preprocess_fwd's rule at the option's default


def _args(P, seed=None, degree=3, w=W, h=H, px_radius=PX_RADIUS):
    import synthetic
    sc = synthetic.make_scene(P, w, h, seed=P if seed is None else seed, px_radius=px_radius)
    sc["bg"] = np.array([0.2, 0.5, 0.9], np.float32)
    a = scene_args(sc)
    a["sh_degree"] = degree
    return a


def _cotangents(a, seed=5):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(3, a["H"], a["W"])).astype(np.float32), rng.normal(size=(7, a["H"], a["W"])).astype(np.float32)


def _frame(a, dma, colors_precomp=None, reread=True):
    """forward + backward(s) under surfel_set_option("preprocess_dma", dma); everything the frame produced, as host arrays.
    dma None: the option is left alone.  reread: a second backward on the re-read SH block (SURFEL_OPT_PBWD_NO_JAC)."""
    import surfel_native as n
    lib = n.load()
    gC, gO = _cotangents(a)
    try:
        if dma is not None:
            assert lib.surfel_set_option(b"preprocess_dma", dma) == 0
        run = HipRun(a, colors_precomp=colors_precomp).forward()
        out = dict(R=run.R, radii=run.radii.cpu().numpy(), color=run.color.cpu().numpy(), others=run.others.cpu().numpy(), depths=run.depths())
        skip = ("sh",) if run.M == 0 else ()          # (colors_precomp: no SH gradient is asked for)
        for tag, dbg in (("rows", 0), ("reread", n.OPT_PBWD_NO_JAC))[:2 if reread else 1]:
            run.debug = dbg
            out[tag] = {k: v for k, v in run.backward(gC, gO).items() if k not in skip}
        run.debug = 0
    finally:
        lib.surfel_set_option(b"preprocess_dma", 1)
    return out, run


def _last_wave(P):
    """first surfel of the last wave (partly filled unless P is a multiple of 64)"""
    return (P - 1) // 64 * 64


def _assert_compared_something(P, out):
    """A case that compares two empty frames is not a case: instances, a surfel of the last wave that reached the image (its colour
    gradient is non-zero), non-zero gradients through both readers of the SH data."""
    first = _last_wave(P)
    assert out["R"] > 0
    assert (out["radii"][first:] > 0).any(), "no visible surfel in the last wave (P = %d)" % P
    for tag in ("rows", "reread"):
        if tag in out:
            g = out[tag]
            assert np.abs(g["colors"][first:]).max() > 0, "no surfel of the last wave reached the image (P = %d)" % P
            assert np.abs(g["means3D"][first:]).max() > 0
            if "sh" in g:
                assert np.abs(g["sh"][first:]).max() > 0


def _assert_identical(x, y, what):
    assert x["R"] == y["R"], what
    for k in ("radii", "color", "others", "depths"):
        assert np.array_equal(x[k], y[k]), "%s: %s differs" % (what, k)
    assert np.isfinite(x["color"]).all() and np.isfinite(x["others"]).all() and x["others"].shape[0] == 7
    for tag in ("rows", "reread"):
        assert (tag in x) == (tag in y)
        if tag in x:
            assert sorted(x[tag]) == sorted(y[tag])
            for k in x[tag]:
                assert np.isfinite(x[tag][k]).all(), (what, tag, k)
                assert np.array_equal(x[tag][k], y[tag][k]), "%s: dL/d%s differs (%s)" % (what, k, tag)


@functools.lru_cache(maxsize=None)
def _pair(P):
    """the frame of _args(P) under forced direct loads (0) and forced DMA (2), rendered once for the tests that share it"""
    a = _args(P)
    direct, _ = _frame(a, 0)
    dma, run = _frame(a, 2)
    return a, direct, dma, run


@pytest.mark.parametrize("P", SIZES)
def test_dma_is_bit_identical_to_direct_loads(P):
    """1 / 63 / 65 ... surfels in the last wave, one to seventeen workgroups: R, radii, colour, the 7-plane allmap and every gradient
    (through the Jacobian rows and through the re-read SH block) have the same bits under preprocess_dma 0 and 2."""
    a, direct, dma, _ = _pair(P)
    _assert_compared_something(P, dma)
    _assert_identical(direct, dma, "P = %d" % P)


@pytest.mark.parametrize("P", SIZES)
def test_dma_matches_the_oracle(P):
    """the forced-DMA frame against the fp64 oracle: the checks of test_forward_backward_small"""
    from oracle.surfel_oracle import Oracle
    a, _, dma, run = _pair(P)
    _assert_compared_something(P, dma)
    o = Oracle("f64")
    R, col, oth, radii, st = oracle_forward(o, a, depth_key=dma["depths"])
    check_binning(run, R, radii)
    check_images(run, col, oth, st)
    assert np.array_equal(run.color.cpu().numpy(), dma["color"])      # (run still holds the forced-DMA frame)
    gC, gO = _cotangents(a)
    og = o.rasterize_backward(st, gC, gO)
    check_grads(dma["rows"], og)
    check_grads(dma["reread"], og)


FALLBACK_P = 300            # 4 full waves + one of 44 surfels, two workgroups


def _fallback_case(kind):
    """(scene arguments, colors_precomp) of the inputs for which preprocess_fwd_kernel<true> keeps the direct loads"""
    if kind in ("degree0", "degree1", "degree2"):      # what the trainer passes below full degree: 16 coefficients, a lower active degree
        return _args(FALLBACK_P, degree=int(kind[-1])), None
    a = _args(FALLBACK_P)
    if kind == "M20":                                   # degree-3 data in a wider store: the coefficients behind the 16th are never read
        extra = np.random.default_rng(3).normal(0.0, 1.0, (FALLBACK_P, 4, 3)).astype(np.float32)
        a["shs"] = np.ascontiguousarray(np.concatenate([a["shs"], extra], 1))
        return a, None
    assert kind == "precomp"
    return a, np.random.default_rng(1).uniform(0, 1, (FALLBACK_P, 3)).astype(np.float32)


@pytest.mark.parametrize("kind", ["degree0", "degree1", "degree2", "M20", "precomp"])
def test_in_kernel_fallbacks(kind):
    """Forced DMA on inputs the DMA does not serve (the first 3000 iterations of every large scene; every precomputed-colour render):
    the <true> instantiation must take its direct loads — bit-identical to preprocess_dma 0, images and gradients, and within the
    parity tolerances of the oracle, at a size with a partly filled last wave."""
    from oracle.surfel_oracle import Oracle
    a, cols = _fallback_case(kind)
    direct, _ = _frame(a, 0, colors_precomp=cols)
    dma, run = _frame(a, 2, colors_precomp=cols)
    _assert_compared_something(FALLBACK_P, dma)
    _assert_identical(direct, dma, kind)
    o = Oracle("f64")
    R, col, oth, radii, st = oracle_forward(o, a, colors_precomp=cols, depth_key=dma["depths"])
    check_binning(run, R, radii)
    check_images(run, col, oth, st)
    gC, gO = _cotangents(a)
    og = o.rasterize_backward(st, gC, gO)
    if kind == "M20":
        assert dma["rows"]["sh"].shape == (FALLBACK_P, 20, 3) and not dma["rows"]["sh"][:, 16:].any()
    if cols is None:
        check_grads(dma["rows"], og)
        check_grads(dma["reread"], og)
    else:      # no SH gradient: the element test and bars of test_precomp_and_override_color, on every gradient this input has
        for tag in ("rows", "reread"):
            for k, ref in [("colors", og.dL_dcolors), ("opacity", og.dL_dopacity), ("means2D", og.dL_dmean2D), ("means3D", og.dL_dmeans3D),
                           ("scales", og.dL_dscales), ("rots", og.dL_drots)]:
                x = dma[tag][k].reshape(ref.shape)
                scale = np.abs(ref).mean() + 1e-30
                assert frac_close(x, ref, 1e-4 * scale, D.G_RTOL) >= D.PASS_FRAC, (tag, k)
                assert cosine(x, ref) >= D.COS_MIN, (tag, k)


# The natural switch.  640 x 480 (1200 tiles), px_radius 0.5: nearly every surfel is a minimum-radius (3 px) splat.  Counted on the CPU with the
# oracle's tile rectangles (an upper bound of what the device emits), seed 11: 778 000 instances at either size, 648 per tile on average,
# 728 in the longest list (the rank-sort fallback of the per-tile depth sort starts at 4096); 48 / 32 visible surfels in the last wave.
SWITCH_FRAME = dict(w=640, h=480, px_radius=0.5)


@pytest.mark.parametrize("P", [SWITCH - 1, SWITCH + 37])
def test_switch_by_size(P):
    """The option at its default: 2^19 - 1 surfels keep the direct loads, 2^19 + 37 take the DMA with a last wave of 37 surfels.  Both
    must be bit-identical to preprocess_dma 0 on the same scene, images and gradients.  The only case above a few thousand surfels; no
    oracle at this size."""
    import surfel_native as n
    a = _args(P, seed=11, **SWITCH_FRAME)
    assert n.load().surfel_set_option(b"preprocess_dma", 1) == 0
    default, _ = _frame(a, None, reread=False)
    direct, _ = _frame(a, 0, reread=False)
    _assert_compared_something(P, default)
    _assert_identical(direct, default, "P = %d" % P)


def test_option_hygiene():
    """values outside 0..2 clamp (they are accepted, and the frame is still the frame), the option holds across frames, and setting
    1 again restores the rule by size — below 2^19 surfels that is the direct-load kernel, whose result is the one under 0"""
    import surfel_native as n
    lib = n.load()
    try:
        a257, direct257, dma257, _ = _pair(257)
        a65, direct65, _, _ = _pair(65)
        for v in (-3, 7, 1 << 20):
            assert lib.surfel_set_option(b"preprocess_dma", v) == 0
            out, _ = _frame(a257, None, reread=False)
            _assert_identical({k: v_ for k, v_ in direct257.items() if k != "reread"}, out, "preprocess_dma = %d" % v)
        assert lib.surfel_set_option(b"preprocess_dma", 2) == 0
        for a, ref in ((a257, direct257), (a65, direct65), (a257, direct257)):      # three frames under one setting
            run = HipRun(a).forward()
            assert run.R == ref["R"] and np.array_equal(run.color.cpu().numpy(), ref["color"]) and np.array_equal(run.others.cpu().numpy(), ref["others"])
        assert lib.surfel_set_option(b"preprocess_dma", 1) == 0
        out, _ = _frame(a257, None)
        _assert_compared_something(257, out)
        _assert_identical(direct257, out, "default after 2")
        _assert_identical(dma257, out, "default after 2 (against the forced DMA)")
    finally:
        lib.surfel_set_option(b"preprocess_dma", 1)
