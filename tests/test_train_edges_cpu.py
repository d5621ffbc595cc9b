"""The bar of tests/test_gpu_train_edges.py, established without a GPU: the oracle's formulas (oracle/train_oracle.py) run in torch
fp32 on the CPU hold every element of every edge-shape case at the tolerance stated in tests/test_gpu_train.py (yard <= 1), the
judge rejects single planted errors that the share-of-elements judge accepts, and the oracle is defined at frames without normals.
Run with -s to print the yard table of LOSSEDGES.md ("Edge-shape bar of the loss kernels")."""
import numpy as np
import pytest
import torch

import train_edge_cases as E
from oracle import train_oracle as O


def _report(tag, yard):
    print("YARD %-34s %s" % (tag, "  ".join("%s %.3g" % kv for kv in yard.items())))
    for k, v in yard.items():
        assert v <= 1.0, (tag, k, v)


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("hw", E.SSIM_W11)
def test_fp32_oracle_holds_every_element_ssim_l1(hw, kind):
    ref, yard = E.photo_reference(hw[0], hw[1], kind)
    _report("ssim11 %dx%d %s" % (hw[0], hw[1], kind), yard)
    o = O.photometric(*E.photo_inputs(hw[0], hw[1], kind), 0.2)        # the dtype-generic restatement is the oracle's own in fp64
    for k in ("g_l1", "g_ssim", "g_loss"):
        assert np.array_equal(o[k], ref[k])
    assert (o["l1"], o["ssim"], o["loss"]) == (ref["l1"], ref["ssim"], ref["loss"])
    img, gt = E.photo_inputs(hw[0], hw[1], kind)
    ties = (img == gt)
    assert (ref["g_l1"][ties] == 0).all()                                    # the planted sign(0) = 0 pixels
    assert (ties[:, 0, 0].all() and ties[:, -1, -1].all()) == (max(hw) > 2)   # (none where every pixel is a corner)


@pytest.mark.parametrize("case", E.SSIM_OTHER)
def test_fp32_oracle_holds_every_element_other_windows(case):
    ws, H, W = case
    _, yard = E.photo_reference(H, W, "noise", ws)
    _report("ssim%d %dx%d noise" % (ws, H, W), yard)


@pytest.mark.parametrize("hw", E.SSIM_PER_IMAGE)
def test_fp32_oracle_holds_every_element_per_image(hw):
    ref, yard = E.per_image_reference(*hw)
    _report("ssim11 per-image %dx%d" % hw, yard)
    imgs, gts = E.per_image_inputs(*hw)
    whole = E.photometric_t(imgs[1], gts[1], torch.float64)              # image b's gradient is its own mean's, times its weight
    assert np.allclose(ref["g_ssim"][1], E.PER_IMAGE_WEIGHTS[1] * whole["g_ssim"], rtol=1e-12, atol=1e-12 * np.abs(ref["g_ssim"]).max()) and ref["ssim"][1] == whole["ssim"]


@pytest.mark.parametrize("ratio", E.POST_RATIOS)
@pytest.mark.parametrize("case", E.POST_CASES)
def test_fp32_oracle_holds_every_element_post(case, ratio):
    W, H, holes = case
    ref, yard = E.post_reference(W, H, holes, ratio)
    _report("post %dx%d%s r%g" % (W, H, " holes" if holes else "", ratio), yard)
    # the restatement on the camera block is the oracle's render_post in fp64
    am, wm, cam = E.post_inputs(W, H, holes)
    mine = E.render_post_t_np(am, wm, cam, ratio, *E.POST_LAMBDAS, torch.float64)
    for k in ("maps", "g_maps", "g_reg"):
        ok = np.isfinite(ref[k])
        assert np.array_equal(ok, np.isfinite(mine[k])) and np.allclose(mine[k][ok], ref[k][ok], rtol=1e-9, atol=1e-12), k
    if holes:
        placed = E.hole_pixels(H, W)
        for k in ("g_maps", "g_reg"):
            bad = ~np.isfinite(ref[k]).all(axis=0)
            assert sorted((int(y), int(x)) for y, x in zip(*np.nonzero(bad))) == placed
    else:
        assert np.isfinite(ref["g_maps"]).all() and np.isfinite(ref["g_reg"]).all()


@pytest.mark.parametrize("hw", E.FUSED_SHAPES)
def test_fp32_oracle_holds_every_element_fused_arguments(hw):
    H, W = hw
    ratio, lam, ln, ld, _ = E.FUSED_ARGS
    _, yard = E.post_reference(W, H, False, ratio, ln, ld)
    _report("fused post %dx%d" % (W, H), yard)
    _, yard = E.photo_reference(H, W, "noise", 11, lam)
    _report("fused ssim11 %dx%d" % (H, W), yard)


def test_judge_rejects_planted_errors_the_share_judge_accepts():
    """One wrong corner, one tile-seam column 1 % off, one element zeroed: hold_all rejects each; grad_ok, the judge of
    tests/test_gpu_train.py (>= 99.9 % of elements and a cosine), accepts the corner and the zeroed element."""
    from test_gpu_train import grad_ok
    H, W = 203, 331                                # the frame of test_l1_ssim_vs_oracle_large_and_reproducible
    g = E.photometric_t(*E.photo_case(H, W, "noise", 9), torch.float64)["g_ssim"]
    tol = E.grad_tol(g)
    assert E.hold_all("unplanted", g, g, *tol) == 0.0
    corner = g.copy(); corner[0, 0, 0] += 0.05 * np.abs(g).mean()
    column = g.copy(); column[:, :, 32] *= 1.01
    zeroed = g.copy(); zeroed[np.unravel_index(np.argmin(np.abs(np.abs(g) - np.abs(g).mean())), g.shape)] = 0.0      # an element of typical size
    for name, planted in (("corner", corner), ("seam column", column), ("zeroed", zeroed)):
        with pytest.raises(AssertionError):
            E.hold_all("planted " + name, planted, g, *tol, yard=0.25)
    grad_ok(corner, g)
    grad_ok(zeroed, g)
    # a device value that is not finite, and a difference under a zero tolerance, count as failures
    nan = g.copy(); nan[1, 5, 7] = np.nan
    with pytest.raises(AssertionError):
        E.hold_all("planted nan", nan, g, *tol)
    with pytest.raises(AssertionError):
        E.hold_all("zero tolerance", np.array([0.0, 1e-30]), np.zeros(2), 0.0, 2e-3)


@pytest.mark.parametrize("wh", E.POST_NO_NORMAL + ((1, 7), (7, 2)))
def test_oracle_without_normals(wh):
    W, H = wh
    am, wm, cam = E.post_case(H, W, 5)
    for ratio in E.POST_RATIOS:
        o = O.render_post_np(am, cam["wvt"], cam["fpt"], W, H, ratio, wmaps=wm, lambda_normal=0.05, lambda_dist=10.0)
        assert (o["maps"][6:9] == 0).all() and o["normal_err_mean"] == 1.0
        assert np.isfinite(o["g_maps"]).all() and np.isfinite(o["g_reg"]).all()
        assert (o["g_reg"][:6] == 0).all() and np.allclose(o["g_reg"][6], 10.0 / (W * H), rtol=1e-15)
