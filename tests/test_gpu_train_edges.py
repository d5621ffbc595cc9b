"""The loss and post-processing kernels (csrc/train_loss_body.h, train_post_body.h, train_fused.hip) at the frame sizes where
their tile, halo and border code can go wrong — EVERY element held to the fp64 oracle (oracle/train_oracle.py) at the tolerances
stated in tests/test_gpu_train.py, through the public wrappers only.  Cases, references and the judge: tests/train_edge_cases.py;
the bar comes from the oracle's own fp32 run on the CPU (tests/test_train_edges_cpu.py), never from the device.
"""
import numpy as np
import pytest

import train_edge_cases as E

pytestmark = pytest.mark.gpu


def dev():
    import torch
    return torch.device("cuda:0")


def T(a):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(dev())      # (a copy: the shared inputs are read-only)


def N(t):
    return t.detach().cpu().numpy()


def _ssim_l1(H, W, kind, tag):
    """l1_loss, ssim, their gradients and the fused photometric loss of one window-11 case against the oracle."""
    import torch
    import surfel_losses as L
    img, tgt = E.photo_inputs(H, W, kind)
    ref, yard = E.photo_reference(H, W, kind)
    x = T(img).requires_grad_(True); y = T(tgt)
    l1 = L.l1_loss(x, y); s = L.ssim(x, y)
    E.hold_all(tag + " l1", float(l1.detach()), ref["l1"], E.TOL_L1, 0, yard["l1"])
    E.hold_all(tag + " ssim", float(s.detach()), ref["ssim"], E.TOL_SSIM, 0, yard["ssim"])
    g_l1, = torch.autograd.grad(l1, x); g_s, = torch.autograd.grad(s, x)
    assert tuple(g_l1.shape) == img.shape and tuple(g_s.shape) == img.shape
    E.hold_all(tag + " g_l1", N(g_l1), ref["g_l1"], *E.L1_GRAD_TOL, yard=yard["g_l1"])            # includes the sign(0) = 0 ties
    E.hold_all(tag + " g_ssim", N(g_s), ref["g_ssim"], *E.grad_tol(ref["g_ssim"]), yard=yard["g_ssim"])
    x2 = T(img).requires_grad_(True)
    loss, means = L.photometric_loss(x2, y, 0.2)                                                  # fused form, train.py:72-74
    E.hold_all(tag + " loss", float(loss.detach()), ref["loss"], E.TOL_LOSS, 0, yard["loss"])
    E.hold_all(tag + " loss l1", float(means[0]), ref["l1"], E.TOL_L1, 0, yard["l1"])
    E.hold_all(tag + " loss ssim", float(means[1]), ref["ssim"], E.TOL_SSIM, 0, yard["ssim"])
    loss.backward()
    E.hold_all(tag + " g_loss", N(x2.grad), ref["g_loss"], *E.grad_tol(ref["g_loss"]), yard=yard["g_loss"])


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("hw", E.SSIM_W11)
def test_ssim_l1_every_element(hw, kind):
    _ssim_l1(hw[0], hw[1], kind, "ssim11 %dx%d %s" % (hw[0], hw[1], kind))


@pytest.mark.parametrize("case", E.SSIM_OTHER)
def test_ssim_other_windows_every_element(case):
    import surfel_losses as L
    ws, H, W = case
    img, tgt = E.photo_inputs(H, W, "noise")
    ref, yard = E.photo_reference(H, W, "noise", ws)
    tag = "ssim%d %dx%d" % (ws, H, W)
    x = T(img).requires_grad_(True)
    s = L.ssim(x, T(tgt), window_size=ws)
    E.hold_all(tag + " ssim", float(s.detach()), ref["ssim"], E.TOL_SSIM, 0, yard["ssim"])
    s.backward()
    E.hold_all(tag + " g_ssim", N(x.grad), ref["g_ssim"], *E.grad_tol(ref["g_ssim"]), yard=yard["g_ssim"])


@pytest.mark.parametrize("hw", E.SSIM_PER_IMAGE)
def test_ssim_per_image_every_element(hw):
    import surfel_losses as L
    imgs, gts = E.per_image_inputs(*hw)
    ref, yard = E.per_image_reference(*hw)
    tag = "ssim11 per-image %dx%d" % hw
    x = T(imgs).requires_grad_(True)
    got = L.ssim(x, T(gts), size_average=False)
    assert tuple(got.shape) == (len(E.PER_IMAGE_WEIGHTS),)
    E.hold_all(tag + " ssim", N(got), ref["ssim"], E.TOL_SSIM, 0, yard["ssim"])
    (got * T(np.array(E.PER_IMAGE_WEIGHTS))).sum().backward()
    E.hold_all(tag + " g_ssim", N(x.grad), ref["g_ssim"], *E.grad_tol(ref["g_ssim"]), yard=yard["g_ssim"])


class _View:
    def __init__(self, cam):
        self.world_view_transform = T(cam["wvt"]); self.full_proj_transform = T(cam["fpt"])
        self.image_width, self.image_height = cam["W"], cam["H"]


def _post_grad(tag, g, gref, yard, holes, placed):
    ok = E.hole_rule(g, gref, placed) if holes else None
    if not holes:
        assert np.isfinite(gref).all()
    return E.hold_all(tag, g, gref, *E.grad_tol(gref), yard=yard, where=ok)


@pytest.mark.parametrize("ratio", E.POST_RATIOS)
@pytest.mark.parametrize("case", E.POST_CASES)
def test_render_post_every_element(case, ratio):
    import surfel_render as R
    W, H, holes = case
    am, wm, cam = E.post_inputs(W, H, holes)
    ref, yard = E.post_reference(W, H, holes, ratio)
    placed = E.hole_pixels(H, W) if holes else []
    tag = "post %dx%d%s r%g" % (W, H, " holes" if holes else "", ratio)
    v = _View(cam)
    a = T(am).requires_grad_(True)
    maps = R.render_post(a, v, ratio)
    m = N(maps)
    assert m.shape == (9, H, W)
    E.hold_all(tag + " maps", m[:6], ref["maps"][:6], *E.MAP_TOL, yard=yard["maps"])
    E.hold_all(tag + " surf_normal", m[6:], ref["maps"][6:], *E.MAP_TOL, yard=yard["surf_normal"])
    (maps * T(wm)).sum().backward()
    g = N(a.grad)
    _post_grad(tag + " g_maps", g, ref["g_maps"], yard["g_maps"], holes, placed)
    a2 = T(am).requires_grad_(True)
    ln, ld = E.POST_LAMBDAS
    reg, means = R.regularizers(a2, v, ratio, ln, ld)
    E.hold_all(tag + " normal_err", float(means[0]), ref["normal_err_mean"], E.TOL_NORMAL_ERR, 0, yard["normal_err"])
    E.hold_all(tag + " dist", float(means[1]), ref["dist_mean"], E.TOL_DIST, 0, yard["dist"])
    reg.backward()
    g2 = N(a2.grad)
    _post_grad(tag + " g_reg", g2, ref["g_reg"], yard["g_reg"], holes, placed)
    if (W, H) in E.POST_NO_NORMAL:
        # no pixel has a normal: surf_normal is exactly zero, nothing flows back through the points, and the depth channels get the
        # upstream gradient of surf_depth alone (d surf_depth / d a0 = (1 - ratio) / a1, d / d a1 = -(1 - ratio) a0 / a1^2, d / d a5 = ratio)
        assert (m[6:9] == 0).all()
        a64, w64 = am.astype(np.float64), wm.astype(np.float64)
        up = np.zeros((7, H, W))
        up[0] = w64[5] * (1 - ratio) / a64[1]
        up[1] = w64[0] - w64[5] * (1 - ratio) * a64[0] / a64[1] ** 2
        up[5] = w64[5] * ratio
        for ch in (0, 1):
            E.hold_all(tag + " upstream a%d" % ch, g[ch], up[ch], *E.grad_tol(up[ch]))
        assert np.array_equal(g[5], wm[5] * np.float32(ratio))                # one fp32 multiply: to the bit
        assert (g2[:6] == 0).all() and (g2[6] == np.float32(ld / (H * W))).all()


def fused_and_separate(img, tgt, allmap, consts, args):
    """The body of tests/test_gpu_train.py::test_fused_loss_launches_keep_the_bits on given inputs: the four combinations of
    FUSED_LOSS and defer_scalars give the same bits.  Returns (total, scalars, image gradient, allmap gradient) of the first."""
    import torch
    import surfel_losses as L
    ratio, lam, ln, ld, up = args
    d = img.device
    res = []
    try:
        # separate launches | fused halves + finalize launch | fused halves, loss scalars deferred to an extra workgroup of the backward
        for fused, defer in ((False, False), (True, False), (True, True), (False, True)):
            L.FUSED_LOSS = fused
            x = img.clone().requires_grad_(True); am = allmap.clone().requires_grad_(True)
            total, sc = L.train_loss(x, am, tgt, consts, ratio, lam, ln, ld, defer_scalars=defer)
            total.backward(torch.full((), up, device=d))
            res.append((total.detach().clone(), sc.clone(), x.grad.clone(), am.grad.clone()))
    finally:
        L.FUSED_LOSS = True
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.isfinite(a).all() and torch.equal(a, b)
    return res[0]


@pytest.mark.parametrize("hw", E.FUSED_SHAPES)
def test_fused_and_separate_launches_keep_the_bits_at_edges(hw):
    """3, 6 or 12 SSIM workgroups (never a multiple of 8: the padding of the fused grid's SSIM part runs) next to 1 .. 9
    post-processing workgroups; that run's gradients and scalars are also held to the oracle element by element."""
    import surfel_render as R
    H, W = hw
    ratio, lam, ln, ld, up = E.FUSED_ARGS
    img, tgt = E.photo_inputs(H, W, "noise")
    am, wm, cam = E.post_inputs(W, H, False)
    pref, pyard = E.photo_reference(H, W, "noise", 11, lam)
    qref, qyard = E.post_reference(W, H, False, ratio, ln, ld)
    consts = T(R.post_consts(cam["wvt"], cam["fpt"], W, H))
    total, sc, g_img, g_am = fused_and_separate(T(img), T(tgt), T(am), consts, E.FUSED_ARGS)
    tag = "fused %dx%d" % (H, W)
    sc = N(sc)
    E.hold_all(tag + " l1", sc[0], pref["l1"], E.TOL_L1, 0, pyard["l1"])
    E.hold_all(tag + " ssim", sc[1], pref["ssim"], E.TOL_SSIM, 0, pyard["ssim"])
    E.hold_all(tag + " normal_err", sc[2], qref["normal_err_mean"], E.TOL_NORMAL_ERR, 0, qyard["normal_err"])
    E.hold_all(tag + " dist", sc[3], qref["dist_mean"], E.TOL_DIST, 0, qyard["dist"])
    E.hold_all(tag + " loss", sc[4], pref["loss"], E.TOL_LOSS, 0, pyard["loss"])
    assert sc[5] == float(total)
    E.hold_all(tag + " g_image", N(g_img), up * pref["g_loss"], *E.grad_tol(up * pref["g_loss"]), yard=pyard["g_loss"])
    E.hold_all(tag + " g_allmap", N(g_am), up * qref["g_reg"], *E.grad_tol(up * qref["g_reg"]), yard=qyard["g_reg"])
