"""Edge-shape cases of the loss and post-processing kernels (csrc/train_loss_body.h, train_post_body.h, train_fused.hip): the
builders, the case lists, the references and the judge shared by tests/test_train_edges_cpu.py and tests/test_gpu_train_edges.py.

Every element is judged (hold_all) at the tolerances stated in tests/test_gpu_train.py.  The bar of a quantity is
max(1, 4 * yard) times its tolerance, where yard is the worst element ratio of the oracle's own formulas run in torch fp32 on the
CPU against their fp64 run (oracle/train_oracle.py) — never anything measured from the device.  4: the device sums separably and
with fused multiply-adds, another order than conv2d and the tensor ops, at the same arithmetic width.  LOSSEDGES.md lists
yard per case ("Edge-shape bar of the loss kernels": per family).
"""
import functools

import numpy as np
import torch

from oracle import train_oracle as O

# ------------------------------------------------------------------------------------------------ tolerances (tests/test_gpu_train.py)
MAP_TOL = (2e-5, 2e-5)           # atol, rtol of the nine maps, surf_normal included
GRAD_RTOL = 2e-3                 # gradients: 2e-3 * mean|ref| + 2e-3 * |ref|
L1_GRAD_TOL = (1e-9, 1e-5)       # the L1 gradient is sign / N: held to rounding
TOL_L1, TOL_SSIM, TOL_LOSS, TOL_NORMAL_ERR, TOL_DIST = 2e-6, 2e-5, 2e-5, 2e-5, 1e-7
MARGIN = 4.0

# ------------------------------------------------------------------------------------------------ case lists
KINDS = ("noise", "smooth")
SSIM_W11 = ((1, 1), (1, 65), (65, 1), (5, 6), (11, 33), (32, 32), (33, 31), (37, 43), (64, 65))          # (H, W); tile 32, radius 5


def window_shapes(ws):
    sr = ws // 2
    return ((sr, sr + 1), (32, 33), (33, 32 - sr), (32 + sr, 33 + sr))


SSIM_OTHER = tuple((ws, H, W) for ws in (3, 7, 15) for (H, W) in window_shapes(ws))
SSIM_PER_IMAGE = ((33, 31), (1, 65))          # B = 3 images of 3 planes
PER_IMAGE_WEIGHTS = (0.7, -1.3, 2.1)          # non-uniform: a plane landing in the wrong image shows
POST_NO_NORMAL = ((1, 1), (2, 5), (5, 2))     # (W, H): no pixel has a normal
POST_SHAPES = POST_NO_NORMAL + ((3, 3), (16, 16), (17, 15), (18, 33), (31, 34), (33, 17), (77, 53))
POST_RATIOS = (0.0, 0.3, 1.0)
POST_CASES = tuple((W, H, False) for (W, H) in POST_SHAPES) + ((17, 15, True), (33, 17, True))
POST_LAMBDAS = (0.05, 10.0)                   # lambda_normal, lambda_dist
FUSED_SHAPES = ((1, 1), (3, 3), (16, 32), (17, 33), (33, 17), (37, 43))       # (H, W): 3, 6 or 12 SSIM workgroups, 1 .. 9 post workgroups
FUSED_ARGS = (0.7, 0.2, 0.05, 100.0, 1.5)     # depth_ratio, lambda_dssim, lambda_normal, lambda_dist, upstream gradient


def shape_seed(H, W, salt=0):
    return 1000003 * salt + 1000 * H + W


# ------------------------------------------------------------------------------------------------ builders
def photo_case(H, W, kind, seed):
    """img, gt [3,H,W] float32 in [0,1]; img == gt exactly at the four corners and at (31,31), (32,32): the sign(0) = 0 branch of
    L1 at the image corners and at the tile seam."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        gt = rng.uniform(0, 1, size=(3, H, W))
        img = np.clip(gt + 0.1 * rng.normal(size=gt.shape), 0, 1)
    elif kind == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        gt = np.stack([0.5 + 0.4 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)])
        img = np.clip(gt + 0.02 * rng.normal(size=gt.shape), 0, 1)
    else:
        raise ValueError(kind)
    img = img.astype(np.float32); gt = gt.astype(np.float32)
    if H <= 2 and W <= 2:
        # every pixel is a corner: with img == gt everywhere SSIM sits at its maximum, the reference gradient is identically zero
        # and a tolerance relative to mean|ref| is zero too — the fp32 oracle itself returns 3e-8 there.  No ties in such a frame.
        return img, gt
    for (y, x) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (31, 31), (32, 32)):
        if y < H and x < W:
            img[:, y, x] = gt[:, y, x]
    return img, gt


def hole_pixels(H, W):
    """(y, x) of the pixels nothing covered in a holes=True case: the corners, the 16-tile seam and one interior pixel."""
    want = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (15, 15), (16, 16), (H // 2, W // 2 - 2))
    return sorted({(y, x) for (y, x) in want if 0 <= y < H and 0 <= x < W})


def post_case(H, W, seed, holes=False):
    """allmap [7,H,W], wmaps [9,H,W] (float32) and the camera (wvt, fpt: float64 matrices as the Camera stores them), built as
    tests/test_gpu_train.py::test_render_post_vs_oracle_odd_size builds them.  The camera is made for a frame of at least 8 x 8 and its
    matrices are kept for smaller ones."""
    import synthetic
    sc = synthetic.make_scene(8, max(W, 8), max(H, 8), seed=1, view_index=3)
    wvt = np.asarray(sc["viewmatrix"], np.float64); fpt = np.asarray(sc["projmatrix"], np.float64)
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    alpha = np.clip(0.7 + 0.3 * np.sin(xx / 9.0) * np.cos(yy / 6.0), 0.05, 0.99).astype(np.float32)
    depth = (4.0 + np.sin(xx / 5.0) + 0.7 * np.cos(yy / 4.0)).astype(np.float32)
    am = np.zeros((7, H, W), np.float32)
    am[0] = depth * alpha; am[1] = alpha
    n = rng.normal(size=(3, H, W)); am[2:5] = (n / np.linalg.norm(n, axis=0)) * alpha
    am[5] = depth * 1.01; am[6] = 0.01 * np.abs(rng.normal(size=(H, W)))
    wm = rng.normal(size=(9, H, W)).astype(np.float32)
    if holes:
        for (y, x) in hole_pixels(H, W):
            am[0, y, x] = am[1, y, x] = am[5, y, x] = 0.0
    return am, wm, dict(wvt=wvt, fpt=fpt, W=W, H=H)


# ------------------------------------------------------------------------------------------------ judge
def grad_tol(ref):
    ref = np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    return GRAD_RTOL * (float(np.abs(ref[ok]).mean()) if ok.any() else 0.0), GRAD_RTOL


def worst_ratio(got, ref, atol, rtol, where=None):
    """max over the elements (those of `where`) of |got - ref| / (atol + rtol * |ref|) and its index; an element that differs
    under a zero tolerance, or that is not finite, counts as infinitely far."""
    got = np.atleast_1d(np.asarray(got, np.float64)); ref = np.atleast_1d(np.asarray(ref, np.float64))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = np.abs(got - ref); tol = atol + rtol * np.abs(ref)
        ratio = np.where(diff == 0, 0.0, diff / tol)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    if where is not None:
        ratio = np.where(where, ratio, 0.0)
    if ratio.size == 0:
        return 0.0, ()
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


def hold_all(name, got, ref, atol, rtol, yard=None, where=None):
    """Every element of `got` within max(1, 4 * yard) tolerances of `ref`.  Prints and returns the worst ratio."""
    worst, idx = worst_ratio(got, ref, atol, rtol, where)
    bar = max(1.0, MARGIN * (yard or 0.0))
    print("EDGE %-44s worst %.4g at %s  (yard %s, bar %.3g)" % (name, worst, idx, "-" if yard is None else "%.4g" % yard, bar))
    assert worst <= bar, "%s: element %s is %.4g tolerances off (bar %.3g): got %r, ref %r" % (
        name, idx, worst, bar, np.atleast_1d(np.asarray(got))[idx], np.atleast_1d(np.asarray(ref))[idx])
    return worst


def hole_rule(g, gref, holes):
    """The 0/0 pixels of a holes=True case: NaN in the reference's autograd at exactly the placed pixels; the device's values are
    finite and its gradient of the depth channel a0 is exactly zero there.  Returns the mask of the elements that are compared."""
    g = np.asarray(g); gref = np.asarray(gref)
    ok = np.isfinite(gref)
    bad = ~ok.all(axis=0)
    assert sorted((int(y), int(x)) for y, x in zip(*np.nonzero(bad))) == list(holes), (np.nonzero(bad), holes)
    assert np.isfinite(g).all()
    assert (g[0][bad] == 0).all()
    return ok


# ------------------------------------------------------------------------------------------------ references (fp64) and yardsticks (fp32)
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def photometric_t(img, gt, dtype, ws=11, lam=0.2):
    """train.py:72-74 from the oracle's dtype-generic l1_loss / ssim: values and gradients w.r.t. img in `dtype`."""
    x = torch.tensor(np.asarray(img), dtype=dtype, requires_grad=True); y = torch.tensor(np.asarray(gt), dtype=dtype)
    l1 = O.l1_loss(x, y); s = O.ssim(x, y, ws)
    loss = (1.0 - lam) * l1 + lam * (1.0 - s)
    g_l1, = torch.autograd.grad(l1, x, retain_graph=True)
    g_ss, = torch.autograd.grad(s, x, retain_graph=True)
    g, = torch.autograd.grad(loss, x)
    return dict(l1=l1.item(), ssim=s.item(), loss=loss.item(), g_l1=g_l1.numpy(), g_ssim=g_ss.numpy(), g_loss=g.numpy())


def per_image_t(imgs, gts, dtype, ws=11):
    """ssim(size_average=False) of [B,3,H,W] (utils/loss_utils.py:70-73: one mean per image) and the gradient of its
    PER_IMAGE_WEIGHTS-weighted sum."""
    x = torch.tensor(np.asarray(imgs), dtype=dtype, requires_grad=True); y = torch.tensor(np.asarray(gts), dtype=dtype)
    vals = torch.stack([O.ssim(x[b], y[b], ws) for b in range(x.shape[0])])
    g, = torch.autograd.grad((vals * torch.tensor(PER_IMAGE_WEIGHTS, dtype=dtype)).sum(), x)
    return dict(ssim=vals.detach().numpy(), g_ssim=g.numpy())


def render_post_t(allmap, consts, W, H, ratio, dtype):
    """oracle.render_post on the 24-float camera block (O.cam_consts: computed in fp64, cast to `dtype` as the device's constants
    are) instead of the two matrices: gaussian_renderer/__init__.py:118-147 with utils/point_utils.py:9-37."""
    c = torch.tensor(np.asarray(consts), dtype=dtype)
    A, K, o = c[0:9].reshape(3, 3), c[9:18].reshape(3, 3), c[18:21]
    render_alpha = allmap[1:2]
    render_normal = (allmap[2:5].permute(1, 2, 0) @ A.T).permute(2, 0, 1)
    med = torch.nan_to_num(allmap[5:6], 0, 0)
    exp = torch.nan_to_num(allmap[0:1] / render_alpha, 0, 0)
    surf_depth = exp * (1 - ratio) + ratio * med
    gx, gy = torch.meshgrid(torch.arange(W, dtype=dtype), torch.arange(H, dtype=dtype), indexing="xy")
    pts = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).reshape(-1, 3)
    points = (surf_depth.reshape(-1, 1) * (pts @ K) + o).reshape(H, W, 3)
    sn = torch.zeros_like(points)
    if H >= 3 and W >= 3:
        dx = points[2:, 1:-1] - points[:-2, 1:-1]
        dy = points[1:-1, 2:] - points[1:-1, :-2]
        sn[1:-1, 1:-1, :] = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
    surf_normal = sn.permute(2, 0, 1) * render_alpha.detach()
    return torch.cat([render_alpha, render_normal, allmap[6:7], surf_depth, surf_normal], dim=0)


def render_post_t_np(allmap, wmaps, cam, ratio, ln, ld, dtype):
    """What oracle.render_post_np returns, from render_post_t in `dtype`."""
    W, H = cam["W"], cam["H"]
    am = torch.tensor(np.asarray(allmap), dtype=dtype, requires_grad=True)
    maps = render_post_t(am, O.cam_consts(cam["wvt"], cam["fpt"], W, H), W, H, ratio, dtype)
    normal_err = (1 - (maps[1:4] * maps[6:9]).sum(dim=0)).mean()
    dist_mean = maps[4].mean()
    g_maps, = torch.autograd.grad((maps * torch.tensor(np.asarray(wmaps), dtype=dtype)).sum(), am, retain_graph=True)
    g_reg, = torch.autograd.grad(ln * normal_err + ld * dist_mean, am)
    return dict(maps=maps.detach().numpy(), normal_err_mean=normal_err.item(), dist_mean=dist_mean.item(), g_maps=g_maps.numpy(),
                g_reg=g_reg.numpy())


@functools.lru_cache(maxsize=None)
def photo_inputs(H, W, kind):
    img, gt = photo_case(H, W, kind, shape_seed(H, W, KINDS.index(kind)))
    img.setflags(write=False); gt.setflags(write=False)
    return img, gt


@functools.lru_cache(maxsize=None)
def photo_reference(H, W, kind, ws=11, lam=0.2):
    """(fp64 reference, yard) of a photometric case; yard: the worst element ratio per quantity of the fp32 run."""
    img, gt = photo_inputs(H, W, kind)
    ref = _frozen(photometric_t(img, gt, torch.float64, ws, lam)); f32 = photometric_t(img, gt, torch.float32, ws, lam)
    yard = dict(l1=worst_ratio(f32["l1"], ref["l1"], TOL_L1, 0)[0], ssim=worst_ratio(f32["ssim"], ref["ssim"], TOL_SSIM, 0)[0],
                loss=worst_ratio(f32["loss"], ref["loss"], TOL_LOSS, 0)[0], g_l1=worst_ratio(f32["g_l1"], ref["g_l1"], *L1_GRAD_TOL)[0],
                g_ssim=worst_ratio(f32["g_ssim"], ref["g_ssim"], *grad_tol(ref["g_ssim"]))[0],
                g_loss=worst_ratio(f32["g_loss"], ref["g_loss"], *grad_tol(ref["g_loss"]))[0])
    return ref, yard


@functools.lru_cache(maxsize=None)
def per_image_inputs(H, W):
    pairs = [photo_case(H, W, "noise", shape_seed(H, W, 10 + b)) for b in range(len(PER_IMAGE_WEIGHTS))]
    imgs = np.stack([p[0] for p in pairs]); gts = np.stack([p[1] for p in pairs])
    imgs.setflags(write=False); gts.setflags(write=False)
    return imgs, gts


@functools.lru_cache(maxsize=None)
def per_image_reference(H, W, ws=11):
    imgs, gts = per_image_inputs(H, W)
    ref = _frozen(per_image_t(imgs, gts, torch.float64, ws)); f32 = per_image_t(imgs, gts, torch.float32, ws)
    yard = dict(ssim=worst_ratio(f32["ssim"], ref["ssim"], TOL_SSIM, 0)[0],
                g_ssim=worst_ratio(f32["g_ssim"], ref["g_ssim"], *grad_tol(ref["g_ssim"]))[0])
    return ref, yard


@functools.lru_cache(maxsize=None)
def post_inputs(W, H, holes):
    am, wm, cam = post_case(H, W, shape_seed(H, W, 20), holes)
    am.setflags(write=False); wm.setflags(write=False)
    return am, wm, cam


@functools.lru_cache(maxsize=None)
def post_reference(W, H, holes, ratio, ln=POST_LAMBDAS[0], ld=POST_LAMBDAS[1]):
    """(fp64 reference = oracle.render_post_np, yard) of a post-processing case at one depth_ratio."""
    am, wm, cam = post_inputs(W, H, holes)
    ref = _frozen(O.render_post_np(am, cam["wvt"], cam["fpt"], W, H, ratio, wmaps=wm, lambda_normal=ln, lambda_dist=ld))
    f32 = render_post_t_np(am, wm, cam, ratio, ln, ld, torch.float32)
    yard = dict(maps=worst_ratio(f32["maps"][:6], ref["maps"][:6], *MAP_TOL)[0],
                surf_normal=worst_ratio(f32["maps"][6:], ref["maps"][6:], *MAP_TOL)[0],
                normal_err=worst_ratio(f32["normal_err_mean"], ref["normal_err_mean"], TOL_NORMAL_ERR, 0)[0],
                dist=worst_ratio(f32["dist_mean"], ref["dist_mean"], TOL_DIST, 0)[0])
    for k in ("g_maps", "g_reg"):
        ok = np.isfinite(ref[k])
        assert np.array_equal(ok, np.isfinite(f32[k])), k           # the fp32 run has its 0/0 pixels where the fp64 run has them
        yard[k] = worst_ratio(f32[k], ref[k], *grad_tol(ref[k]), where=ok)[0]
    return ref, yard
