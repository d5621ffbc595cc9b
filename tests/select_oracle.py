"""fp64 oracle of the label pass (SELECT.md) — TEST INFRASTRUCTURE.

The ray / plane walk of tests/contrib_oracle.py::walk restated so that it keeps, per surfel, the map of its blend weights w = alpha * T
over the frame (trace); the weights are then routed by a label image (route).  Pixels are independent, so a pixel the label image ignores
(label >= K) drops out of the sums and is neither determined nor undetermined; every other pixel walks as it does without labels, and
one trace serves every label image of a scene.  MARGINAL pairs and UNDETERMINED pixels are contrib_oracle's, by its own rule and
constants: with nothing ignored the per-label sums add up to contrib_oracle.walk's.

Per (surfel, label) the result comes twice: `lo` over the determined pixels of that label (sum of weights, pairs), `hi` with every
undetermined pixel of that label that the surfel's tile rect reaches counted in the device's favour (a weight of 0.99, one pair).
"""
import math

import numpy as np

import analytic as A
from contrib_oracle import REL, _near


def trace(sc, n_theta=200_000):
    """dict: pairs = [(surfel, in_rect, composited, w, candidate)] in depth order (bool / float64 [H, W] maps; candidate: the pair is
    geometrically live at the pixel and its alpha reaches (1/255)(1 - 1e-3), whatever lies in front), undetermined, covered [H, W]"""
    W, H = int(sc["W"]), int(sc["H"])
    Am, b = A.pixel_map(sc)
    V = np.asarray(sc["viewmatrix"], np.float64)
    Rwc, t = V[:3, :3].T, V[3, :3]
    P = sc["means3D"].shape[0]
    mod = float(sc.get("scale_modifier", 1.0))
    gx, gy = (W + 15) // 16, (H + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    Ainv = np.linalg.inv(Am)
    org = -b @ Ainv
    dirs = np.stack([xs, ys, np.ones_like(xs)], -1) @ Ainv
    dirs = dirs / dirs[..., 2:3]
    th = np.linspace(0.0, 2 * math.pi, n_theta, endpoint=False)
    circ = 3.0 * np.stack([np.cos(th), np.sin(th)], 1)
    discs = []
    for i in range(P):
        c = Rwc @ np.asarray(sc["means3D"][i], np.float64) + t
        if c[2] <= 0.2:
            continue
        Rq = Rwc @ A.quat_to_rot(sc["rotations"][i])
        su, sv = mod * float(sc["scales"][i][0]), mod * float(sc["scales"][i][1])
        tu, tv = Rq[:, 0], Rq[:, 1]
        npl = np.cross(tu, tv)
        tud = np.cross(tv, npl); tud /= tu @ tud
        tvd = np.cross(npl, tu); tvd /= tv @ tvd
        pts = c[None] + circ[:, :1] * su * tu[None] + circ[:, 1:] * sv * tv[None]
        assert (pts[:, 2] > 1e-6).all()
        pp = pts @ Am + b
        px = pp[:, 0] / pp[:, 2]; py = pp[:, 1] / pp[:, 2]
        bx, by = 0.5 * (px.max() + px.min()), 0.5 * (py.max() + py.min())
        ex, ey = 0.5 * (px.max() - px.min()), 0.5 * (py.max() - py.min())
        r = int(math.ceil(max(ex, ey, 3.0 * A.FILTER_SIGMA)))
        rect = A._tile_rect(bx, by, r, gx, gy)
        if (rect[2] - rect[0]) * (rect[3] - rect[1]) == 0:
            continue
        discs.append((np.float32(c[2]), i, c, tud, tvd, npl, su, sv, (bx, by), rect))
    discs.sort(key=lambda d: (d[0], d[1]))
    tile_x, tile_y = (xs // 16).astype(int), (ys // 16).astype(int)
    T = np.ones((H, W)); done = np.zeros((H, W), bool); und = np.zeros((H, W), bool); covered = np.zeros((H, W), bool)
    best = np.zeros((H, W)); second = np.zeros((H, W))
    pairs = []
    for _, i, c, tu, tv, npl, su, sv, (bx, by), (x0, y0, x1, y1) in discs:
        in_rect = (tile_x >= x0) & (tile_x < x1) & (tile_y >= y0) & (tile_y < y1)
        dn = dirs @ npl
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = ((c - org) @ npl) / dn
            q = org + dirs * tt[..., None] - c
            tt = tt + org[2]
            u = (q @ tu) / su; v = (q @ tv) / sv
        rho3d = u * u + v * v
        rho2d = 2.0 * ((bx - xs) ** 2 + (by - ys) ** 2)
        depth = np.where(rho3d <= rho2d, tt, c[2])
        alpha = np.minimum(A.ALPHA_MAX, float(np.ravel(sc["opacities"][i])[0]) * np.exp(-0.5 * np.minimum(rho3d, rho2d)))
        geo = in_rect & (dn != 0) & np.isfinite(rho3d)
        live = geo & ~done
        ok = live & (depth >= A.NEAR_N) & (alpha >= A.ALPHA_MIN)
        testT = T * (1 - alpha)
        und |= live & (_near(alpha, A.ALPHA_MIN) | _near(depth, A.NEAR_N))
        und |= ok & _near(testT, A.T_EPS)
        stop = ok & (testT < A.T_EPS)
        done |= stop
        comp = ok & ~stop
        w = np.where(comp, alpha * T, 0.0)
        covered |= ok
        gt = comp & (w > best)
        second = np.where(gt, best, np.maximum(second, np.where(comp, w, 0.0)))
        best = np.where(gt, w, best)
        T = np.where(comp, testT, T)
        pairs.append((i, in_rect, comp, w, geo & (alpha >= A.ALPHA_MIN * (1 - REL))))
    und |= (second > 0) & (best - second <= REL * best)      # (contrib_oracle counts a near-tie of the two heaviest weights as marginal)
    return dict(P=P, pairs=pairs, undetermined=und, covered=covered)


def route(tr, labels, K):
    """lo / hi = dicts of sum_w (float64 [P, K]) and pairs (int64 [P, K]); undetermined [H, W] (never an ignored pixel)"""
    L = np.asarray(labels)
    P = tr["P"]
    voting = L < K
    und = tr["undetermined"] & voting
    det = voting & ~und
    lo = dict(sum_w=np.zeros((P, K)), pairs=np.zeros((P, K), np.int64))
    hi = dict(sum_w=np.zeros((P, K)), pairs=np.zeros((P, K), np.int64))
    masks = [(L == k) for k in range(K)]
    for i, in_rect, comp, w, _ in tr["pairs"]:
        cd = comp & det
        ru = in_rect & und
        for k, mk in enumerate(masks):
            sel = cd & mk
            lo["sum_w"][i, k] = w[sel].sum(); lo["pairs"][i, k] = int(sel.sum())
            nu = int((ru & mk).sum())
            hi["sum_w"][i, k] = lo["sum_w"][i, k] + A.ALPHA_MAX * nu; hi["pairs"][i, k] = lo["pairs"][i, k] + nu
    return dict(lo=lo, hi=hi, undetermined=und)


def walk(sc, labels, K, n_theta=200_000):
    return route(trace(sc, n_theta), labels, K)


def check_device(weights, o):
    """weights: float64 [P, K], the device's votes / 2^24 of ONE view, against route()'s result.  The project's own bounds
    (contrib_oracle.check_device): [lo (1 - 1e-4) - n 2^-24, hi (1 + 1e-4) + n 2^-24], n = the oracle's hi pair count of (surfel, label)."""
    lo, hi = o["lo"]["sum_w"], o["hi"]["sum_w"]
    q = o["hi"]["pairs"].astype(np.float64) * 2.0 ** -24
    bad = np.argwhere((weights < lo * (1 - 1e-4) - q) | (weights > hi * (1 + 1e-4) + q))
    assert bad.size == 0, (bad[:8], [(weights[p, k], lo[p, k], hi[p, k]) for p, k in bad[:8]])
