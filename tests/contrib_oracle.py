"""fp64 oracle of the contribution pass (CONTRIB.md) — TEST INFRASTRUCTURE.

The ray / plane walk of tests/analytic.py::raycast_render restated so that it returns, per surfel, what the pass accumulates: the sum
and the maximum of the blend weights w = alpha * T, the composited pairs, the pixels the surfel dominates and whether it was seen
(composited or terminated a pixel).  It is the test suite's own formulation and shares nothing with oracle/surfel_oracle.c.

fp32 decides some pairs differently from fp64: a pair is MARGINAL where alpha lies within a relative 1e-3 of 1/255, T (1 - alpha) of 1e-4
or depth of the near plane, and a pixel is marginal where its two heaviest weights lie within 1e-3 of each other (1e-3 = ten times the
fp32 image tolerance of tests/test_gpu_analytic.py).  A pixel holding a marginal pair is UNDETERMINED (everything behind such a pair in
the pixel may differ).  Every statistic comes twice: `lo` over the determined pixels only, `hi` with every undetermined pixel the
surfel's tile rect reaches counted in the device's favour (one more pair, one more dominated pixel, a weight of 0.99).
"""
import math

import numpy as np

import analytic as A

REL = 1e-3


def _near(x, thr):
    return np.abs(x - thr) <= REL * abs(thr)


def walk(sc, n_theta=200_000):
    """sc: scene dict as analytic.raycast_render takes it.  Returns a dict: lo / hi = dicts of sum_w, max_w (float64 [P]), hits, dominant
    (int64 [P]), seen (bool [P]); full_sum_w (the sum over all pixels); dominant_id [H, W] int (-1 = none); undetermined, covered [H, W] bool."""
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
    best = np.zeros((H, W)); second = np.zeros((H, W)); best_id = np.full((H, W), -1, np.int64)
    pairs = []      # (surfel, in_rect, composited, w, ok) per disc, for the two passes over the pixels below
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
        live = in_rect & ~done & (dn != 0) & np.isfinite(rho3d)
        ok = live & (depth >= A.NEAR_N) & (alpha >= A.ALPHA_MIN)
        testT = T * (1 - alpha)
        und |= live & (_near(alpha, A.ALPHA_MIN) | _near(depth, A.NEAR_N))
        und |= ok & _near(testT, A.T_EPS)
        stop = ok & (testT < A.T_EPS)
        done |= stop
        comp = ok & ~stop
        w = np.where(comp, alpha * T, 0.0)
        covered |= ok
        gt = comp & (w > best)                       # a tie keeps the nearer surfel
        second = np.where(gt, best, np.maximum(second, np.where(comp, w, 0.0)))
        best_id = np.where(gt, i, best_id)
        best = np.where(gt, w, best)
        T = np.where(comp, testT, T)
        pairs.append((i, in_rect, comp, w, ok))
    und |= (second > 0) & (best - second <= REL * best)
    det = ~und
    z = lambda dt: np.zeros(P, dt)
    lo = dict(sum_w=z(np.float64), max_w=z(np.float64), hits=z(np.int64), dominant=z(np.int64), seen=z(bool))
    hi = dict(sum_w=z(np.float64), max_w=z(np.float64), hits=z(np.int64), dominant=z(np.int64), seen=z(bool))
    full = z(np.float64)      # every pixel counted as fp64 decides it: what another fp64 formulation computes
    for i, in_rect, comp, w, ok in pairs:
        full[i] = w.sum()
        cd = comp & det
        lo["sum_w"][i] = w[cd].sum(); lo["max_w"][i] = w[cd].max(initial=0.0); lo["hits"][i] = int(cd.sum())
        lo["dominant"][i] = int(((best_id == i) & det).sum()); lo["seen"][i] = bool((ok & det).any())
        nu = int((in_rect & und).sum())
        hi["sum_w"][i] = lo["sum_w"][i] + A.ALPHA_MAX * nu
        hi["max_w"][i] = max(lo["max_w"][i], A.ALPHA_MAX) if nu else lo["max_w"][i]
        hi["hits"][i] = lo["hits"][i] + nu; hi["dominant"][i] = lo["dominant"][i] + nu
        hi["seen"][i] = lo["seen"][i] or nu > 0
    return dict(lo=lo, hi=hi, full_sum_w=full, dominant_id=best_id, undetermined=und, covered=covered)


def check_device(stats, o, nviews=1):
    """The GPU tests' comparison: stats = dict(sum_w float64, max_w, hits, dominant, views [P] numpy, dominant_id [H, W] or None) of ONE view
    against walk()'s result o.  Bounds as the issue sets them: integers in [lo, hi]; sum_w in [lo (1 - 1e-4) - hits 2^-24, hi (1 + 1e-4)
    + hits 2^-24] (each weight is rounded to 2^-24: half a unit per pair would do, a whole one is allowed); max_w within 1e-4 relative."""
    lo, hi = o["lo"], o["hi"]
    hits = stats["hits"].astype(np.float64)
    for k in ("hits", "dominant"):
        bad = np.nonzero((stats[k] < lo[k]) | (stats[k] > hi[k]))[0]
        assert bad.size == 0, (k, bad[:8], stats[k][bad[:8]], lo[k][bad[:8]], hi[k][bad[:8]])
    q = hits * 2.0 ** -24
    bad = np.nonzero((stats["sum_w"] < lo["sum_w"] * (1 - 1e-4) - q) | (stats["sum_w"] > hi["sum_w"] * (1 + 1e-4) + q))[0]
    assert bad.size == 0, ("sum_w", bad[:8], stats["sum_w"][bad[:8]], lo["sum_w"][bad[:8]], hi["sum_w"][bad[:8]])
    mw = stats["max_w"].astype(np.float64)
    bad = np.nonzero((mw < lo["max_w"] * (1 - 1e-4)) | (mw > hi["max_w"] * (1 + 1e-4)))[0]
    assert bad.size == 0, ("max_w", bad[:8], mw[bad[:8]], lo["max_w"][bad[:8]], hi["max_w"][bad[:8]])
    seen = stats["views"] > 0
    assert np.all(stats["views"] <= nviews) and not np.any(lo["seen"] & ~seen) and not np.any(seen & ~hi["seen"])
    if stats.get("dominant_id") is not None:
        det = ~o["undetermined"]
        assert np.array_equal(stats["dominant_id"][det], o["dominant_id"][det])
