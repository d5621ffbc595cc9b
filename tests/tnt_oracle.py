"""numpy restatement of TNT.md rules 1-8 (the Tanks-and-Temples-style evaluation), in fp64 throughout and in the operation orders the
rules state; scipy's cKDTree finds the neighbours.  Slow and plain on purpose: it is what the HIP kernels and the Python surface of
surfel_eval_tnt are compared with, and what tests/golden/make_golden_tnt.py puts behind the reference's own run.py in place of Open3D."""
import math

import numpy as np
from scipy.spatial import cKDTree

RELATIVE_FITNESS, RELATIVE_RMSE, MAX_ITERATION = 1e-6, 20.0, 30
MAX_POINT_NUMBER = 4e6
NEAR_MARGIN = 1e-6      # |d - threshold| below which icp_evaluate counts a pair as decided by rounding (fp32 at unit scale: 2.4e-7)


# ------------------------------------------------------------------------------------------------ rule 1
def mesh_cloud(verts, tris):
    v = np.asarray(verts, np.float64)
    return np.concatenate([v, v[np.asarray(tris, np.int64)].mean(axis=1)], axis=0)


def transform(points, T):
    p, T = np.asarray(points, np.float64), np.asarray(T, np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


# ------------------------------------------------------------------------------------------------ rule 2
class CropVolume:
    def __init__(self, orthogonal_axis, axis_min, axis_max, bounding_polygon):
        self.orthogonal_axis, self.axis_min, self.axis_max = orthogonal_axis, float(axis_min), float(axis_max)
        self.bounding_polygon = np.asarray(bounding_polygon, np.float64).reshape(-1, 3)

    def uvw(self):
        return {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}[self.orthogonal_axis]


def crop_mask(points, vol):
    """The order-free crossing rule: inside iff the number of nodes below p.u is odd and no node equals p.u."""
    p = np.asarray(points, np.float64)
    u, v, w = vol.uvw()
    pu, pv, pw = p[:, u], p[:, v], p[:, w]
    below = np.zeros(len(p), np.int64)
    on = np.zeros(len(p), bool)
    poly = vol.bounding_polygon
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(len(poly)):
            a, b = poly[k], poly[(k + 1) % len(poly)]
            cross = ((a[v] < pv) & (b[v] >= pv)) | ((b[v] < pv) & (a[v] >= pv))
            node = a[u] + (pv - a[v]) / (b[v] - a[v]) * (b[u] - a[u])
            below += cross & (node < pu)
            on |= cross & (node == pu)
    return (pw >= vol.axis_min) & (pw <= vol.axis_max) & (below % 2 == 1) & ~on


def crop(points, vol):
    return np.asarray(points)[crop_mask(points, vol)]


# ------------------------------------------------------------------------------------------------ rules 3, 4
def voxel_cells(points, voxel):
    p = np.asarray(points, np.float64)
    origin = p.min(axis=0) - voxel / 2 if len(p) else np.zeros(3)
    return np.floor((p - origin) / voxel).astype(np.int64)


def voxel_down_sample(points, voxel, origin_from=None):
    """(means [M, 3], counts [M], cells [M, 3]) in ascending (z, y, x) cell order; the sum of a cell runs in input order.
    origin_from: the cloud whose minimum corner sets the origin (default: points itself)."""
    p = np.asarray(points, np.float64)
    if len(p) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    src = p if origin_from is None else np.asarray(origin_from, np.float64)
    c = np.floor((p - (src.min(axis=0) - voxel / 2)) / voxel).astype(np.int64)
    order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))      # stable: input order inside a cell
    cs = c[order]
    head = np.ones(len(p), bool)
    head[1:] = np.any(cs[1:] != cs[:-1], axis=1)
    seg = np.cumsum(head) - 1
    m = seg[-1] + 1
    sums = np.zeros((m, 3))
    for k in range(3):      # (np.add.at adds one element after the other, in index order)
        np.add.at(sums[:, k], seg, p[order, k])
    counts = np.bincount(seg, minlength=m)
    return sums / counts[:, None], counts, cs[head]


def uniform_down_sample(points, max_points=MAX_POINT_NUMBER):
    n = len(points)
    if n > max_points:
        return np.asarray(points)[::int(round(n / float(max_points)))]
    return np.asarray(points)


# ------------------------------------------------------------------------------------------------ rule 5
def nearest(queries, cloud, max_dist=math.inf, k=1):
    """(distance, index) of the nearest point; +inf and -1 where it is not below max_dist.  k = 2: the two nearest, unfiltered."""
    q = np.asarray(queries, np.float64)
    if len(cloud) == 0 or len(q) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1, np.int64)
    d, i = cKDTree(np.asarray(cloud, np.float64)).query(q, k=k)
    if k != 1:
        return d, i
    hit = d < max_dist
    return np.where(hit, d, np.inf), np.where(hit, i, -1)


def correspondence_sums(moved, index, target):
    x, idx = np.asarray(moved, np.float64), np.asarray(index)
    sel = idx >= 0
    x, y = x[sel], np.asarray(target, np.float64)[idx[sel]]
    d = x - y
    return np.concatenate([[float(len(x))], x.sum(0), y.sum(0), (y[:, :, None] * x[:, None, :]).sum(0).reshape(-1),
                           [((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).sum()],
                           [((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum()]])


def umeyama_from_sums(s):
    n = s[0]
    mx, my = s[1:4] / n, s[4:7] / n
    cov = s[7:16].reshape(3, 3) / n - np.outer(my, mx)
    var = s[16] / n - mx @ mx
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = (D * S).sum() / var
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = my - c * (R @ mx)
    return T


def umeyama(x, y):
    """Umeyama with scaling from two point lists (centred form)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = x.mean(0), y.mean(0)
    cov = (y - my).T @ (x - mx) / len(x)
    var = ((x - mx) ** 2).sum() / len(x)
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = (D * S).sum() / var
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = my - c * (R @ mx)
    return T


def icp_evaluate(source, target, T, threshold, tree=None):
    moved = transform(source, T)
    if len(moved) == 0 or len(target) == 0:
        return 0.0, 0.0, np.zeros(18), moved, np.full(len(moved), -1, np.int64)
    d, i = (tree or cKDTree(np.asarray(target, np.float64))).query(moved)
    idx = np.where(d < threshold, i, -1)
    sums = correspondence_sums(moved, idx, target)
    n = sums[0]
    icp_evaluate.near = int((np.abs(d - threshold) < NEAR_MARGIN).sum())      # pairs an fp32 distance could put on the other side
    return n / len(moved), (math.sqrt(sums[17] / n) if n else 0.0), sums, moved, idx


def icp_similarity(source, target, threshold, init=None, relative_fitness=RELATIVE_FITNESS, relative_rmse=RELATIVE_RMSE, max_iteration=MAX_ITERATION):
    """Open3D's registration_icp loop with the point-to-point estimate with scaling.  history: (fitness, rmse, pairs within NEAR_MARGIN of
    the threshold) of every evaluation."""
    T = np.eye(4) if init is None else np.asarray(init, np.float64)
    tree = cKDTree(np.asarray(target, np.float64)) if len(target) else None
    fitness, rmse, sums, _, _ = icp_evaluate(source, target, T, threshold, tree)
    history = [(fitness, rmse, getattr(icp_evaluate, "near", 0))]
    it = 0
    while it < max_iteration and sums[0] > 0:
        T = umeyama_from_sums(sums) @ T
        f0, r0 = fitness, rmse
        fitness, rmse, sums, _, _ = icp_evaluate(source, target, T, threshold, tree)
        history.append((fitness, rmse, getattr(icp_evaluate, "near", 0)))
        it += 1
        if abs(f0 - fitness) < relative_fitness and abs(r0 - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fitness, "inlier_rmse": rmse, "iterations": it, "correspondences": int(sums[0]), "history": history}


# ------------------------------------------------------------------------------------------------ rule 7
def trajectory_alignment(est_centres, gt_centres, gt_trans=None, seed=0, threshold=0.2, ransac_n=6, draws=100000):
    src, dst = np.asarray(est_centres, np.float64), np.asarray(gt_centres, np.float64)
    if gt_trans is not None:
        G = np.asarray(gt_trans, np.float64)
        dst = transform(dst, G)
    pick = np.random.default_rng(seed).integers(0, len(src), size=(int(draws), int(ransac_n)))
    best = (-1.0, math.inf, np.eye(4))
    for idx in pick:
        with np.errstate(divide="ignore", invalid="ignore"):
            T = umeyama(src[idx], dst[idx])
        if not np.all(np.isfinite(T)):
            continue
        d2 = ((src @ T[:3, :3].T + T[:3, 3] - dst) ** 2).sum(1)
        inl = np.sqrt(d2) < threshold
        if not inl.any():
            continue
        fit, rmse = inl.sum() / len(src), math.sqrt(d2[inl].sum() / inl.sum())
        if (fit, -rmse) > (best[0], -best[1]):
            best = (fit, rmse, T)
    return best[2], best[0], best[1]


# ------------------------------------------------------------------------------------------------ rule 8
def histogram(dist, edges):
    """numpy.histogram restated: bin i holds edges[i] <= d < edges[i + 1], the last bin also d == edges[-1]."""
    d, e = np.asarray(dist, np.float64), np.asarray(edges, np.float64)
    d = d[(d >= e[0]) & (d <= e[-1])]
    b = np.searchsorted(e, d, side="right") - 1
    b[d == e[-1]] = len(e) - 2
    return np.bincount(b, minlength=len(e) - 1)[:len(e) - 1]


def score(distance1, distance2, tau, plot_stretch=5):
    if not (len(distance1) and len(distance2)):
        return {"precision": 0.0, "recall": 0.0, "fscore": 0.0, "edges": np.array([0.0]), "cum_source": np.array([0.0]), "cum_target": np.array([0.0])}
    r, p = float((np.asarray(distance2) < tau).sum()) / len(distance2), float((np.asarray(distance1) < tau).sum()) / len(distance1)
    edges = np.arange(0, tau * plot_stretch, tau / 100)
    return {"precision": p, "recall": r, "fscore": 2 * r * p / (r + p) if r + p > 0 else 0.0, "edges": edges,
            "cum_source": np.cumsum(histogram(distance1, edges)).astype(float) / len(distance1),
            "cum_target": np.cumsum(histogram(distance2, edges)).astype(float) / len(distance2)}


# ------------------------------------------------------------------------------------------------ rules 6, 8: the protocol
def crop_down(points, vol, method, voxel, T, max_points=MAX_POINT_NUMBER):
    p = np.asarray(points, np.float64) if T is None else transform(points, T)
    if vol is not None:
        p = crop(p, vol)
    return voxel_down_sample(p, voxel)[0] if method == "voxel" else uniform_down_sample(p, max_points)


def evaluate_tnt(pcd, gt, vol, tau, init_transform, relative_fitness=RELATIVE_FITNESS, relative_rmse=RELATIVE_RMSE, max_iteration=MAX_ITERATION,
                 plot_stretch=5, return_clouds=False):
    T = np.asarray(init_transform, np.float64)
    stages = []
    for method, voxel, threshold in (("voxel", tau, 80 * tau), ("voxel", tau / 2.0, 20 * tau), ("uniform", None, 2 * tau)):
        s, t = crop_down(pcd, vol, method, voxel, T), crop_down(gt, vol, method, voxel, None)
        reg = icp_similarity(s, t, threshold, None, relative_fitness, relative_rmse, max_iteration)
        T = reg["transformation"] @ T
        stages.append({"source": len(s), "target": len(t), "iterations": reg["iterations"], "fitness": reg["fitness"],
                       "inlier_rmse": reg["inlier_rmse"], "history": reg["history"]})
    s, t = crop_down(pcd, vol, "voxel", tau / 2.0, T), crop_down(gt, vol, "voxel", tau / 2.0, None)
    d1, d2 = nearest(s, t)[0], nearest(t, s)[0]
    out = score(d1, d2, tau, plot_stretch)
    out.update(transformation=T, stages=stages, source=len(s), target=len(t))
    if return_clouds:
        out.update(source_cloud=s, target_cloud=t, distance1=d1, distance2=d2)
    return out


def hot(x):
    """matplotlib's "hot" as a continuous function: three linear ramps."""
    x = np.asarray(x, np.float64)
    return np.stack([np.clip(0.0416 + (1 - 0.0416) * x / 0.365079, 0, 1), np.clip((x - 0.365079) / (0.746032 - 0.365079), 0, 1),
                     np.clip((x - 0.746032) / (1 - 0.746032), 0, 1)], -1)
