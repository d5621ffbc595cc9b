"""Tanks-and-Temples-style mesh evaluation on MI355X — the reference's scripts/eval_tnt/run.py::run_evaluation (the cloud of the mesh,
trajectory alignment, three crop / down-sample / similarity-ICP refinements, the two nearest-neighbour passes, precision / recall /
F-score and the cumulative histograms), without Open3D, trimesh or matplotlib.

The cloud of the mesh, the transforms, the polygon-volume crop, the voxel down-sampling, the correspondence sums of the ICP loop and
the histograms are HIP kernels of libsurfel_hip.so (include/surfel_eval_tnt.h); the neighbour search is surfel_eval's.  The rules they
follow are written down in TNT.md.  Clouds stay on the device; only counts, sums, 4 x 4 transforms and histograms cross the host
boundary, and the host does the 3 x 3 / 4 x 4 algebra, file I/O and the camera-centre RANSAC.  No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_eval_tnt.py --dataset-dir DIR/Barn --traj-path TRAJ.{log,npy} --ply-path MESH.ply ...
"""
import argparse
import ctypes as C
import functools
import json
import math
import os
import sys

import numpy as np
import torch

import surfel_native as _n
import surfel_eval as _e
from surfel_mesh import MeshLimitError, TriangleMesh, read_mesh  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

DEFAULT_BUDGET = _e.DEFAULT_BUDGET
MAX_POINT_NUMBER = 4e6          # registration.py:41
PLOT_STRETCH = 5                # run.py:164
# scripts/eval_tnt/config.py: tau per scene
SCENES_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01, "Truck": 0.005}
# Open3D's ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration = 30) as the reference's positional call
# ICPConvergenceCriteria(1e-6, max_itr = 20) fills it (TNT.md rule 5)
RELATIVE_FITNESS, RELATIVE_RMSE, MAX_ITERATION = 1e-6, 20.0, 30


_dev = functools.partial(_n.device_tensor, "surfel_eval_tnt")
_points = functools.partial(_n.rows, "surfel_eval_tnt", dtype=torch.float32)


def _mat4(T):
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4))
    if not np.all(np.isfinite(T)):
        raise ValueError("surfel_eval_tnt: the transform holds non-finite entries")
    return T


# ------------------------------------------------------------------------------------------------ rule 1: the cloud of a mesh
def mesh_cloud(mesh):
    """run.py:94-108: every vertex, then the centroid of every triangle in triangle order -> [V + F, 3] float32."""
    verts = _points(mesh.vertices, "mesh.vertices")
    tris = _dev(mesh.triangles, "mesh.triangles").detach().to(torch.int32).contiguous()
    V, F = verts.shape[0], tris.shape[0]
    pts = torch.empty((V + F, 3), dtype=torch.float32, device=verts.device)
    _n.call(verts.device, "surfel_tnt_mesh_cloud", V, F, verts, tris, pts)
    return pts


def transform(points, T):
    """fp32(T . (p, 1)) per point, T a 4 x 4 held in fp64 on the host."""
    p = _points(points, "points")
    out = torch.empty_like(p)
    Tm = _mat4(T)
    _n.call(p.device, "surfel_tnt_transform", p.shape[0], p, Tm.ctypes.data_as(C.POINTER(C.c_double)), out)
    return out


# ------------------------------------------------------------------------------------------------ rule 2: the crop volume
class CropVolume:
    """Open3D's SelectionPolygonVolume: an axis ("X" | "Y" | "Z"), its bounds and a polygon [nv, 3] seen along that axis."""

    def __init__(self, orthogonal_axis, axis_min, axis_max, bounding_polygon):
        axis = str(orthogonal_axis).upper()
        if axis not in ("X", "Y", "Z"):
            raise ValueError("surfel_eval_tnt: orthogonal_axis must be X, Y or Z, got %r" % (orthogonal_axis,))
        self.orthogonal_axis, self.axis_min, self.axis_max = axis, float(axis_min), float(axis_max)
        self.bounding_polygon = np.asarray(bounding_polygon, np.float64).reshape(-1, 3)

    @property
    def axis(self):
        return "XYZ".index(self.orthogonal_axis)

    def uv(self):
        """[nv, 2] fp64: (u, v) = (Y, Z), (X, Z), (X, Y) for the axis X, Y, Z."""
        return np.ascontiguousarray(self.bounding_polygon[:, [(1, 2), (0, 2), (0, 1)][self.axis]])


def read_crop_volume(path):
    """The crop file of a Tanks-and-Temples scene (run.py:153, read_selection_polygon_volume)."""
    with open(path, encoding="utf-8") as f:
        d = json.load(f)
    return CropVolume(d["orthogonal_axis"], d["axis_min"], d["axis_max"], d["bounding_polygon"])


def write_crop_volume(path, volume):
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"class_name": "SelectionPolygonVolume", "orthogonal_axis": volume.orthogonal_axis, "axis_min": volume.axis_min,
                   "axis_max": volume.axis_max, "bounding_polygon": volume.bounding_polygon.tolist(), "version_major": 1, "version_minor": 0}, f, indent=1)


def crop(points, volume, return_mask=False):
    """The points inside the volume, in input order (or their mask [N], bool)."""
    p = _points(points, "points")
    uv = torch.from_numpy(volume.uv()).to(p.device)
    mask = torch.zeros(p.shape[0], dtype=torch.uint8, device=p.device)
    _n.call(p.device, "surfel_tnt_crop", p.shape[0], p, volume.axis, volume.axis_min, volume.axis_max, uv.shape[0], uv, mask)
    mask = mask.bool()
    return mask if return_mask else p[mask]


# ------------------------------------------------------------------------------------------------ rules 3, 4: down-sampling
def voxel_down_sample(points, voxel, return_counts=False, return_cells=False, budget_bytes=DEFAULT_BUDGET):
    """One point per occupied voxel, the mean of its points, in ascending (z, y, x) cell order -> [M, 3] float32.  return_counts: also
    the points per cell [M] (int64); return_cells: also the cell indices [M, 3] (int32)."""
    p = _points(points, "points")
    dev, n = p.device, p.shape[0]
    voxel = float(voxel)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError("surfel_eval_tnt: bad voxel size %r" % (voxel,))
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev) if return_counts else None
    cells = torch.empty((n, 3), dtype=torch.int32, device=dev) if return_cells else None
    lo = torch.amin(p, dim=0).cpu().numpy().astype(np.float64) if n else np.zeros(3)
    origin = np.ascontiguousarray(lo - voxel / 2)
    alloc = _n.TorchAllocator(dev)
    m = _n.call(dev, "surfel_tnt_voxel_down_sample", alloc.cb, None, n, p, voxel, origin.ctypes.data_as(C.POINTER(C.c_double)), int(budget_bytes),
                out, counts, cells)
    res = (out[:m].clone(),)
    if return_counts:
        res += (counts[:m].to(torch.int64),)
    if return_cells:
        res += (cells[:m].clone(),)
    return res[0] if len(res) == 1 else res


def uniform_down_sample(points, max_points=MAX_POINT_NUMBER):
    """registration.py:124-128: above max_points keep every k-th point from 0, k = int(round(n / max_points))."""
    p = _points(points, "points")
    n = p.shape[0]
    if n > max_points:
        return p[::int(round(n / float(max_points)))].contiguous()
    return p


# ------------------------------------------------------------------------------------------------ rule 5: similarity ICP
def umeyama_from_sums(s):
    """The similarity (4 x 4, fp64) that maps x onto y in the least-squares sense (Umeyama 1991, with scaling), from the count and the sums
    of x, y, y x^T and |x|^2 (the first 17 numbers of surfel_tnt_corr_sums)."""
    s = np.asarray(s, np.float64)
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


def correspondence_sums(moved, index, target):
    """The 18 fp64 sums of surfel_tnt_corr_sums over the pairs (moved[i], target[index[i]]) with index[i] >= 0, on the host."""
    x, y = _points(moved, "moved"), _points(target, "target")
    idx = _dev(index, "index").detach().to(torch.int32).contiguous()
    out = torch.empty(18, dtype=torch.float64, device=x.device)
    alloc = _n.TorchAllocator(x.device)
    _n.call(x.device, "surfel_tnt_corr_sums", alloc.cb, None, x.shape[0], x, idx, y.shape[0], y, out)
    return out.cpu().numpy()


class _IcpTarget:
    def __init__(self, target, budget_bytes):
        self.points = target
        self.grid = _e.Grid(target, _e._nearest_cell(target), None, budget_bytes)


def icp_evaluate(source, target, T, threshold, return_index=False, budget_bytes=DEFAULT_BUDGET):
    """One evaluation of registration_icp: the source moved by T (fp32), paired with its nearest target point where the distance is below
    threshold.  Returns (fitness, inlier_rmse, sums[18]) and, with return_index, the moved source and the index [N] (int32, -1: none)."""
    src = _points(source, "source")
    tgt = target if isinstance(target, _IcpTarget) else _IcpTarget(_points(target, "target"), budget_bytes)
    moved = transform(src, T)
    if src.shape[0] == 0 or tgt.points.shape[0] == 0:
        sums = np.zeros(18)
        index = torch.full((src.shape[0],), -1, dtype=torch.int32, device=src.device)
    else:
        _, index = _e._nearest(moved, tgt.grid, threshold, True)
        sums = correspondence_sums(moved, index, tgt.points)
    n = sums[0]
    fitness = n / src.shape[0] if src.shape[0] else 0.0
    rmse = math.sqrt(sums[17] / n) if n else 0.0
    return (fitness, rmse, sums, moved, index) if return_index else (fitness, rmse, sums)


def icp_similarity(source, target, threshold, init=None, relative_fitness=RELATIVE_FITNESS, relative_rmse=RELATIVE_RMSE, max_iteration=MAX_ITERATION,
                   budget_bytes=DEFAULT_BUDGET):
    """Open3D's registration_icp with TransformationEstimationPointToPoint(with_scaling=True).  The source stays as given; iteration i
    queries fp32(T_i . p) with T_i in fp64 on the host.  Returns transformation (4 x 4), fitness, inlier_rmse, iterations (updates
    made), correspondences."""
    src, tgt = _points(source, "source"), _points(target, "target")
    if src.device != tgt.device:
        raise RuntimeError("surfel_eval_tnt: source and target live on different devices")
    T = np.eye(4) if init is None else _mat4(init)
    tg = _IcpTarget(tgt, budget_bytes)
    fitness, rmse, sums = icp_evaluate(src, tg, T, threshold)
    it = 0
    while it < int(max_iteration) and sums[0] > 0:
        T = umeyama_from_sums(sums) @ T
        f0, r0 = fitness, rmse
        fitness, rmse, sums = icp_evaluate(src, tg, T, threshold)
        it += 1
        if abs(f0 - fitness) < relative_fitness and abs(r0 - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fitness, "inlier_rmse": rmse, "iterations": it, "correspondences": int(sums[0])}


# ------------------------------------------------------------------------------------------------ rule 7: trajectory alignment (host)
def umeyama(x, y):
    """Batched Umeyama with scaling on the host: x, y [..., K, 3] -> [..., 4, 4] mapping x onto y."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = x.mean(-2, keepdims=True), y.mean(-2, keepdims=True)
    xc, yc = x - mx, y - my
    cov = np.swapaxes(yc, -1, -2) @ xc / x.shape[-2]
    var = (xc * xc).sum((-1, -2)) / x.shape[-2]
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(D.shape)
    S[..., 2] = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
    R = (U * S[..., None, :]) @ Vt
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (D * S).sum(-1) / var
    T = np.zeros(x.shape[:-2] + (4, 4))
    T[..., :3, :3] = c[..., None, None] * R
    T[..., :3, 3] = my[..., 0, :] - c[..., None] * (R @ mx[..., 0, :, None])[..., 0]
    T[..., 3, 3] = 1.0
    return T


def trajectory_alignment(est_centres, gt_centres, gt_trans=None, seed=0, threshold=0.2, ransac_n=6, draws=100000, batch=8192):
    """registration.py:65-108: RANSAC over the i <-> i correspondences of the estimated and the COLMAP camera centres (the latter moved by
    gt_trans).  Draws of ransac_n indices from numpy.random.default_rng(seed); each is fitted by Umeyama with scaling and scored on every
    camera; the best is the draw of highest fitness, then lowest inlier rmse, then earliest.  Returns (4 x 4, fitness, inlier_rmse)."""
    src, dst = np.asarray(est_centres, np.float64).reshape(-1, 3), np.asarray(gt_centres, np.float64).reshape(-1, 3)
    if gt_trans is not None:
        G = _mat4(gt_trans)
        dst = dst @ G[:3, :3].T + G[:3, 3]
    if len(src) != len(dst) or len(src) < ransac_n:
        raise ValueError("surfel_eval_tnt: the two trajectories need the same number of cameras, at least %d (got %d, %d)" % (ransac_n, len(src), len(dst)))
    pick = np.random.default_rng(seed).integers(0, len(src), size=(int(draws), int(ransac_n)))
    best = (-1.0, math.inf, np.eye(4))
    for b in range(0, len(pick), batch):
        idx = pick[b:b + batch]
        T = umeyama(src[idx], dst[idx])
        moved = src[None] @ np.swapaxes(T[:, :3, :3], 1, 2) + T[:, None, :3, 3]
        d2 = ((moved - dst[None]) ** 2).sum(-1)
        inl = np.sqrt(d2) < threshold
        cnt = inl.sum(1)
        fit = cnt / len(src)
        with np.errstate(divide="ignore", invalid="ignore"):
            rmse = np.where(cnt > 0, np.sqrt(np.where(inl, d2, 0.0).sum(1) / np.maximum(cnt, 1)), math.inf)
        ok = np.all(np.isfinite(T), axis=(1, 2))
        fit, rmse = np.where(ok, fit, -1.0), np.where(ok, rmse, math.inf)
        k = np.lexsort((np.arange(len(idx)), rmse, -fit))[0]
        if (fit[k], -rmse[k]) > (best[0], -best[1]):
            best = (float(fit[k]), float(rmse[k]), T[k])
    return best[2], best[0], best[1]


def read_trajectory_log(path):
    """trajectory_io.py:23-35: blocks of a metadata line and four matrix rows -> (poses [N, 4, 4], metadata rows)."""
    poses, meta = [], []
    with open(path) as f:
        lines = [ln for ln in f.read().split("\n")]
    k = 0
    while k < len(lines) and lines[k].strip():
        meta.append([int(x) for x in lines[k].split()])
        poses.append([[float(x) for x in lines[k + 1 + r].split()] for r in range(4)])
        k += 5
    return np.asarray(poses, np.float64).reshape(-1, 4, 4), meta


def write_trajectory_log(path, poses, meta=None):
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    with open(path, "w") as f:
        for i, p in enumerate(poses):
            f.write(" ".join(str(x) for x in (meta[i] if meta is not None else (i, i, 0))) + "\n")
            f.write("\n".join(" ".join("{0:.12f}".format(x) for x in row) for row in p.tolist()) + "\n")


def read_trajectory(path):
    """Camera-to-world poses [N, 4, 4] from a .log trajectory or a .npy pose stack (run.py:117-142)."""
    if path.endswith(".npy"):
        return np.asarray(np.load(path), np.float64).reshape(-1, 4, 4)
    if path.endswith(".json"):
        raise ValueError("surfel_eval_tnt: .json trajectories are not supported (the reference's branch needs torch and a helper it does not import)")
    return read_trajectory_log(path)[0]


def read_alignment(path):
    return _mat4(np.loadtxt(path))


# ------------------------------------------------------------------------------------------------ rule 8: scoring
def histogram(dist, edges, bound):
    """(numpy.histogram(dist, edges)[0] as int64 [len(edges) - 1], number of dist < bound) counted on the device."""
    d = _dev(dist, "dist").detach().to(torch.float32).contiguous().reshape(-1)
    e = torch.from_numpy(np.ascontiguousarray(edges, np.float64)).to(d.device)
    hist = torch.empty(e.shape[0], dtype=torch.int32, device=d.device)
    _n.call(d.device, "surfel_tnt_histogram", d.shape[0], d, e.shape[0], e, float(bound), hist)
    h = hist.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return h[:-1], int(h[-1])


def score(distance1, distance2, tau, plot_stretch=PLOT_STRETCH):
    """evaluation.py:173-215 (get_f1_score_histo2): precision, recall, fscore, the edges and the two cumulative curves."""
    n1, n2 = int(distance1.numel()), int(distance2.numel())
    if not (n1 and n2):
        return {"precision": 0.0, "recall": 0.0, "fscore": 0.0, "edges": np.array([0.0]), "cum_source": np.array([0.0]), "cum_target": np.array([0.0])}
    edges = np.arange(0, tau * plot_stretch, tau / 100)
    h1, b1 = histogram(distance1, edges, tau)
    h2, b2 = histogram(distance2, edges, tau)
    p, r = b1 / n1, b2 / n2
    return {"precision": p, "recall": r, "fscore": 2 * r * p / (r + p) if r + p > 0 else 0.0, "edges": edges,
            "cum_source": np.cumsum(h1).astype(float) / n1, "cum_target": np.cumsum(h2).astype(float) / n2}


# ------------------------------------------------------------------------------------------------ rules 6, 8: the protocol
def _crop_down(points, volume, method, voxel, T, max_points, budget_bytes):
    """registration.py:111-129 (crop_and_downsample)"""
    p = points if T is None else transform(points, T)
    if volume is not None:
        p = crop(p, volume)
    if method == "voxel":
        return voxel_down_sample(p, voxel, budget_bytes=budget_bytes)
    return uniform_down_sample(p, max_points)


def evaluate_tnt(data, gt, volume, tau, *, init_transform=None, est_traj=None, gt_traj=None, gt_trans=None, seed=0,
                 relative_fitness=RELATIVE_FITNESS, relative_rmse=RELATIVE_RMSE, max_iteration=MAX_ITERATION, plot_stretch=PLOT_STRETCH,
                 max_points=MAX_POINT_NUMBER, return_clouds=False, timings=None, budget_bytes=DEFAULT_BUDGET):
    """run.py::run_evaluation as a function.  data: a mesh (.vertices, .triangles) or a cloud [N, 3]; gt: the ground-truth cloud [M, 3];
    volume: a CropVolume (None: no crop); tau: the scene's distance threshold.  The initial transform is init_transform (4 x 4), or comes
    from trajectory_alignment(est_traj, gt_traj, gt_trans, seed) over camera-to-world poses [N, 4, 4].  Returns precision, recall, fscore,
    tau, the edges and the two cumulative curves, the final transformation and per stage the cloud sizes, iterations, fitness and rmse;
    return_clouds adds the two scored clouds and their distances.  timings: a dict that receives ms per part (cloud, trajectory: the host's
    RANSAC, register_0 .. register_2: crop, down-sampling and ICP of a refinement, score; synchronises between parts)."""
    gt = _points(gt, "gt")
    laps = _e._Laps(timings, gt.device)
    pcd = mesh_cloud(data) if hasattr(data, "triangles") else _points(data, "data")
    laps.lap("cloud")
    if pcd.device != gt.device:
        raise RuntimeError("surfel_eval_tnt: data and gt live on different devices")
    tau = float(tau)
    out = {"tau": tau, "points": pcd.shape[0], "gt_points": gt.shape[0]}
    if init_transform is not None:
        T = _mat4(init_transform)
    elif est_traj is not None and gt_traj is not None:
        T, fit, rmse = trajectory_alignment(np.asarray(est_traj)[:, :3, 3], np.asarray(gt_traj)[:, :3, 3], gt_trans, seed)
        out["trajectory"] = {"fitness": fit, "inlier_rmse": rmse, "transformation": T.tolist()}
    else:
        raise ValueError("surfel_eval_tnt: give init_transform, or est_traj and gt_traj")
    laps.lap("trajectory")
    crit = dict(relative_fitness=relative_fitness, relative_rmse=relative_rmse, max_iteration=max_iteration, budget_bytes=budget_bytes)
    stages = []
    for method, voxel, threshold in (("voxel", tau, 80 * tau), ("voxel", tau / 2.0, 20 * tau), ("uniform", None, 2 * tau)):      # run.py:156-160
        s = _crop_down(pcd, volume, method, voxel, T, max_points, budget_bytes)
        t = _crop_down(gt, volume, method, voxel, None, max_points, budget_bytes)
        reg = icp_similarity(s, t, threshold, None, **crit)
        T = reg["transformation"] @ T
        stages.append({"method": method, "voxel_size": voxel, "threshold": threshold, "source": s.shape[0], "target": t.shape[0],
                       "iterations": reg["iterations"], "fitness": reg["fitness"], "inlier_rmse": reg["inlier_rmse"]})
        del s, t
        laps.lap("register_%d" % (len(stages) - 1))
    # evaluation.py:60-170 (EvaluateHisto)
    s = _crop_down(pcd, volume, "voxel", tau / 2.0, T, max_points, budget_bytes)
    t = _crop_down(gt, volume, "voxel", tau / 2.0, None, max_points, budget_bytes)
    cut = plot_stretch * tau
    d1 = _e._nearest(s, _e.Grid(t, _e._nearest_cell(t), None, budget_bytes), cut) if s.shape[0] else torch.zeros(0, device=gt.device)
    d2 = _e._nearest(t, _e.Grid(s, _e._nearest_cell(s), None, budget_bytes), cut) if t.shape[0] else torch.zeros(0, device=gt.device)
    out.update(score(d1, d2, tau, plot_stretch))
    laps.lap("score")
    out.update(transformation=T, stages=stages, source=s.shape[0], target=t.shape[0])
    if return_clouds:
        out.update(source_cloud=s, target_cloud=t, distance1=d1, distance2=d2)
    return out


# ------------------------------------------------------------------------------------------------ rule 9: outputs
_HOT = ((0.0416, 0.365079, 0.0), (0.0, 0.746032, 0.365079), (0.0, 1.0, 0.746032))      # per channel: value at its start, end of its ramp, start


def hot_r(x):
    """matplotlib's "hot_r" without matplotlib: its 256-entry table looked up at int(x * 256); "hot" is three linear ramps (red from
    0.0416 over [0, 0.365079], green over [0.365079, 0.746032], blue over [0.746032, 1]) and hot_r its mirror.  x in [0, 1] (tensor or
    array) -> [..., 3]."""
    xp = torch if torch.is_tensor(x) else np
    i = xp.clip(xp.floor(x * 256), 0, 255)
    xi = (255 - i) / 255.0
    ch = [xp.clip(v0 + (1.0 - v0) * (xi - a) / (b - a), v0, 1.0) for v0, b, a in _HOT]
    return xp.stack(ch, -1)


def write_outputs(result, out_dir, scene, clouds=True):
    """The reference's three text files (evaluation.py:155-160), results.json and, with clouds, the two clouds coloured by distance
    (evaluation.py:50-57: hot_r at min(d, 3 tau) / (3 tau))."""
    import surfel_io
    os.makedirs(out_dir, exist_ok=True)
    tau = result["tau"]
    np.savetxt(os.path.join(out_dir, scene + ".recall.txt"), result["cum_target"])
    np.savetxt(os.path.join(out_dir, scene + ".precision.txt"), result["cum_source"])
    np.savetxt(os.path.join(out_dir, scene + ".prf_tau_plotstr.txt"), np.array([result["precision"], result["recall"], result["fscore"], tau, PLOT_STRETCH]))
    with open(os.path.join(out_dir, "results.json"), "w") as fp:
        json.dump({"precision": result["precision"], "recall": result["recall"], "fscore": result["fscore"], "tau": tau,
                   "transformation": np.asarray(result["transformation"]).tolist(), "stages": result["stages"], "source": result["source"],
                   "target": result["target"], "trajectory": result.get("trajectory")}, fp, indent=True)
    if clouds:
        empty = torch.zeros((0, 3), dtype=torch.int32)
        for tag, pts, d in (("precision", result["source_cloud"], result["distance1"]), ("recall", result["target_cloud"], result["distance2"])):
            col = hot_r(d.clamp(max=3 * tau) / (3 * tau)) if pts.shape[0] else torch.zeros((0, 3))
            surfel_io.write_triangle_mesh(os.path.join(out_dir, "%s.%s.ply" % (scene, tag)), TriangleMesh(pts, empty, col))


def _cloud_of_ply(path, dev):
    import surfel_io
    p = surfel_io.read_ply(path)
    return torch.from_numpy(np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Tanks-and-Temples F-score of a mesh (the reference's scripts/eval_tnt/run.py)")
    ap.add_argument("--dataset-dir", type=str, required=True, help="DIR/SCENE holding SCENE.ply, SCENE.json, SCENE_COLMAP_SfM.log, SCENE_trans.txt")
    ap.add_argument("--traj-path", type=str, required=True, help="estimated trajectory (.log or .npy)")
    ap.add_argument("--ply-path", type=str, required=True, help="reconstructed mesh")
    ap.add_argument("--out-dir", type=str, default="")
    ap.add_argument("--tau", type=float, default=None, help="distance threshold (default: the scene's, from its name)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--relative_fitness", type=float, default=RELATIVE_FITNESS)
    ap.add_argument("--relative_rmse", type=float, default=RELATIVE_RMSE)
    ap.add_argument("--max_iteration", type=int, default=MAX_ITERATION)
    ap.add_argument("--no_clouds", action="store_true")
    args = ap.parse_args(argv)
    scene = os.path.basename(os.path.normpath(args.dataset_dir))
    if args.tau is None and scene not in SCENES_TAU:
        raise SystemExit("invalid dataset-dir: %s is none of %s (give --tau)" % (scene, ", ".join(SCENES_TAU)))
    tau = SCENES_TAU[scene] if args.tau is None else args.tau
    out_dir = args.out_dir.strip() or os.path.join(os.path.dirname(args.ply_path), "evaluation")
    dev = torch.device("cuda:0")
    mesh = read_mesh(args.ply_path, dev)
    base = os.path.join(args.dataset_dir, scene)
    res = evaluate_tnt(mesh, _cloud_of_ply(base + ".ply", dev), read_crop_volume(base + ".json"), tau, est_traj=read_trajectory(args.traj_path),
                       gt_traj=read_trajectory(base + "_COLMAP_SfM.log"), gt_trans=read_alignment(base + "_trans.txt"), seed=args.seed,
                       relative_fitness=args.relative_fitness, relative_rmse=args.relative_rmse, max_iteration=args.max_iteration,
                       return_clouds=not args.no_clouds)
    write_outputs(res, out_dir, scene, clouds=not args.no_clouds)
    print("precision : %.4f\nrecall : %.4f\nf-score : %.4f" % (res["precision"], res["recall"], res["fscore"]))
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
