"""DTU-style mesh evaluation on MI355X — the reference's scripts/eval_dtu/eval.py (sampling, thinning, observation mask, the two
nearest-neighbour passes, chamfer means), the mask culling of scripts/eval_dtu/evaluate_single_scene.py and the F-score of
scripts/eval_tnt/evaluation.py:173-190, without Open3D, scikit-learn, scikit-image, trimesh or OpenCV.

The sampling, the thinning rounds, the neighbour walk, the means, the dilation and the vertex test are HIP kernels of
libsurfel_hip.so (include/surfel_eval.h); the rules they follow are written down in EVAL.md.  Clouds stay on the device; only counts,
the shuffle order and the final sums cross the host boundary.  No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_eval.py --data MESH.ply --scan N --dataset_dir DIR [--mode mesh|pcd] ...
"""
import argparse
import ctypes as C
import functools
import json
import math
import os
import sys
import time

import numpy as np
import torch

import surfel_native as _n
from surfel_mesh import MeshLimitError, TriangleMesh, read_mesh  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

DEFAULT_BUDGET = 16 << 30
MAX_CELLS = 1 << 27          # cells of one grid (8 B each), and at most 64 per point (2^20 for small clouds)
THIN_CELL = 1.0 + 1.0 / 512  # cell edge of the thinning grid in units of density (the library asks for 1 + 2^-10)


_dev = functools.partial(_n.device_tensor, "surfel_eval")
_points = functools.partial(_n.rows, "surfel_eval", dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ rule 1: sampling
def sample_mesh(mesh, density, budget_bytes=DEFAULT_BUDGET, return_counts=False):
    """Points of a mesh as eval.py:48-71: every vertex, then the lattice samples of every triangle in triangle order -> [N, 3] float32.
    return_counts: also the samples per triangle [F] (int64).  MeshLimitError when the cloud would exceed budget_bytes."""
    verts = _points(mesh.vertices, "mesh.vertices")
    tris = _dev(mesh.triangles, "mesh.triangles").detach().to(torch.int32).contiguous()
    dev = verts.device
    V, F = verts.shape[0], tris.shape[0]
    alloc = _n.TorchAllocator(dev)
    offsets = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    total = _n.call(dev, "surfel_eval_sample_count", alloc.cb, None, V, F, verts, tris, float(density), int(budget_bytes), offsets)
    pts = torch.empty((V + total, 3), dtype=torch.float32, device=dev)
    _n.call(dev, "surfel_eval_sample_emit", V, F, verts, tris, float(density), offsets, total, pts)
    if not return_counts:
        return pts
    off = offsets[:F].to(torch.int64)
    return pts, torch.diff(off, append=torch.tensor([total], dtype=torch.int64, device=dev))


# ------------------------------------------------------------------------------------------------ the grid
class Grid:
    """surfel_eval_grid over a cloud: origin = the cloud's minimum corner, `cell` grown from `min_cell` until the dense cell table
    holds at most MAX_CELLS cells (a larger cell costs time, never exactness)."""

    def __init__(self, points, min_cell, rank=None, budget_bytes=DEFAULT_BUDGET):
        self.points, self.device, self.lib = points, points.device, _n.load()
        n = points.shape[0]
        if n:
            lo, hi = (x.cpu().numpy().astype(np.float64) for x in torch.aminmax(points, dim=0))
            if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
                raise ValueError("surfel_eval: the cloud holds non-finite coordinates")
        else:
            lo = hi = np.zeros(3)
        cell = float(np.float32(min_cell))
        if not (cell > 0 and math.isfinite(cell)):
            raise ValueError("surfel_eval: bad cell size %r" % (min_cell,))
        while True:
            dims = np.floor((hi - lo) / cell).astype(np.int64) + 1
            if int(np.prod(dims)) <= min(MAX_CELLS, max(64 * n, 1 << 20)):
                break
            cell = float(np.float32(cell * 1.1))
        self.alloc = _n.TorchAllocator(self.device)
        self.g = _n.EvalGrid()
        self.g.origin[:] = [float(np.float32(x)) for x in lo]
        self.g.cell = cell
        self.g.dims[:] = [int(x) for x in dims]
        self.g.budget_bytes = int(budget_bytes)
        _n.call(self.device, "surfel_eval_grid_build", self.alloc.cb, None, self.g, n, points, rank)


def shuffle_rank(n, seed, device):
    """rank[i] = place of point i in the thinning order: the order is numpy.random.default_rng(seed).permutation(n) (seed None: the
    input order), made on the host."""
    if seed is None:
        return None
    rank = np.empty(n, np.int64)
    rank[np.random.default_rng(seed).permutation(n)] = np.arange(n)
    return torch.from_numpy(rank.astype(np.int32)).to(device)


# ------------------------------------------------------------------------------------------------ rule 3: thinning
def thin(points, density, seed=0, return_rounds=False, budget_bytes=DEFAULT_BUDGET):
    """eval.py:81-94: in the shuffled order a point is kept iff no kept point earlier in the order lies within `density` (<=).
    Returns the kept mask [N] (bool, input order)."""
    pts = _points(points, "points")
    keep, rounds = _thin(_thin_grid(pts, density, seed, budget_bytes), density)
    return (keep, rounds) if return_rounds else keep


def _thin_grid(pts, density, seed, budget_bytes, rank=False):
    d32 = np.float32(density)
    rank = shuffle_rank(pts.shape[0], seed, pts.device) if rank is False else rank
    return Grid(pts, np.float32(d32 * np.float32(THIN_CELL)), rank, budget_bytes)


def _thin(grid, density):
    dev, n = grid.device, grid.points.shape[0]
    keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    rounds = C.c_int(0)
    _n.call(dev, "surfel_eval_thin", grid.alloc.cb, None, grid.g, float(np.float32(density)), keep, rounds)
    return keep.bool(), rounds.value


# ------------------------------------------------------------------------------------------------ rule 5: nearest neighbour
def _nearest_cell(cloud):
    """About one surface point per occupied cell: a cloud of n points spread over a surface as wide as the cloud's largest extent
    has a spacing near 1.8 extent / sqrt(n)."""
    n = cloud.shape[0]
    if n == 0:
        return 1.0
    lo, hi = torch.aminmax(cloud, dim=0)
    ext = float((hi - lo).max())
    return max(2.0 * ext / math.sqrt(n), 1e-30) if ext > 0 and math.isfinite(ext) else 1.0


def nearest(queries, cloud, max_dist=math.inf, return_index=False, budget_bytes=DEFAULT_BUDGET):
    """Distance [Q] (float32) from every query to its nearest point of `cloud`; +inf where it is not below max_dist (eval.py:118-134
    only uses the distances below max_dist).  return_index: also the point's index (int32, -1 for none).  Exact, not approximate."""
    q, c = _points(queries, "queries"), _points(cloud, "cloud")
    if q.device != c.device:
        raise RuntimeError("surfel_eval: queries and cloud live on different devices")
    return _nearest(q, Grid(c, _nearest_cell(c), None, budget_bytes), max_dist, return_index)


def _nearest(q, grid, max_dist, return_index=False):
    dev = q.device
    dist = torch.empty(q.shape[0], dtype=torch.float32, device=dev)
    idx = torch.empty(q.shape[0], dtype=torch.int32, device=dev) if return_index else None
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_eval_nearest", alloc.cb, None, grid.g, q.shape[0], q, float(max_dist), dist, idx)
    return (dist, idx) if return_index else dist


def sum_count_below(dist, bound):
    """(sum, count) in fp64 of the distances below `bound`, accumulated on the device in a fixed order."""
    d = _dev(dist, "dist").detach().to(torch.float32).contiguous().reshape(-1)
    dev = d.device
    out = torch.empty(2, dtype=torch.float64, device=dev)
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_eval_mean_below", alloc.cb, None, d.shape[0], d, float(bound), out)
    s, c = out.cpu().tolist()
    return s, int(c)


def mean_below(dist, bound):
    """dist[dist < bound].mean(); nan when nothing is below (numpy's mean of an empty array)."""
    s, c = sum_count_below(dist, bound)
    return s / c if c else float("nan")


def fscore(d2s, s2d, tau):
    """scripts/eval_tnt/evaluation.py:173-190: precision = mean(d2s < tau), recall = mean(s2d < tau) over all queries (a "none" counts as
    >= tau), fscore = 2 p r / (p + r), 0 when both are 0."""
    p = sum_count_below(d2s, tau)[1] / max(int(d2s.numel()), 1)
    r = sum_count_below(s2d, tau)[1] / max(int(s2d.numel()), 1)
    return {"precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0}


# ------------------------------------------------------------------------------------------------ rules 2-5: the DTU protocol
class _Laps:
    def __init__(self, out, dev):
        self.out, self.dev = out, dev
        self.lap(None)

    def lap(self, name):
        if self.out is None:
            return
        torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        if name is not None:
            self.out[name] = self.out.get(name, 0.0) + (now - self.t) * 1e3
        self.t = now


def evaluate_dtu(data, stl, obs_mask, bb, res, plane, *, mode="mesh", density=0.2, patch=60, max_dist=20, seed=0, return_distances=False,
                 timings=None, budget_bytes=DEFAULT_BUDGET):
    """eval.py as a function.  data: a mesh (mode "mesh": .vertices, .triangles) or a cloud [N, 3] (mode "pcd"); stl: the ground-truth
    cloud [M, 3]; obs_mask: uint8 [X, Y, Z]; bb: [2, 3]; res: the mask's voxel size; plane: 4 coefficients.  Everything on the device
    except bb, res, plane.  Returns mean_d2s, mean_s2d, overall and the point count of every stage (the reference's variable names);
    return_distances adds the clouds, masks and per-point distances that error_clouds() draws.  timings: a dict that receives ms per
    stage (sample, shuffle: the host's permutation and its copy, grid: the three grid builds, thin, mask, d2s, s2d; synchronises
    between stages)."""
    if mode not in ("mesh", "pcd"):
        raise ValueError("surfel_eval: mode must be 'mesh' or 'pcd', got %r" % (mode,))
    stl = _points(stl, "stl")
    dev = stl.device
    obs_mask = _dev(obs_mask, "obs_mask")
    if obs_mask.ndim != 3:
        raise ValueError("surfel_eval: obs_mask must be [X, Y, Z]")
    obs_mask = (obs_mask != 0).to(torch.uint8).contiguous() if obs_mask.dtype != torch.uint8 else obs_mask.contiguous()
    laps = _Laps(timings, dev)
    data_pcd = sample_mesh(data, density, budget_bytes) if mode == "mesh" else _points(data, "data")
    laps.lap("sample")
    rank = shuffle_rank(data_pcd.shape[0], seed, dev)
    laps.lap("shuffle")
    grid = _thin_grid(data_pcd, density, seed, budget_bytes, rank)
    laps.lap("grid")
    keep, rounds = _thin(grid, density)
    del grid
    laps.lap("thin")
    data_down = data_pcd[keep]
    n = data_down.shape[0]
    inbound = torch.zeros(n, dtype=torch.uint8, device=dev)
    in_obs = torch.zeros(n, dtype=torch.uint8, device=dev)
    bbf = (C.c_float * 6)(*[float(x) for x in np.asarray(bb, np.float32).reshape(-1)[:6]])
    dims = (C.c_int * 3)(*obs_mask.shape)
    _n.call(dev, "surfel_eval_obs_mask", n, data_down, bbf, float(patch), float(np.asarray(res, np.float64).reshape(-1)[0]), obs_mask, dims, inbound, in_obs)
    inbound, in_obs = inbound.bool(), in_obs.bool()
    data_in, data_in_obs = data_down[inbound], data_down[in_obs]
    above = torch.zeros(stl.shape[0], dtype=torch.uint8, device=dev)
    pl = (C.c_double * 4)(*[float(x) for x in np.asarray(plane, np.float64).reshape(-1)[:4]])
    _n.call(dev, "surfel_eval_above_plane", stl.shape[0], stl, pl, above)
    above = above.bool()
    stl_above = stl[above]
    laps.lap("mask")
    grid = Grid(stl, _nearest_cell(stl), None, budget_bytes)
    laps.lap("grid")
    dist_d2s = _nearest(data_in_obs, grid, max_dist)
    laps.lap("d2s")
    grid = Grid(data_in, _nearest_cell(data_in), None, budget_bytes)
    laps.lap("grid")
    dist_s2d = _nearest(stl_above, grid, max_dist)
    del grid
    laps.lap("s2d")
    mean_d2s, mean_s2d = mean_below(dist_d2s, max_dist), mean_below(dist_s2d, max_dist)
    out = {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2, "data_pcd": data_pcd.shape[0], "data_down": n,
           "data_in": data_in.shape[0], "data_in_obs": data_in_obs.shape[0], "stl": stl.shape[0], "stl_above": stl_above.shape[0], "rounds": rounds}
    if return_distances:
        out.update(points_down=data_down, inbound=inbound, in_obs=in_obs, dist_d2s=dist_d2s, points_stl=stl, above=above, dist_s2d=dist_s2d)
    return out


def _error_colors(n, where, dist, max_dist, vis, dev):
    col = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    col[:, 2] = 1.0                                                        # blue: outside the mask / below the plane
    a = (dist.clamp(max=vis) / vis)[:, None]
    c = torch.tensor([1.0, 0.0, 0.0], device=dev) * a + (1 - a)            # white -> red
    c[dist >= max_dist] = torch.tensor([0.0, 1.0, 0.0], device=dev)        # green: no neighbour below max_dist
    col[where] = c
    return col


def error_clouds(result, out_dir, scan, max_dist=20, visualize_threshold=10):
    """The reference's two colour-coded clouds (eval.py:137-152) from evaluate_dtu(..., return_distances=True):
    vis_{scan:03}_d2s.ply and vis_{scan:03}_s2d.ply under out_dir."""
    import surfel_io
    dev = result["points_down"].device
    empty = torch.zeros((0, 3), dtype=torch.int32)
    for tag, pts, where, dist in (("d2s", result["points_down"], result["in_obs"], result["dist_d2s"]),
                                  ("s2d", result["points_stl"], result["above"], result["dist_s2d"])):
        col = _error_colors(pts.shape[0], where, dist, max_dist, visualize_threshold, dev)
        surfel_io.write_triangle_mesh(os.path.join(out_dir, "vis_%03d_%s.ply" % (scan, tag)), TriangleMesh(pts, empty, col))


# ------------------------------------------------------------------------------------------------ rule 7: mask culling
def projections(intrinsics, poses):
    """[V, 12] float32: rows 0..2 of K . inverse(pose) per view, in fp32 as the reference multiplies them."""
    K = np.asarray(intrinsics, np.float32).reshape(-1, 4, 4)
    P = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    return np.stack([(K[i] @ np.linalg.inv(P[i]).astype(np.float32))[:3].reshape(-1) for i in range(K.shape[0])]).astype(np.float32)


def dilate_masks(masks, radius=24):
    """masks uint8 [V, H, W] -> (masks != 0) dilated by the disk dx^2 + dy^2 <= radius^2, uint8 0 / 1."""
    m = _dev(masks, "masks")
    if m.ndim != 3 or m.dtype != torch.uint8:
        raise ValueError("surfel_eval: masks must be uint8 [V, H, W]")
    m = m.contiguous()
    out = torch.empty_like(m)
    alloc = _n.TorchAllocator(m.device)
    _n.call(m.device, "surfel_eval_dilate_masks", alloc.cb, None, m.shape[0], m.shape[1], m.shape[2], m, int(radius), out)
    return out


def cull_vertices(vertices, proj, dilated):
    """Kept mask [N] (bool): the vertex falls on the dilated mask, or outside the image, in every view.  proj: [V, 12] (projections())."""
    v = _points(vertices, "vertices")
    d = _dev(dilated, "dilated").contiguous()
    p = torch.as_tensor(np.asarray(proj, np.float32).reshape(-1, 12)).to(v.device).contiguous()
    if d.ndim != 3 or d.dtype != torch.uint8 or d.shape[0] != p.shape[0]:
        raise ValueError("surfel_eval: dilated must be uint8 [V, H, W] with one view per projection")
    keep = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
    _n.call(v.device, "surfel_eval_cull_vertices", v.shape[0], v, p.shape[0], p, d.shape[1], d.shape[2], d, keep)
    return keep.bool()


def compact_kept(verts, tris, keep, vertex_colors=None):
    """The tail of a vertex cull (shared with surfel_cull): the triangles whose three vertices are kept (keep: bool [V]), then the vertices
    some kept triangle uses, in their order, with their colours (zeros where the mesh has none) -> (vertices, int32 triangles, colours).
    verts [V, 3] float32, tris [F, 3] int64 with every index inside [0, V)."""
    dev = verts.device
    tkeep = keep[tris].all(dim=1)
    tris = tris[tkeep]
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=dev)
    used[tris.reshape(-1)] = True
    remap = torch.cumsum(used.to(torch.int64), 0) - 1
    cols = vertex_colors[used] if vertex_colors is not None and vertex_colors.shape[0] == verts.shape[0] else \
        torch.zeros((int(used.sum()), 3), dtype=torch.float32, device=dev)
    return verts[used], remap[tris].to(torch.int32), cols


def cull_mesh(mesh, intrinsics, poses, masks, dilate=24, scale=1.0, offset=0.0):
    """evaluate_single_scene.py:57-99: drop the vertices that some view sees outside its dilated mask, the triangles that lose a vertex
    and the vertices no kept triangle uses (order kept), then vertices * scale + offset.  intrinsics, poses (camera to world): [V, 4, 4]
    on the host; masks: uint8 [V, H, W] on the device."""
    verts = _points(mesh.vertices, "mesh.vertices")
    tris = _dev(mesh.triangles, "mesh.triangles").detach().to(torch.int64)
    dev = verts.device
    keep = cull_vertices(verts, projections(intrinsics, poses), dilate_masks(masks, dilate))
    kept, tris, cols = compact_kept(verts, tris, keep, getattr(mesh, "vertex_colors", None))
    off = torch.as_tensor(np.broadcast_to(np.asarray(offset, np.float32), (3,)).copy(), device=dev)
    return TriangleMesh(kept * float(scale) + off, tris, cols)


# ------------------------------------------------------------------------------------------------ command line
def _load_arrays(stem, names):
    """{name: array} from stem.mat (scipy.io.loadmat, when scipy is importable) or stem.npz holding the same arrays."""
    if os.path.exists(stem + ".mat"):
        try:
            from scipy.io import loadmat
        except ImportError:
            loadmat = None
        if loadmat is not None:
            m = loadmat(stem + ".mat")
            return {k: m[k] for k in names}
    if os.path.exists(stem + ".npz"):
        z = np.load(stem + ".npz")
        return {k: z[k] for k in names}
    raise FileNotFoundError("%s.mat needs scipy (scipy.io.loadmat), which is not importable here, and there is no %s.npz holding %s: convert the "
                            ".mat once where scipy is installed (numpy.savez)" % (stem, stem, ", ".join(names))
                            if os.path.exists(stem + ".mat") else "neither %s.mat nor %s.npz exists" % (stem, stem))


def main(argv=None):
    import surfel_io
    ap = argparse.ArgumentParser(description="DTU chamfer distance of a mesh or a point cloud (the reference's scripts/eval_dtu/eval.py)")
    ap.add_argument("--data", type=str, default="data_in.ply")
    ap.add_argument("--scan", type=int, default=1)
    ap.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    ap.add_argument("--dataset_dir", type=str, default=".")
    ap.add_argument("--vis_out_dir", type=str, default=".")
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--patch_size", type=float, default=60)
    ap.add_argument("--max_dist", type=float, default=20)
    ap.add_argument("--visualize_threshold", type=float, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.mode == "mesh":
        data = read_mesh(args.data, dev)
    else:
        p = surfel_io.read_ply(args.data)
        data = torch.from_numpy(np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)).to(dev)
    obs = _load_arrays(os.path.join(args.dataset_dir, "ObsMask", "ObsMask%d_10" % args.scan), ["ObsMask", "BB", "Res"])
    plane = _load_arrays(os.path.join(args.dataset_dir, "ObsMask", "Plane%d" % args.scan), ["P"])["P"]
    s = surfel_io.read_ply(os.path.join(args.dataset_dir, "Points", "stl", "stl%03d_total.ply" % args.scan))
    stl = torch.from_numpy(np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float32)).to(dev)
    mask = torch.from_numpy(np.ascontiguousarray(obs["ObsMask"] != 0).astype(np.uint8)).to(dev)
    res = evaluate_dtu(data, stl, mask, obs["BB"], obs["Res"], plane, mode=args.mode, density=args.downsample_density, patch=args.patch_size,
                       max_dist=args.max_dist, seed=args.seed, return_distances=True)
    os.makedirs(args.vis_out_dir, exist_ok=True)
    error_clouds(res, args.vis_out_dir, args.scan, args.max_dist, args.visualize_threshold)
    print(res["mean_d2s"], res["mean_s2d"], res["overall"])
    with open(os.path.join(args.vis_out_dir, "results.json"), "w") as fp:
        json.dump({k: res[k] for k in ("mean_d2s", "mean_s2d", "overall")}, fp, indent=True)
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
