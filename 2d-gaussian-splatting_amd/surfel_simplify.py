"""Simplify an extracted mesh on MI355X by quadric vertex clustering — the decimation step that otherwise goes through Open3D, MeshLab
or Blender.

The cell keys, the sorts, the ordered fp64 sums and the closed-form solve are HIP kernels of libsurfel_hip.so
(include/surfel_simplify.h); the rules they follow, operation for operation, are written down in SIMPLIFY.md.  The mesh stays on the
device; only counts and the six bounds cross to the host.  No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_simplify.py --ply-path MESH.ply [--cell C | --faces N | --ratio R]      -> MESH_simplified.ply
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

import surfel_native as _n
from surfel_mesh import MeshLimitError, TriangleMesh, mesh_arrays, read_mesh  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

LAM = 1e-3                      # the regulariser as a share of the quadric's trace (SIMPLIFY.md §Rules 6)
N_MAX = 1 << 20                 # the finest grid resolution the bisection tries: its cell indices fit 21 bits
STAGES = ("keys_ms", "sorts_ms", "sums_solve_ms", "remap_dedupe_ms", "compaction_ms")      # stage_ms of include/surfel_simplify.h
COUNTS = ("clusters", "vertices", "triangles", "dropped", "collapsed", "duplicates")        # counts of include/surfel_simplify.h


def _cell(cell):
    c = np.float32(cell)
    if not (np.isfinite(c) and c > 0):
        raise ValueError("surfel_simplify: the cell size must be positive and finite, got %r" % (cell,))
    return float(c)


def _origin(origin):
    if origin is None:
        return None
    o = np.asarray(origin.detach().cpu() if torch.is_tensor(origin) else origin, np.float32).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("surfel_simplify: origin must be three finite numbers")
    return (C.c_float * 3)(*o.tolist())


def mesh_bounds(vertices):
    """(lo [3], hi [3]) float32 on the host: the component-wise extrema of the vertices whose three coordinates are finite, computed on the
    device; None when no vertex is finite."""
    verts = _n.rows("surfel_simplify", vertices, "vertices", torch.float32)
    out = (C.c_float * 6)()
    alloc = _n.TorchAllocator(verts.device)
    if not _n.call(verts.device, "surfel_simplify_bounds", alloc.cb, None, verts.shape[0], verts, out):
        return None
    b = np.array(out[:], np.float32)
    return b[:3], b[3:]


def _bounds_arg(b):
    return None if b is None else (C.c_float * 6)(*np.concatenate(b).tolist())


def vertex_clusters(mesh, cell, origin=None):
    """int32 [V] on the device: per vertex the number of its grid cell among the occupied cells in key order (z, then y, then x), -1 for a
    vertex with a non-finite coordinate (SIMPLIFY.md §Rules 2, 3).  origin: the grid's corner, default the minimum of the finite vertices."""
    verts = _n.rows("surfel_simplify", mesh.vertices, "mesh.vertices", torch.float32)
    cluster = torch.empty(verts.shape[0], dtype=torch.int32, device=verts.device)
    alloc = _n.TorchAllocator(verts.device)
    _n.call(verts.device, "surfel_simplify_clusters", alloc.cb, None, verts.shape[0], verts, None, _origin(origin), _cell(cell), cluster)
    return cluster


def count_faces(mesh, cell, origin=None, bounds=None):
    """{clusters, triangles, dropped, collapsed, duplicates} of the mesh simplify_mesh would return at this cell size, without the sums,
    the solve and the outputs (SIMPLIFY.md §Rules 8: one probe of the bisection).  bounds: mesh_bounds' result, to spare its kernel."""
    verts, tris, _ = mesh_arrays("surfel_simplify", mesh, colors=True)
    counts = (C.c_int64 * len(COUNTS))()
    alloc = _n.TorchAllocator(verts.device)
    _n.call(verts.device, "surfel_simplify_count", alloc.cb, None, verts.shape[0], tris.shape[0], verts, tris, _bounds_arg(bounds), _origin(origin),
            _cell(cell), counts)
    return {k: v for k, v in _n.counts_dict(COUNTS, counts).items() if k != "vertices"}


def grid_cell(bounds, n):
    """The cell of grid resolution n (SIMPLIFY.md §Rules 8): the smallest fp32 >= fp32(longest extent / n) that puts the maximum into cell
    n - 1 — the quotient advanced by an ulp or two, so that the longest extent holds n cells and no extra layer with the extreme vertices
    alone.  fp32 throughout."""
    lo, hi = bounds
    ext = np.float32((hi - lo).max())
    if not ext > 0:
        return 1.0
    cell = ext / np.float32(n)
    while np.floor(ext / cell) >= n:
        cell = np.nextafter(cell, np.float32(np.inf))
    return float(cell)


def bisect_resolution(faces, target):
    """(n, probes): a grid resolution with faces(n) <= target < faces(n + 1).  faces(1) = 0 (one cell); the resolution doubles from 2 until
    the count passes the target (or N_MAX is reached: then n = N_MAX), then the bracket is halved.  The count is not exactly monotone in n,
    so the condition is the local one this search maintains."""
    lo, hi, probes = 1, 2, 0
    while True:
        probes += 1
        if faces(hi) > target:
            break
        lo = hi
        if hi == N_MAX:
            return lo, probes
        hi = min(2 * hi, N_MAX)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        if faces(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo, probes


def simplify_mesh(mesh, cell=None, target_faces=None, origin=None, lam=LAM, timings=None):
    """(TriangleMesh, stats): the mesh with one vertex per occupied grid cell, at the clamped minimiser of the cell's plane quadrics, and
    the triangles that still span three cells, each rotated triple once (SIMPLIFY.md).  cell: the cell's edge length; or target_faces: the
    grid resolution n is bisected so that faces(n) <= target_faces < faces(n + 1), cell = longest extent / n (a target of at least the
    mesh's triangle count returns the mesh unchanged, n = 0).  stats: clusters, vertices, triangles, dropped (rule 1), collapsed, duplicates,
    n, cell, probes, and the device tensors cluster [V] (the cell number of every input vertex) and cluster_vertex [clusters] (the output
    vertex of every cell, -1 for a cell no surviving triangle uses).  timings: a dict that receives the ms of the five stages and of the
    bisection (synchronises)."""
    if (cell is None) == (target_faces is None):
        raise ValueError("surfel_simplify: give cell or target_faces")
    verts, tris, cols = mesh_arrays("surfel_simplify", mesh, colors=True)
    dev = verts.device
    V, F = verts.shape[0], tris.shape[0]
    stats = {"n": 0, "probes": 0}
    bounds = None
    if target_faces is not None:
        if origin is not None:
            raise ValueError("surfel_simplify: target_faces places the grid itself (no origin)")
        if int(target_faces) < 0:
            raise ValueError("surfel_simplify: target_faces must not be negative")
        if int(target_faces) >= F:
            stats.update(clusters=V, vertices=V, triangles=F, dropped=0, collapsed=0, duplicates=0, cell=0.0, cluster=None, cluster_vertex=None)
            if timings is not None:
                timings.update({k: 0.0 for k in STAGES}, bisection_ms=0.0)
            return TriangleMesh(mesh.vertices, mesh.triangles, getattr(mesh, "vertex_colors", None)), stats
        bounds = mesh_bounds(verts)
        if bounds is None:
            cell = 1.0      # no finite vertex: every grid gives the empty mesh
        else:
            if timings is not None:
                torch.cuda.synchronize(dev)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
            probe = TriangleMesh(verts, tris, None)
            n, probes = bisect_resolution(lambda k: count_faces(probe, grid_cell(bounds, k), bounds=bounds)["triangles"], int(target_faces))
            if timings is not None:
                stop.record()
                stop.synchronize()
                timings["bisection_ms"] = float(start.elapsed_time(stop))
            cell = grid_cell(bounds, n)
            stats.update(n=n, probes=probes)
    cell = _cell(cell)
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    cluster_vertex = torch.empty(V, dtype=torch.int32, device=dev)
    vout = torch.empty((V, 3), dtype=torch.float32, device=dev)
    cout = torch.empty((V, 3), dtype=torch.float32, device=dev) if cols is not None else None
    tout = torch.empty((F, 3), dtype=torch.int32, device=dev)
    counts = (C.c_int64 * len(COUNTS))()
    ms = (C.c_float * len(STAGES))() if timings is not None else None
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_simplify_mesh", alloc.cb, None, V, F, verts, cols, tris, _bounds_arg(bounds), _origin(origin), cell, float(lam), cluster,
            cluster_vertex, vout, cout, tout, counts, ms)
    stats.update(_n.counts_dict(COUNTS, counts))
    nv, nf = stats["vertices"], stats["triangles"]
    stats.update(cell=cell, cluster=cluster, cluster_vertex=cluster_vertex[:stats["clusters"]])
    if timings is not None:
        timings.update({k: float(v) for k, v in zip(STAGES, ms)})
        timings.setdefault("bisection_ms", 0.0)
    return TriangleMesh(vout[:nv], tout[:nf], cout[:nv] if cout is not None else None), stats


def main(argv=None):
    import surfel_io
    ap = argparse.ArgumentParser(description="Simplify a mesh by quadric vertex clustering (SIMPLIFY.md)")
    ap.add_argument("--ply-path", type=str, required=True, help="mesh to simplify; MESH.ply -> MESH_simplified.ply")
    ap.add_argument("--cell", type=float, default=None, help="edge length of a grid cell")
    ap.add_argument("--faces", type=int, default=None, help="target triangle count: the grid resolution is bisected")
    ap.add_argument("--ratio", type=float, default=None, help="target triangle count as a share of the input's")
    ap.add_argument("--lam", type=float, default=LAM, help="regulariser towards the cell's mean vertex, as a share of the quadric's trace")
    args = ap.parse_args(argv)
    if sum(x is not None for x in (args.cell, args.faces, args.ratio)) != 1:
        raise SystemExit("give exactly one of --cell, --faces and --ratio")
    dev = torch.device("cuda:0")
    mesh = read_mesh(args.ply_path, dev)
    V, F = mesh.vertices.shape[0], mesh.triangles.shape[0]
    target = args.faces if args.faces is not None else (int(args.ratio * F) if args.ratio is not None else None)
    out, stats = simplify_mesh(mesh, cell=args.cell, target_faces=target, lam=args.lam)
    stem = surfel_io.ply_stem(args.ply_path)
    surfel_io.write_triangle_mesh(stem + "_simplified.ply", out)
    print("cell %g (n = %d): %d of %d vertices, %d of %d triangles (%d collapsed, %d duplicates) -> %s" %
          (stats["cell"], stats["n"], out.vertices.shape[0], V, out.triangles.shape[0], F, stats["collapsed"], stats["duplicates"],
           stem + "_simplified.ply"))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
