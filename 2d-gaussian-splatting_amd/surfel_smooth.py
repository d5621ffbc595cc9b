"""Smooth an extracted mesh on MI355X: the vertex adjacency as a device CSR and the Laplacian / Taubin filter over it — the step that
otherwise goes through Open3D (filter_smooth_taubin / filter_smooth_laplacian) or MeshLab.

The half-edge sort, the CSR and the ordered fp64 row sums are HIP kernels of libsurfel_hip.so (include/surfel_smooth.h); the rules they
follow, operation for operation, are written down in SMOOTH.md.  The mesh stays on the device; only the eight counts cross to the host.
No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_smooth.py --ply-path MESH.ply [--iterations N --method M --lam L --mu U --boundary B --colors]
                                                                                                                  -> MESH_smoothed.ply
"""
import argparse
import collections
import ctypes as C
import functools
import os
import sys

import torch

import surfel_native as _n
from surfel_mesh import MeshLimitError, TriangleMesh, mesh_arrays, read_mesh  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

METHODS = ("taubin", "laplacian")
BOUNDARY = ("free", "fixed", "curve")      # SURFEL_SMOOTH_FREE / _FIXED / _CURVE of include/surfel_smooth.h, in this order
COUNTS = ("kept", "dropped", "directed_edges", "border_edges", "nonmanifold_edges", "boundary_vertices", "isolated_vertices",
          "max_degree")                    # counts of include/surfel_smooth.h
FLAG_BOUNDARY, FLAG_NONMANIFOLD, FLAG_ISOLATED = 1, 2, 4

Adjacency = collections.namedtuple("Adjacency", "offsets neighbors multiplicity flags stats")
Adjacency.__doc__ = """The vertex adjacency of a mesh on the device (SMOOTH.md §Rules 3): offsets [V + 1] int32, neighbors [E2] int32 ascending
within each row, multiplicity [E2] int32 (the kept triangles on that edge: 1 a border edge, more than 2 a non-manifold one), flags [V] uint8
(FLAG_* bits), stats: the COUNTS as a dict of ints."""


_dev = functools.partial(_n.device_tensor, "surfel_smooth")
_rows = functools.partial(_n.rows, "surfel_smooth")


def check_arguments(iterations, method, lam, mu, boundary):
    """SMOOTH.md §Rules 5: ValueError for anything but N >= 0, a known method and boundary mode, 0 < lam <= 1 and, for taubin, mu < -lam.
    Returns the factors of the schedule's steps."""
    if method not in METHODS:
        raise ValueError("surfel_smooth: method must be one of %s, got %r" % (", ".join(METHODS), method))
    if boundary not in BOUNDARY:
        raise ValueError("surfel_smooth: boundary must be one of %s, got %r" % (", ".join(BOUNDARY), boundary))
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
        raise ValueError("surfel_smooth: iterations must be a whole number >= 0, got %r" % (iterations,))
    lam = float(lam)
    if not 0.0 < lam <= 1.0:
        raise ValueError("surfel_smooth: lam must lie in (0, 1], got %r" % (lam,))
    if method == "laplacian":
        return [lam] * int(iterations)
    mu = float(mu)
    if not mu < -lam:      # (NaN fails too)
        raise ValueError("surfel_smooth: taubin needs mu < -lam, got mu = %r, lam = %r" % (mu, lam))
    if mu == float("-inf"):
        raise ValueError("surfel_smooth: mu must be finite")
    return [lam, mu] * int(iterations)


def mesh_adjacency(mesh):
    """Adjacency of mesh.vertices [V, 3] / mesh.triangles [F, 3] (SMOOTH.md §Rules 1-3).  A triangle that names an index outside [0, V),
    repeats an index or names a vertex with a non-finite coordinate contributes nothing.  The same bytes on every run."""
    verts, tris = mesh_arrays("surfel_smooth", mesh)
    dev = verts.device
    V, F = verts.shape[0], tris.shape[0]
    offsets = torch.empty(V + 1, dtype=torch.int32, device=dev)
    neighbors = torch.empty(6 * F, dtype=torch.int32, device=dev)
    multiplicity = torch.empty(6 * F, dtype=torch.int32, device=dev)
    flags = torch.empty(V, dtype=torch.uint8, device=dev)
    counts = (C.c_int64 * len(COUNTS))()
    alloc = _n.TorchAllocator(dev)
    e2 = _n.call(dev, "surfel_smooth_adjacency", alloc.cb, None, V, F, verts, tris, offsets, neighbors, multiplicity, flags, counts)
    return Adjacency(offsets, neighbors[:e2], multiplicity[:e2], flags, _n.counts_dict(COUNTS, counts))


def filter_steps(adjacency, attribute, factors, boundary="free"):
    """[V, 3] float32: `attribute` after one step per entry of `factors` over the adjacency (SMOOTH.md §Rules 4); no entry returns a copy.
    The input is not written."""
    attr = _rows(attribute, "attribute", torch.float32)
    V = attr.shape[0]
    if adjacency.offsets.shape[0] != V + 1:
        raise ValueError("surfel_smooth: the adjacency has %d rows, the attribute %d" % (adjacency.offsets.shape[0] - 1, V))
    factors = [float(f) for f in factors]
    out = torch.empty_like(attr)
    scratch = torch.empty_like(attr) if len(factors) > 1 else None
    _n.call(attr.device, "surfel_smooth_steps", V, _dev(adjacency.offsets, "offsets"), _dev(adjacency.neighbors, "neighbors"),
            _dev(adjacency.multiplicity, "multiplicity"), _dev(adjacency.flags, "flags"), BOUNDARY.index(boundary), len(factors),
            (C.c_double * max(len(factors), 1))(*factors), attr, scratch, out)
    return out


def smooth_mesh(mesh, iterations=10, method="taubin", lam=0.5, mu=-0.53, boundary="free", colors=False, adjacency=None, timings=None):
    """(TriangleMesh, stats): the mesh with its vertices filtered over their edge neighbours with unit weights (SMOOTH.md) — `laplacian`:
    `iterations` steps with lam; `taubin`: `iterations` pairs of steps, lam then mu (Open3D's defaults).  boundary: `free` every neighbour
    counts (Open3D's rule), `fixed` boundary vertices keep their bits, `curve` a boundary vertex averages along the border only.  The
    triangles are the input's tensor; so are the colours, unless colors=True filters them through the same steps.  adjacency: a
    mesh_adjacency result of this mesh, to spare building it.  stats: the adjacency's counts, steps, and the Adjacency itself.  timings: a
    dict that receives adjacency_ms and steps_ms (synchronises)."""
    factors = check_arguments(iterations, method, lam, mu, boundary)
    cols = getattr(mesh, "vertex_colors", None)
    if colors and cols is None:
        raise ValueError("surfel_smooth: colors=True needs mesh.vertex_colors")
    # (not mesh_arrays: the triangles are checked where the adjacency is built, after the colours, and not at all when it is passed in)
    verts = _rows(mesh.vertices, "mesh.vertices", torch.float32)
    if colors and _rows(cols, "mesh.vertex_colors", torch.float32).shape[0] != verts.shape[0]:
        raise ValueError("surfel_smooth: %d colours for %d vertices" % (cols.shape[0], verts.shape[0]))
    dev = verts.device
    if timings is not None:
        torch.cuda.synchronize(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
    if adjacency is None:
        adjacency = mesh_adjacency(mesh)
    if timings is not None:
        ev[1].record()
    vout = filter_steps(adjacency, verts, factors, boundary)
    cout = filter_steps(adjacency, cols, factors, boundary) if colors else cols
    if timings is not None:
        ev[2].record()
        ev[2].synchronize()
        timings.update(adjacency_ms=float(ev[0].elapsed_time(ev[1])), steps_ms=float(ev[1].elapsed_time(ev[2])))
    stats = dict(adjacency.stats, steps=len(factors), adjacency=adjacency)
    return TriangleMesh(vout, mesh.triangles, cout), stats


def main(argv=None):
    import surfel_io
    ap = argparse.ArgumentParser(description="Smooth a mesh with a Laplacian or Taubin filter (SMOOTH.md)")
    ap.add_argument("--ply-path", type=str, required=True, help="mesh to smooth; MESH.ply -> MESH_smoothed.ply")
    ap.add_argument("--iterations", type=int, default=10, help="steps (laplacian) or pairs of steps (taubin)")
    ap.add_argument("--method", default="taubin", choices=METHODS)
    ap.add_argument("--lam", type=float, default=0.5, help="the shrinking step's factor, in (0, 1]")
    ap.add_argument("--mu", type=float, default=-0.53, help="taubin: the inflating step's factor, below -lam")
    ap.add_argument("--boundary", default="free", choices=BOUNDARY, help="free: every neighbour counts; fixed: boundary vertices stay; curve: a "
                    "boundary vertex averages along the border only")
    ap.add_argument("--colors", action="store_true", help="filter the vertex colours too")
    args = ap.parse_args(argv)
    check_arguments(args.iterations, args.method, args.lam, args.mu, args.boundary)
    dev = torch.device("cuda:0")
    mesh = read_mesh(args.ply_path, dev)
    out, stats = smooth_mesh(mesh, iterations=args.iterations, method=args.method, lam=args.lam, mu=args.mu, boundary=args.boundary, colors=args.colors)
    stem = surfel_io.ply_stem(args.ply_path)
    surfel_io.write_triangle_mesh(stem + "_smoothed.ply", out)
    print("%s, %d steps over %d vertices and %d directed edges (%d border, %d non-manifold edges, largest degree %d) -> %s" %
          (args.method, stats["steps"], mesh.vertices.shape[0], stats["directed_edges"], stats["border_edges"], stats["nonmanifold_edges"], stats["max_degree"],
           stem + "_smoothed.ply"))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
