"""Repair an extracted mesh on MI355X: cut the triangles on non-manifold and misoriented edges, split the vertices with more than one
fan, find the border loops and close the small ones — the steps that otherwise go through MeshLab ("remove faces from non-manifold
edges", "split non-manifold vertices", "close holes") or Open3D (remove_non_manifold_edges, fill_holes).

The half-edge sort, the cut, the pointer jumping over fans and loops and the ordered fp64 centroid sums are HIP kernels of
libsurfel_hip.so (include/surfel_repair.h); the rules they follow, operation for operation, are written down in REPAIR.md.  The mesh
stays on the device; only the counts cross to the host.  No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_repair.py --ply-path MESH.ply [--max_hole_edges N] [--report]      -> MESH_repaired.ply
"""
import argparse
import collections
import ctypes as C
import numbers
import os
import sys

import torch

import surfel_native as _n
from surfel_mesh import MeshLimitError, TriangleMesh, mesh_arrays, read_mesh  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

COUNTS = ("kept", "dropped", "cut_triangles", "nonmanifold_edges", "misoriented_edges", "split_vertices", "loops", "border_edges",
          "longest_loop", "filled_loops", "fill_triangles", "fill_vertices", "border_edges_after", "label_rounds")      # include/surfel_repair.h
STAGES = ("sort", "cut", "fans", "loops", "fill")      # stage_ms of include/surfel_repair.h; emit_ms is added to the last by repair_mesh

Loops = collections.namedtuple("Loops", "half_edge loop position lengths stats")
Loops.__doc__ = """The border loops of a mesh after the cut and the split (REPAIR.md §Rules 1-5), on the device: half_edge [B] int32, the border
half-edges 3 m + k of the repaired mesh's triangles in ascending order; loop [B] int32, the loop of each; position [B] int32, its distance
from the loop's smallest half-edge; lengths [n_loops] int32; stats: the COUNTS as a dict of ints (nothing filled)."""


def check_arguments(max_hole_edges):
    """REPAIR.md §Interface: ValueError for anything but a whole number >= 0 (a bool is no number here).  Returns it as an int."""
    ok = isinstance(max_hole_edges, numbers.Real) and not isinstance(max_hole_edges, bool)      # (numpy's bool_ is no Real)
    if not ok or not 0 <= max_hole_edges < 2 ** 62 or int(max_hole_edges) != max_hole_edges:      # (NaN fails the comparison)
        raise ValueError("surfel_repair: max_hole_edges must be a whole number >= 0, got %r" % (max_hole_edges,))
    return int(max_hole_edges)


def _analyze(mesh, cap, stage_ms=None):
    """(verts, tris, colors, plan, stats, allocator): rules 1-5 and the fill's sizes; the plan's arrays live in the allocator"""
    verts, tris, cols = mesh_arrays("surfel_repair", mesh, colors=True)
    dev = verts.device
    plan = _n.RepairPlan()
    counts = (C.c_int64 * len(COUNTS))()
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_repair_analyze", alloc.cb, None, verts.shape[0], tris.shape[0], verts, tris, cap, C.byref(plan), counts, stage_ms)
    return verts, tris, cols, plan, _n.counts_dict(COUNTS, counts), alloc


def repair_mesh(mesh, max_hole_edges=32, timings=None):
    """(TriangleMesh, stats): the mesh with every edge in at most two triangles of opposite direction, one fan per referenced vertex, and
    the border loops of at most max_hole_edges edges closed (REPAIR.md): a loop of three by one triangle, a longer one by a fan around
    its centroid.  The input's vertices stay at their indices, split copies and centroids follow; colours likewise.  stats: the COUNTS
    and vertex_source [V_out], triangle_source [F_out], loop_lengths [n_loops] (int32, on the device).  The input is not written; the
    same bytes on every run.  timings: a dict that receives one entry per stage, sort_ms .. fill_ms (synchronises)."""
    cap = check_arguments(max_hole_edges)
    stage_ms = (C.c_float * len(STAGES))() if timings is not None else None
    verts, tris, cols, plan, stats, alloc = _analyze(mesh, cap, stage_ms)
    dev = verts.device
    nv = plan.V + plan.split + plan.fill_vertices
    nt = plan.survivors + plan.fill_triangles
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_c = torch.empty(nv, 3, dtype=torch.float32, device=dev) if cols is not None else None
    out_t = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    vsrc = torch.empty(nv, dtype=torch.int32, device=dev)
    tsrc = torch.empty(nt, dtype=torch.int32, device=dev)
    lengths = torch.empty(plan.loops, dtype=torch.int32, device=dev)
    if timings is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
    _n.call(dev, "surfel_repair_emit", C.byref(plan), verts, cols, out_v, out_c, out_t, vsrc, tsrc, lengths)
    if timings is not None:
        ev[1].record()
        ev[1].synchronize()
        timings.update({"%s_ms" % k: float(v) for k, v in zip(STAGES, stage_ms)})
        timings["fill_ms"] += float(ev[0].elapsed_time(ev[1]))
    del alloc      # (the plan's arrays: the stream orders their reuse behind the kernels that read them)
    return TriangleMesh(out_v, out_t, out_c), dict(stats, vertex_source=vsrc, triangle_source=tsrc, loop_lengths=lengths)


def border_loops(mesh):
    """Loops: the border loops of the mesh after the cut and the split, nothing filled (REPAIR.md §Rules 1-5) — a report, and a way to
    choose max_hole_edges.  The half-edges are those of repair_mesh(mesh, max_hole_edges=0)'s triangles."""
    verts, tris, cols, plan, stats, alloc = _analyze(mesh, 0)
    dev = verts.device
    half_edge, loop, position = (torch.empty(plan.border, dtype=torch.int32, device=dev) for _ in range(3))
    lengths = torch.empty(plan.loops, dtype=torch.int32, device=dev)
    _n.call(dev, "surfel_repair_loops", C.byref(plan), half_edge, loop, position, lengths)
    del alloc
    return Loops(half_edge, loop, position, lengths, stats)


def summary(stats):
    """one line with the counts"""
    return ("%d triangles cut on %d non-manifold and %d misoriented edges, %d vertices split, %d of %d loops filled (longest %d edges) by %d "
            "triangles and %d vertices, %d of %d border edges left" %
            (stats["cut_triangles"], stats["nonmanifold_edges"], stats["misoriented_edges"], stats["split_vertices"], stats["filled_loops"],
             stats["loops"], stats["longest_loop"], stats["fill_triangles"], stats["fill_vertices"], stats["border_edges_after"],
             stats["border_edges"]))


def main(argv=None):
    import surfel_io
    ap = argparse.ArgumentParser(description="Repair a mesh: manifold cut, fan split and hole fill (REPAIR.md)")
    ap.add_argument("--ply-path", type=str, required=True, help="mesh to repair; MESH.ply -> MESH_repaired.ply")
    ap.add_argument("--max_hole_edges", type=int, default=32, help="close the border loops of at most this many edges; 0 closes none")
    ap.add_argument("--report", action="store_true", help="print the counts and a histogram of the loop lengths; write nothing")
    args = ap.parse_args(argv)
    cap = check_arguments(args.max_hole_edges)
    dev = torch.device("cuda:0")
    mesh = read_mesh(args.ply_path, dev)
    if args.report:
        loops = border_loops(mesh)
        print(", ".join("%s %d" % (k, loops.stats[k]) for k in COUNTS[:9]))
        lengths = loops.lengths.cpu().numpy()
        edge = 3
        while len(lengths) and edge <= int(lengths.max()):      # bins [3, 4), [4, 8), [8, 16), ...
            top = 4 if edge == 3 else 2 * edge
            inside = (lengths >= edge) & (lengths < top)
            print("loops of %d..%d edges: %d (%d edges)" % (edge, top - 1, int(inside.sum()), int(lengths[inside].sum())))
            edge = top
        return loops
    out, stats = repair_mesh(mesh, max_hole_edges=cap)
    stem = surfel_io.ply_stem(args.ply_path)
    surfel_io.write_triangle_mesh(stem + "_repaired.ply", out)
    print("%s -> %s" % (summary(stats), stem + "_repaired.ply"))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
