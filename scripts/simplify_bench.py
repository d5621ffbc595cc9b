#!/usr/bin/env python
"""Timing of the mesh simplification (SIMPLIFY.md) on the trained states' extracted meshes: one JSON line per (state, case).

    python scripts/simplify_bench.py [--states trained,garden] [--res 1024] [--cells 2,4,8] [--faces 200000] [--trained-state PATH.ply]
                                     [--garden-state PATH.ply]

The mesh is the bounded extraction at mesh_res after post_process_mesh (what fuse_post.ply holds).  Cases: a cell of K voxels for every
K of --cells, and the bisection towards --faces triangles.  Per case: V and F before and after, the milliseconds of the five stages
(keys, sorts, sums and solve, remap and dedupe, compaction; events on the stream) and of the bisection, the whole call between device
synchronisations, clusters, collapsed and duplicate triangles, and the edges that more than two triangles share.  Second of two runs.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def run_case(dev, state, res, mesh, case, repeat=2, **kw):
    import surfel_simplify
    for _ in range(repeat):
        timings = {}
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        out, stats = surfel_simplify.simplify_mesh(mesh, timings=timings, **kw)
        torch.cuda.synchronize(dev)
        wall = (time.perf_counter() - t0) * 1e3
    import surfel_smooth
    edges = surfel_smooth.mesh_adjacency(out).stats      # the triangles on every edge, from the vertex adjacency (SMOOTH.md)
    over, border = edges["nonmanifold_edges"], edges["border_edges"]
    line = {"state": state, "mesh_res": res, "case": case, "V": int(mesh.vertices.shape[0]), "F": int(mesh.triangles.shape[0]),
            "V_out": int(out.vertices.shape[0]), "F_out": int(out.triangles.shape[0]), "cell": float("%.6g" % stats["cell"]), "n": stats["n"],
            "probes": stats["probes"], "clusters": stats["clusters"], "collapsed": stats["collapsed"], "duplicates": stats["duplicates"],
            "edges_over_two": over, "edges_of_one": border, "ms": {k[:-3]: round(v, 3) for k, v in timings.items()}, "call_ms": round(wall, 3)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", default="trained,garden")
    ap.add_argument("--res", default=1024, type=int)
    ap.add_argument("--cells", default="2,4,8")
    ap.add_argument("--faces", default=200000, type=int)
    ap.add_argument("--garden-state", default=None, help="cached garden .ply (trained once, then loaded)")
    ap.add_argument("--trained-state", default=None, help="cached trained .ply")
    args = ap.parse_args()
    import helpers_bench as HB
    import mesh_bench
    dev = torch.device("cuda:0")
    for name in args.states.split(","):
        state = args.garden_state if name == "garden" else args.trained_state
        model, train_cams, _, _, _ = HB.trained_state(dev, name, state=state)
        ext, mesh, post = mesh_bench._run(dev, name, model, train_cams, args.res, quiet=True)
        voxel = 2.0 * ext.radius / args.res
        del ext, mesh, model
        torch.cuda.empty_cache()
        for k in (float(x) for x in args.cells.split(",")):
            run_case(dev, name, args.res, post, "cell %g voxels" % k, cell=k * voxel)
        run_case(dev, name, args.res, post, "%d faces" % args.faces, target_faces=args.faces)
        del post
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
