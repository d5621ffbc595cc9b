#!/usr/bin/env python
"""Timing of the mesh repair (REPAIR.md) on the trained states' extracted meshes: one JSON line per state and cap.

    python scripts/repair_bench.py [--states trained,garden] [--res 1024] [--trained-state PATH.ply] [--garden-state PATH.ply]

The mesh is the bounded extraction at mesh_res after post_process_mesh (what fuse_post.ply holds), obtained as scripts/smooth_bench.py
does.  Per state and cap — 0, 32 and one above the longest loop —: V, F, every count of the repair and label_rounds; the stages in ms
(sort, cut, fans, loops, fill: events on the stream, median of five calls after a warm-up; fill is the bookkeeping of the analysis plus
the emit entry); the whole repair_mesh call between device synchronisations (allocations and the host's part included), median of five
with the smallest and largest beside it; what the smoothing's adjacency finds on the output (non-manifold and border edges).  Beside
it, in the same run, the yardstick: mesh_adjacency of the input, which makes one sort and one pass over the same half-edges.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def run_state(dev, state, res, mesh):
    import surfel_repair as P
    import surfel_smooth
    from smooth_bench import event_ms
    V, F = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    adj_ms = event_ms(lambda: surfel_smooth.mesh_adjacency(mesh))
    before = surfel_smooth.mesh_adjacency(mesh).stats
    longest = P.border_loops(mesh).stats["longest_loop"]
    for cap in (0, 32, longest + 1):
        P.repair_mesh(mesh, max_hole_edges=cap)      # warm-up
        stages, calls = [], []
        for _ in range(5):
            timings = {}
            torch.cuda.synchronize(dev); t0 = time.perf_counter()
            out, stats = P.repair_mesh(mesh, max_hole_edges=cap, timings=timings)
            torch.cuda.synchronize(dev)
            calls.append((time.perf_counter() - t0) * 1e3)
            stages.append(timings)
        plain = []
        for _ in range(5):      # without the stage events
            torch.cuda.synchronize(dev); t0 = time.perf_counter()
            out, stats = P.repair_mesh(mesh, max_hole_edges=cap)
            torch.cuda.synchronize(dev)
            plain.append((time.perf_counter() - t0) * 1e3)
        after = surfel_smooth.mesh_adjacency(out).stats
        line = {"state": state, "mesh_res": res, "max_hole_edges": cap, "V": V, "F": F}
        line.update({k: stats[k] for k in P.COUNTS})
        line.update({"V_out": int(out.vertices.shape[0]), "F_out": int(out.triangles.shape[0])})
        line.update({"%s_ms" % s: round(statistics.median(t["%s_ms" % s] for t in stages), 3) for s in P.STAGES})
        line.update({"call_ms": round(statistics.median(plain), 3), "call_ms_min_max": [round(min(plain), 3), round(max(plain), 3)],
                     "timed_call_ms": round(statistics.median(calls), 3),
                     "adjacency_ms": round(adj_ms[0], 3), "adjacency_ms_min_max": [round(adj_ms[1], 3), round(adj_ms[2], 3)],
                     "input_nonmanifold_edges": before["nonmanifold_edges"], "input_border_edges": before["border_edges"],
                     "output_nonmanifold_edges": after["nonmanifold_edges"], "output_border_edges": after["border_edges"]})
        print(json.dumps(line), flush=True)
        del out, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", default="trained,garden")
    ap.add_argument("--res", default=1024, type=int)
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
        del ext, mesh, model
        torch.cuda.empty_cache()
        run_state(dev, name, args.res, post)
        del post
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
