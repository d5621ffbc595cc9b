#!/usr/bin/env python
"""Timing of the mesh smoothing (SMOOTH.md) on the trained states' extracted meshes: one JSON line per state.

    python scripts/smooth_bench.py [--states trained,garden] [--res 1024] [--steps 100] [--trained-state PATH.ply] [--garden-state PATH.ply]

The mesh is the bounded extraction at mesh_res after post_process_mesh (what fuse_post.ply holds), obtained as scripts/simplify_bench.py
does.  Per state: V, F, the adjacency's counts; the adjacency in ms (events on the stream around the call, median of five after a warm-up);
one filter step in us (--steps steps in one call between events on the stream, median of five after a warm-up) and the bytes per second that
makes of the bytes a step must move — the CSR (offsets, flags, neighbours) once, every 12-byte position row read once and written once; the
rows the gathers ask for, 12 B per directed edge, are given beside it; the whole smooth_mesh call for 10 Taubin iterations between device
synchronisations (allocations and the host's part included), second of two runs.  Beside the step: the same step restated in torch on the
same adjacency — an fp32 index_add_ over the directed edges, a division and the blend — timed the same way, and the largest difference
between the two after one step (fp32 sums in arrival order against ordered fp64 sums).
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


def event_ms(fn, repeats=5):
    """median ms of fn() between two events on the current stream, after one warm-up call"""
    fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def torch_step(p, rows, nbrs, deg, f):
    """what a user would write: scatter-add the neighbours' rows, divide by the count, blend (fp32; float atomics inside index_add_)"""
    s = torch.zeros_like(p).index_add_(0, rows, p[nbrs])
    m = s / deg
    return torch.where(deg > 0, p + f * (m - p), p)


def run_state(dev, state, res, mesh, steps):
    import surfel_smooth as P
    V, F = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    adj_ms = event_ms(lambda: P.mesh_adjacency(mesh))
    adj = P.mesh_adjacency(mesh)
    E2 = adj.stats["directed_edges"]
    verts = mesh.vertices.float().contiguous()
    factors = [0.5, -0.53] * (steps // 2)
    hip_ms = event_ms(lambda: P.filter_steps(adj, verts, factors))
    deg = (adj.offsets[1:] - adj.offsets[:-1]).to(torch.float32)[:, None]
    rows = torch.repeat_interleave(torch.arange(V, device=dev), (adj.offsets[1:] - adj.offsets[:-1]).long())
    nbrs = adj.neighbors.long()

    def torch_steps():
        p = verts
        for f in factors:
            p = torch_step(p, rows, nbrs, deg, f)
        return p

    torch_ms = event_ms(torch_steps)
    one_hip = P.filter_steps(adj, verts, [0.5])
    one_torch = torch_step(verts, rows, nbrs, deg, 0.5)
    for _ in range(2):
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        out, stats = P.smooth_mesh(mesh, iterations=10)
        torch.cuda.synchronize(dev)
        call_ms = (time.perf_counter() - t0) * 1e3
    must = 4 * (V + 1) + V + 4 * E2 + 24 * V
    step_us = hip_ms[0] * 1e3 / len(factors)
    line = {"state": state, "mesh_res": res, "V": V, "F": F, "E2": E2, "border_edges": adj.stats["border_edges"],
            "nonmanifold_edges": adj.stats["nonmanifold_edges"], "boundary_vertices": adj.stats["boundary_vertices"],
            "isolated_vertices": adj.stats["isolated_vertices"], "max_degree": adj.stats["max_degree"], "dropped": adj.stats["dropped"],
            "adjacency_ms": round(adj_ms[0], 3), "adjacency_ms_min_max": [round(adj_ms[1], 3), round(adj_ms[2], 3)],
            "steps_timed": len(factors), "step_us": round(step_us, 2), "step_us_min_max": [round(hip_ms[1] * 1e3 / len(factors), 2), round(hip_ms[2] * 1e3 / len(factors), 2)],
            "step_bytes": must, "step_GBps": round(must / step_us / 1e3, 1), "gathered_bytes": 12 * E2,
            "torch_step_us": round(torch_ms[0] * 1e3 / len(factors), 2),
            "torch_step_us_min_max": [round(torch_ms[1] * 1e3 / len(factors), 2), round(torch_ms[2] * 1e3 / len(factors), 2)],
            "max_abs_diff_to_torch": float((one_hip - one_torch).abs().max()), "taubin10_call_ms": round(call_ms, 3)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", default="trained,garden")
    ap.add_argument("--res", default=1024, type=int)
    ap.add_argument("--steps", default=100, type=int, help="filter steps per timed call (an even number: Taubin pairs)")
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
        run_state(dev, name, args.res, post, args.steps)
        del post
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
