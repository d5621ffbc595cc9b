#!/usr/bin/env python
"""Timing of the mesh viewer (MESHVIEW.md) on a trained state's bounded mesh: one JSON line.

    python scripts/meshview_bench.py [--res 1024] [--trained-state PATH.ply] [--views 32] [--repeat 3]

The mesh and the cameras are those of scripts/cull_bench.py: the trained state's mesh at mesh_res 1024 (not post-processed), seen at
1920 x 1080 with the Tanks-and-Temples intrinsics by `views` OpenCV cameras on an orbit at 1.5 times the radius of its bounding sphere.
Per supersampling factor (1 and 2) the line reports ms per view of the visibility buffer's small-class and large-class launches (timed
between events inside the library) and of the shading pass (between events here, mode "shaded" with vertex normals), triangles/s of the
visibility pass, and beside them the same figures of surfel_cull.mesh_depth on the same sample grid, so the cost of the 64-bit key is
visible.  Vertex normals are timed once.  The fastest of `repeat` runs counts.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "scripts"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(dev, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return out, e0.elapsed_time(e1)


def run(dev, name, mesh, views, repeat, factors=(1, 2)):
    import cull_bench
    import surfel_cull as C
    import surfel_meshview as P
    lo, hi = (x.cpu().numpy().astype(np.float64) for x in torch.aminmax(mesh.vertices, dim=0))
    center, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    w2c = C.world_to_camera(cull_bench.orbit(center, 1.5 * radius, views), "opencv")
    H, W, k = C.TNT_H, C.TNT_W, C.TNT_INTRINSICS
    zfar = max(C.ZFAR, 4 * radius)
    V, F = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    normals, normals_ms = None, None
    for _ in range(repeat):
        normals, ms = _timed(dev, lambda: P.vertex_normals(mesh))
        normals_ms = ms if normals_ms is None else min(normals_ms, ms)
    line = {"state": name, "V": V, "F": F, "views": views, "H": H, "W": W, "zfar": round(zfar, 3), "vertex_normals_ms": round(normals_ms, 4), "ssaa": {}}
    for s in factors:
        ks = P.scaled_intrinsics(k, s)
        best = None
        for _ in range(repeat):
            vis, dep = {}, {}
            key = P.visibility(mesh, w2c, ks, H * s, W * s, C.ZNEAR, zfar, timings=vis)
            frames, shade_ms = _timed(dev, lambda: P.shade(mesh, key, w2c, ks, H, W, s, "shaded", normals))
            covered = float((frames != 255).any(-1).float().mean())
            del key, frames
            depth = C.mesh_depth(mesh, w2c, ks, H * s, W * s, C.ZNEAR, zfar, timings=dep)
            del depth
            got = dict(small=vis["small_ms"], large=vis["large_ms"], other=vis["other_ms"], shade=shade_ms, depth_small=dep["small_ms"],
                       depth_large=dep["large_ms"], depth_other=dep["other_ms"], large_pairs=vis["large_pairs"], covered=covered)
            if best is None or got["small"] + got["large"] + got["shade"] < best["small"] + best["large"] + best["shade"]:
                best = got
        vis_ms = best["small"] + best["large"] + best["other"]
        depth_ms = best["depth_small"] + best["depth_large"] + best["depth_other"]
        line["ssaa"][str(s)] = {
            "covered": round(best["covered"], 4), "large_pairs": best["large_pairs"],
            "ms_per_view": {"small": round(best["small"] / views, 4), "large": round(best["large"] / views, 4), "other": round(best["other"] / views, 4),
                            "shade": round(best["shade"] / views, 4)},
            "triangles_per_s": float("%.4g" % (F * views / (vis_ms * 1e-3))),
            "mesh_depth_ms_per_view": {"small": round(best["depth_small"] / views, 4), "large": round(best["depth_large"] / views, 4),
                                       "other": round(best["depth_other"] / views, 4)},
            "mesh_depth_triangles_per_s": float("%.4g" % (F * views / (depth_ms * 1e-3))),
            "key_over_depth": round(vis_ms / depth_ms, 3)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--trained-state", default=None, help="cached trained .ply")
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import helpers_bench as HB
    import mesh_bench
    dev = torch.device("cuda:0")
    model, train_cams, _, _, _ = HB.trained_state(dev, "trained", state=args.trained_state)
    ext, mesh, _ = mesh_bench._run(dev, "trained", model, train_cams, args.res, quiet=True)
    del ext, model
    torch.cuda.empty_cache()
    run(dev, "trained/%d" % args.res, mesh, args.views, args.repeat)


if __name__ == "__main__":
    main()
