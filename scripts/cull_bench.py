#!/usr/bin/env python
"""Timing of the view culling (CULL.md) on a trained state's bounded mesh: one JSON line.

    python scripts/cull_bench.py [--res 1024] [--trained-state PATH.ply] [--views 32] [--repeat 3]

The mesh is the trained state's mesh at mesh_res 1024, built the way scripts/eval_bench.py gets it (not post-processed).  It is seen at
1920 x 1080 with the Tanks-and-Temples intrinsics by `views` OpenCV cameras on an orbit around the mesh's centre, at 1.5 times the
radius of its bounding sphere.  The depth kernels are timed between events inside the library (the small-class and the large-class launches
apart), the visibility kernel between events here; the line reports the fastest of `repeat` runs, per view.
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


def orbit(center, radius, n):
    """OpenCV camera-to-world poses [n, 4, 4] on a tilted circle around center, looking at it"""
    out = []
    for k in range(n):
        az, el = 2 * np.pi * k / n, 0.35 * np.sin(4 * np.pi * k / n)
        eye = center + radius * np.array([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el)])
        z = (center - eye) / np.linalg.norm(center - eye)
        x = np.cross([0.0, -1.0, 0.0], z)
        x /= np.linalg.norm(x)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
        out.append(m)
    return np.asarray(out, np.float32)


def run(dev, name, mesh, views, repeat):
    import surfel_cull as P
    lo, hi = (x.cpu().numpy().astype(np.float64) for x in torch.aminmax(mesh.vertices, dim=0))
    center, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    w2c = P.world_to_camera(orbit(center, 1.5 * radius, views), "opencv")
    H, W, k = P.TNT_H, P.TNT_W, P.TNT_INTRINSICS
    zfar = max(P.ZFAR, 4 * radius)
    best = None
    for _ in range(repeat):
        ms = {}
        depth = P.mesh_depth(mesh, w2c, k, H, W, P.ZNEAR, zfar, timings=ms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts = P.view_counts(mesh.vertices, depth, w2c, k)
        e1.record()
        torch.cuda.synchronize(dev)
        ms["visibility_ms"] = e0.elapsed_time(e1)
        if best is None or ms["small_ms"] + ms["large_ms"] + ms["visibility_ms"] < best["small_ms"] + best["large_ms"] + best["visibility_ms"]:
            best = ms
        covered = float((depth > 0).float().mean())
        del depth
    V, F = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    depth_ms = best["small_ms"] + best["large_ms"] + best["other_ms"]
    line = {"state": name, "V": V, "F": F, "views": views, "H": H, "W": W, "zfar": round(zfar, 3), "covered": round(covered, 4),
            "kept_vertices": int((counts >= P.MIN_VIEWS).sum()), "large_pairs": best["large_pairs"],
            "ms_per_view": {"depth_small": round(best["small_ms"] / views, 4), "depth_large": round(best["large_ms"] / views, 4),
                            "depth_other": round(best["other_ms"] / views, 4), "visibility": round(best["visibility_ms"] / views, 4)},
            "triangles_per_s": float("%.4g" % (F * views / (depth_ms * 1e-3))),
            "vertex_views_per_s": float("%.4g" % (V * views / (best["visibility_ms"] * 1e-3)))}
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
