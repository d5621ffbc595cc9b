#!/usr/bin/env python
"""Timing of the mesh texturing (TEXTURE.md) on the trained state's extracted mesh: one JSON line.

    python scripts/texture_bench.py [--res 1024] [--faces 200000] [--atlas 4096] [--views 32] [--repeat 3] [--trained-state PATH.ply]

The mesh is the bounded extraction at mesh_res after post_process_mesh, simplified to about --faces triangles (SIMPLIFY.md); the views
are OpenCV cameras at 1920 x 1080 with the Tanks-and-Temples intrinsics on an orbit at 1.5 times the radius of the mesh's bounding sphere
(scripts/cull_bench.py's), their images seeded noise (the kernels' work does not depend on what the images show).  Per stage the best of
--repeat runs, events on the stream: the density search (its probes, each a classify call with a host wait), the layout, the depth
images, the bake kernel, the resolve; then owned and seen texels, the (texel, view) pairs per second of the bake — every owned texel
against every view — and the share of pairs that passed every test.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "scripts")):
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


def run(dev, name, mesh, atlas, views, repeat, blend="average", batch=8):
    import cull_bench
    import surfel_cull as C
    import surfel_texture as P
    lo, hi = (x.cpu().numpy().astype(np.float64) for x in torch.aminmax(mesh.vertices, dim=0))
    center, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    w2c = C.world_to_camera(cull_bench.orbit(center, 1.5 * radius, views), "opencv")
    H, W, k = C.TNT_H, C.TNT_W, C.TNT_INTRINSICS
    zfar = max(C.ZFAR, 4 * radius)
    gen = torch.Generator(device=dev).manual_seed(0)
    best = {}

    def keep(stage, ms):
        best[stage] = ms if stage not in best else min(best[stage], ms)

    for _ in range(repeat):
        stats = {}
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        lay = P.atlas_layout(mesh, atlas_size=atlas, stats=stats)
        torch.cuda.synchronize(dev)
        keep("search_and_layout", (time.perf_counter() - t0) * 1e3)
        cls, counts = P.classify(mesh, lay.density)
        keep("layout", _timed(dev, lambda: P.layout(mesh, cls, counts, atlas, lay.density))[1])
        acc = P.new_accumulator(lay)
        depth_ms = bake_ms = 0.0
        for b in range(0, views, batch):
            depth, ms = _timed(dev, lambda: C.mesh_depth(mesh, w2c[b:b + batch], k, H, W, C.ZNEAR, zfar))
            depth_ms += ms
            images = torch.rand((depth.shape[0], 3, H, W), generator=gen, device=dev)
            bake_ms += _timed(dev, lambda: P.bake(mesh, lay, w2c[b:b + batch], k, depth, images, acc, blend=blend))[1]
            del depth, images
        keep("depth", depth_ms)
        keep("bake", bake_ms)
        (tex, counted), ms = _timed(dev, lambda: P.resolve(mesh, lay, acc, blend))
        keep("resolve", ms)
        owned, seen = (int(x) for x in counted.cpu())
    line = {"state": name, "V": int(mesh.vertices.shape[0]), "F": int(mesh.triangles.shape[0]), "atlas": [lay.width, lay.height], "views": views, "H": H, "W": W,
            "blend": blend, "density": float("%.6g" % lay.density), "probes": stats["probes"], "classes": lay.counts, "owned": owned, "seen": seen,
            "ms": {s: round(v, 3) for s, v in best.items()}, "bake_ms_per_view": round(best["bake"] / views, 4),
            "texel_views_per_s": float("%.4g" % (owned * views / (best["bake"] * 1e-3)))}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--faces", type=int, default=200000)
    ap.add_argument("--atlas", type=int, default=4096)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--trained-state", default=None, help="cached trained .ply")
    args = ap.parse_args()
    import helpers_bench as HB
    import mesh_bench
    import surfel_simplify
    dev = torch.device("cuda:0")
    model, train_cams, _, _, _ = HB.trained_state(dev, "trained", state=args.trained_state)
    ext, mesh, post = mesh_bench._run(dev, "trained", model, train_cams, args.res, quiet=True)
    del ext, mesh, model
    simple, _ = surfel_simplify.simplify_mesh(post, target_faces=args.faces)
    del post
    torch.cuda.empty_cache()
    run(dev, "trained/%d -> %d faces" % (args.res, simple.triangles.shape[0]), simple, args.atlas, args.views, args.repeat)


if __name__ == "__main__":
    main()
