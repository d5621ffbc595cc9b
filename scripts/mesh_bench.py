#!/usr/bin/env python
"""Timing of the bounded TSDF mesh extraction (MESH.md) on trained states: one JSON line per (state, mesh_res).

    python scripts/mesh_bench.py [--states trained,garden] [--res 512,1024] [--garden-state PATH.ply] [--model-dir DIR] [--unbounded]

Every stage is timed with a device synchronisation around it: render (every view through render()), touch (allocation passes and
pool allocation), integrate (touch lists + fusion of every view), extract (counts, scans, emission), clusters (post_process_mesh).
--model-dir: also writes the `trained` state as a model directory the CLI reads (point_cloud/iteration_N/point_cloud.ply +
cameras.json) so that `surfel_mesh.py -m DIR` can be run on it.
--unbounded: the unbounded extraction (MESH.md §Unbounded) at resolution N = res instead: render, fuse (view packing + lattice
fusion), extract (both slab sweeps), color, clusters; M, V, F and the fusion's sample-views per second.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_model_dir(model, cams, out, iteration):
    """point_cloud/iteration_N/point_cloud.ply and cameras.json in the reference's layout (utils/camera_utils.py:64-84's fields)."""
    d = os.path.join(out, "point_cloud", "iteration_%d" % iteration)
    os.makedirs(d, exist_ok=True)
    model.save_ply(os.path.join(d, "point_cloud.ply"))
    entries = []
    for k, c in enumerate(cams):
        R = np.asarray(c.R, np.float64); T = np.asarray(c.T, np.float64)
        W, H = c.image_width, c.image_height
        entries.append({"id": k, "img_name": c.image_name, "width": W, "height": H, "position": (-R @ T).tolist(), "rotation": R.tolist(),
                        "fy": H / (2 * np.tan(c.FoVy / 2)), "fx": W / (2 * np.tan(c.FoVx / 2))})
    json.dump(entries, open(os.path.join(out, "cameras.json"), "w"))


def run(dev, name, model, cams, res, repeat=2):
    """`repeat` extractions; the line reports the last (the first pays the one-time costs: code objects, allocator growth)."""
    for _ in range(repeat - 1):
        _run(dev, name, model, cams, res, quiet=True)
    return _run(dev, name, model, cams, res)


def _run(dev, name, model, cams, res, quiet=False):
    import surfel_mesh
    from surfel_render import render
    import surfel_trainer as TR
    timings = {}
    ext = surfel_mesh.GaussianExtractor(model, render, TR.pipeline_params(depth_ratio=0.0))
    ext.timings = timings
    sh = model.active_sh_degree
    model.active_sh_degree = 0
    ext.reconstruction(cams)
    depth_trunc = 2.0 * ext.radius
    voxel = depth_trunc / res
    mesh = ext.extract_mesh_bounded(voxel_size=voxel, sdf_trunc=5 * voxel, depth_trunc=depth_trunc)
    torch.cuda.synchronize(dev); t0 = time.perf_counter()
    post = surfel_mesh.post_process_mesh(mesh, 50)
    torch.cuda.synchronize(dev)
    timings["clusters"] = (time.perf_counter() - t0) * 1e3
    model.active_sh_degree = sh
    v = ext.volume.v
    if quiet:
        return ext, mesh, post
    touched = []      # an untimed second fusion that counts every view's touched blocks: the integrate kernel's traffic
    depths, rgbas, cb = [], [], []
    for i, cam in enumerate(ext.viewpoint_stack):
        d, rgba = surfel_mesh.prepare_view(ext.depthmaps[i], ext.rgbmaps[i], None, depth_trunc)
        depths.append(d); rgbas.append(rgba); cb.append(torch.from_numpy(surfel_mesh.camera_block(cam)).to(dev))
    again = surfel_mesh.fuse(depths, rgbas, cb, voxel, 5 * voxel, depth_trunc, ext.budget_bytes, dev, touched=touched)
    updates = int(again.blocks()[2].double().sum()) if again.v.nblocks else 0      # = voxel updates over all views
    line = {"state": name, "mesh_res": res, "views": len(cams), "image": [cams[0].image_width, cams[0].image_height],
            "voxel_size": round(voxel, 6), "blocks": int(v.nblocks), "table_blocks": int(np.prod(list(v.dims))),
            "voxel_bytes": int(v.nblocks) * 4096 * 20, "V": int(mesh.vertices.shape[0]), "F": int(mesh.triangles.shape[0]),
            "V_post": int(post.vertices.shape[0]), "F_post": int(post.triangles.shape[0]),
            "touched_blocks": int(sum(touched)), "voxel_updates": updates,
            # integrate: an updated voxel's 20 B record read and written, its 4 B depth and 4 B colour gathered; a touched voxel that
            # is not updated reads only its pixel's depth (4 B) when it projects into the image
            "integrate_bytes": updates * 48 + (int(sum(touched)) * 4096 - updates) * 4,
            "ms": {k: round(x, 2) for k, x in timings.items()}}
    print(json.dumps(line), flush=True)
    return ext, mesh, post


def run_unbounded(dev, name, model, cams, res, repeat=2):
    """`repeat` extractions; the line reports the last."""
    import surfel_mesh
    from surfel_render import render
    import surfel_trainer as TR
    for k in range(repeat):
        timings = {}
        ext = surfel_mesh.GaussianExtractor(model, render, TR.pipeline_params(depth_ratio=0.0))
        ext.timings = timings
        sh = model.active_sh_degree
        model.active_sh_degree = 0
        ext.reconstruction(cams)
        mesh = ext.extract_mesh_unbounded(res)
        torch.cuda.synchronize(dev); t0 = time.perf_counter()
        post = surfel_mesh.post_process_mesh(mesh, 50)
        torch.cuda.synchronize(dev)
        timings["clusters"] = (time.perf_counter() - t0) * 1e3
        model.active_sh_degree = sh
        M = int(ext.lattice.v.M)
        line = {"state": name, "mode": "unbounded", "resolution": res, "M": M, "R": round(float(ext.lattice.v.R), 5), "views": len(cams),
                "image": [cams[0].image_width, cams[0].image_height], "slabs": int(ext.lattice.v.nslabs),
                "V": int(mesh.vertices.shape[0]), "F": int(mesh.triangles.shape[0]),
                "V_post": int(post.vertices.shape[0]), "F_post": int(post.triangles.shape[0]),
                "ms": {k_: round(x, 2) for k_, x in timings.items()},
                "fuse_sample_views_per_s": float("%.4g" % (M ** 3 * len(cams) / (timings["fuse"] * 1e-3)))}
        del ext, mesh, post
        torch.cuda.empty_cache()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", default="trained,garden")
    ap.add_argument("--res", default="512,1024")
    ap.add_argument("--garden-state", default=None, help="cached garden .ply (trained once, then loaded)")
    ap.add_argument("--trained-state", default=None, help="cached trained .ply")
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--unbounded", action="store_true", help="time extract_mesh_unbounded (res = resolution N, a multiple of 512)")
    args = ap.parse_args()
    import helpers_bench as HB
    dev = torch.device("cuda:0")
    for name in args.states.split(","):
        state = args.garden_state if name == "garden" else args.trained_state
        model, train_cams, _, _, info = HB.trained_state(dev, name, state=state)
        if args.model_dir and name == "trained":
            write_model_dir(model, train_cams, args.model_dir, 6000)
        for res in (int(r) for r in args.res.split(",")):
            (run_unbounded if args.unbounded else run)(dev, name, model, train_cams, res)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
