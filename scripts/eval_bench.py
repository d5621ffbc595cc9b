#!/usr/bin/env python
"""Timing of the mesh evaluation (EVAL.md) on a trained state's bounded mesh: one JSON line per case.

    python scripts/eval_bench.py [--states trained] [--res 1024] [--trained-state PATH.ply] [--repeat 2]

The mesh (mesh_res as given, not post-processed) is evaluated against a ground-truth cloud made from the same mesh: sampled at the same
density, thinned with another seed and moved by a known offset of two voxels along x, so both chamfer means are known to lie between
0 and the offset.  density = voxel / 2; the observation mask is all ones over the mesh's bounding box, the plane keeps every point.
Stages are timed between device synchronisations (evaluate_dtu's `timings`); the line reports the last of `repeat` runs.
--states sphere: the scaled fixture scene of tests/eval_scenes.py (SCALED) with the reference's default parameters instead, the case
tests/golden/make_golden_eval.py --time runs through the reference's eval.py on CPUs.
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


def run(dev, name, mesh, voxel, repeat=2):
    import surfel_eval
    density, offset = voxel / 2, 2 * voxel
    gt = surfel_eval.sample_mesh(mesh, density)
    gt = gt[surfel_eval.thin(gt, density, seed=1)] + torch.tensor([offset, 0.0, 0.0], device=dev)
    lo, hi = (x.cpu().numpy() for x in torch.aminmax(mesh.vertices, dim=0))
    res = float((hi - lo).max()) / 255
    mask = torch.ones(tuple(int(x) for x in np.floor((hi - lo) / res) + 2), dtype=torch.uint8, device=dev)
    for _ in range(repeat):
        ms = {}
        r = surfel_eval.evaluate_dtu(mesh, gt, mask, np.stack([lo, hi]), res, (0.0, 0.0, 0.0, 1.0), density=density, patch=60 * voxel,
                                     max_dist=20 * voxel, seed=0, timings=ms)
    total = sum(ms.values())
    line = {"state": name, "V": int(mesh.vertices.shape[0]), "F": int(mesh.triangles.shape[0]), "voxel_size": round(voxel, 6), "density": round(density, 6),
            "offset": round(offset, 6), "points": {k: r[k] for k in ("data_pcd", "data_down", "data_in", "data_in_obs", "stl", "stl_above")},
            "rounds": r["rounds"], "mean_d2s": r["mean_d2s"], "mean_s2d": r["mean_s2d"], "overall": r["overall"],
            "ms": {k: round(x, 2) for k, x in ms.items()}, "ms_total": round(total, 2),
            "thin_points_per_s": float("%.4g" % (r["data_pcd"] / (ms["thin"] * 1e-3))),
            "d2s_queries_per_s": float("%.4g" % (r["data_in_obs"] / (ms["d2s"] * 1e-3))),
            "s2d_queries_per_s": float("%.4g" % (r["stl_above"] / (ms["s2d"] * 1e-3)))}
    print(json.dumps(line), flush=True)


def run_sphere(dev, repeat=2):
    import eval_scenes as S
    import surfel_eval
    from surfel_mesh import TriangleMesh
    v, t = S.fixture_mesh(S.SCALED)
    mesh = TriangleMesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), torch.zeros((len(v), 3), device=dev))
    stl = torch.from_numpy(S.fixture_ground_truth(S.SCALED)).to(dev)
    mask, bb, res, plane = S.fixture_obs(S.SCALED)
    mask = torch.from_numpy(mask).to(dev)
    for _ in range(repeat):
        ms = {}
        r = surfel_eval.evaluate_dtu(mesh, stl, mask, bb, res, plane, seed=0, timings=ms, **S.PARAMS[0])
    line = {"state": "sphere", "V": len(v), "F": len(t), "points": {k: r[k] for k in ("data_pcd", "data_down", "data_in", "data_in_obs", "stl", "stl_above")},
            "rounds": r["rounds"], "mean_d2s": r["mean_d2s"], "mean_s2d": r["mean_s2d"], "overall": r["overall"],
            "ms": {k: round(x, 2) for k, x in ms.items()}, "ms_total": round(sum(ms.values()), 2)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", default="trained")
    ap.add_argument("--res", default="1024")
    ap.add_argument("--trained-state", default=None, help="cached trained .ply")
    ap.add_argument("--garden-state", default=None, help="cached garden .ply")
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    import helpers_bench as HB
    import mesh_bench
    dev = torch.device("cuda:0")
    for name in args.states.split(","):
        if name == "sphere":
            run_sphere(dev, args.repeat)
            continue
        model, train_cams, _, _, _ = HB.trained_state(dev, name, state=args.garden_state if name == "garden" else args.trained_state)
        for res in (int(r) for r in args.res.split(",")):
            ext, mesh, _ = mesh_bench._run(dev, name, model, train_cams, res, quiet=True)
            voxel = 2.0 * ext.radius / res
            del ext
            torch.cuda.empty_cache()
            run(dev, "%s/%d" % (name, res), mesh, voxel, args.repeat)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
