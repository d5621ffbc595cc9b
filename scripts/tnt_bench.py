#!/usr/bin/env python
"""Timing of the Tanks-and-Temples-style evaluation (TNT.md): one JSON line per case.

    python scripts/tnt_bench.py [--cases fixture,scaled] [--repeat 2]

fixture: the scene of tests/tnt_scenes.py (120 000 ground-truth points, 59 600 mesh points), the case tests/golden/make_golden_tnt.py
runs through the reference's run.py on CPUs.  scaled: the same surface with 4 000 000 ground-truth points and a mesh of 3 000 000
vertices and centroids, the size of a real scene.  Both start from the trajectory alignment of the scene's cameras (timed as
`trajectory`, host numpy) and run with the default criteria.  Parts are timed between device synchronisations (evaluate_tnt's
`timings`); the line reports the last of `repeat` runs.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

SCALED = {"gt_points": 4000000, "nlat": 707, "nlon": 1414}


def run(dev, name, scene, repeat):
    import surfel_eval_tnt as P
    import tnt_scenes as S
    from surfel_mesh import TriangleMesh
    v, t = S.mesh(scene)
    mesh = TriangleMesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), torch.zeros((len(v), 3), device=dev))
    gt = torch.from_numpy(S.ground_truth(scene)).to(dev)
    vol = P.CropVolume(**S.crop_fields(scene))
    est, col = S.cameras(scene)
    for _ in range(repeat):
        ms = {}
        r = P.evaluate_tnt(mesh, gt, vol, scene["tau"], est_traj=est, gt_traj=col, gt_trans=S.alignment(scene), seed=S.RANSAC_SEED, timings=ms)
    total = sum(ms.values())
    line = {"case": name, "V": len(v), "F": len(t), "gt_points": int(gt.shape[0]), "tau": scene["tau"],
            "precision": r["precision"], "recall": r["recall"], "fscore": r["fscore"], "scored": [r["source"], r["target"]],
            "stages": [{k: s[k] for k in ("source", "target", "iterations", "fitness", "inlier_rmse")} for s in r["stages"]],
            "ms": {k: round(x, 2) for k, x in ms.items()}, "ms_total": round(total, 2), "ms_device": round(total - ms.get("trajectory", 0.0), 2)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="fixture,scaled")
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    import tnt_scenes as S
    dev = torch.device("cuda:0")
    for name in args.cases.split(","):
        run(dev, name, S.FIXTURE if name == "fixture" else dict(S.FIXTURE, **SCALED), args.repeat)


if __name__ == "__main__":
    main()
