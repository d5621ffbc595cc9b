#!/usr/bin/env python
"""Binning budget of the per-tile depth sort on the bench workloads' own frames (sibling of scripts/sort_ab.py, which takes synthetic
scenes through the bare forward): the timed window of a workload's trainer with every rasterizer stage bracketed by events, once per
"tile_depth_sort" setting (1 = the library's rule, 0 = depth-presorted emission, 2 = surfel-order emission + per-tile depth sort), and the
run lengths per tile (img.ranges) of four views of that window.  GPU only.

    python scripts/pertile_budget.py garden C4 [--steps 16]  ->  one JSON line per workload

budget_ms = sum of the stages below without tile_depth_sort under setting 2, set against their sum under setting 0: what a per-tile sorter
may cost before the per-tile path stops paying."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
sys.path.insert(0, REPO)
STAGES = ("depth_sort_scan", "emit_instances", "tile_sort", "tile_depth_sort", "blend_fwd", "blend_bwd", "preprocess_bwd")


def run_lengths():
    import torch
    import diff_surfel_rasterization as dsr
    buf, gx, gy = dsr._last_image
    ranges = buf[:gx * gy * 8].view(torch.int32).view(gy * gx, 2)
    return (ranges[:, 1] - ranges[:, 0]).cpu().numpy()


def main():
    import torch
    import synthetic
    import surfel_native
    import diff_surfel_rasterization as dsr
    from helpers_bench import TRAINED_PRESETS, make_trainer, reseed_views, trained_trainer, window_census
    args = sys.argv[1:]
    steps = 16
    if "--steps" in args:
        k = args.index("--steps")
        steps = int(args[k + 1])
        del args[k:k + 2]
    dev = torch.device("cuda:0")
    lib = surfel_native.load()
    for wl in args or ["garden", "C4"]:
        if wl in TRAINED_PRESETS:
            tr, _ = trained_trainer(dev, wl, os.environ.get("SURFEL_STATE_%s" % wl))
            W, H = TRAINED_PRESETS[wl]["res"]
        else:
            _, W, H, _ = synthetic.CONFIGS[wl]
            tr = make_trainer(dev, wl, n_views=8)
        for _ in range(max(10, len(tr.cams))):      # every view's buffer sizes seen before the windows
            tr.step()
        row = {"workload": wl, "P": int(tr.model.P), "tiles": ((W + 15) // 16) * ((H + 15) // 16), "steps": steps}
        for mode, name in ((1, "default"), (0, "presorted"), (2, "pertile")):
            lib.surfel_set_option(b"tile_depth_sort", mode)
            for _ in range(4):
                tr.step()
            torch.cuda.synchronize()
            st, cen = window_census(tr, steps, W, H)
            ms = {k: round(st[k][0] / st[k][1], 4) for k in STAGES if k in st}
            row[name] = {"stage_ms": ms, "sum_without_tile_depth_sort_ms": round(sum(v for k, v in ms.items() if k != "tile_depth_sort"), 4),
                         "R": round(cen["R"], 1)}
        lib.surfel_set_option(b"tile_depth_sort", 1)
        row["budget_ms"] = round(row["presorted"]["sum_without_tile_depth_sort_ms"] - row["pertile"]["sum_without_tile_depth_sort_ms"], 4)
        reseed_views(tr)
        n = []
        for _ in range(4):
            tr.step()
            torch.cuda.synchronize()
            n.append(run_lengths())
        n = np.concatenate(n)
        row["run_length"] = {"views": 4, "mean": round(float(n.mean()), 1), "quantiles_50_90_99_999": [int(np.percentile(n, q)) for q in (50, 90, 99, 99.9)],
                             "max": int(n.max()), "tiles_over": {str(k): int((n > k).sum()) for k in (256, 512, 1024, 2048, 3072, 4096, 8192)},
                             "instances_in_tiles_over": {str(k): int(n[n > k].sum()) for k in (256, 512, 1024, 2048, 3072, 4096, 8192)}}
        line = json.dumps(row)
        print(line, flush=True)
        del tr
        dsr.set_grad_arena(None)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
