#!/usr/bin/env python
"""Where the per-tile depth sort's register network hands over to the LDS radix: one launch over `tiles` runs of one length, float-depth
keys, the network forced (surfel_debug_set_tile_radix_min(2048)) against the radix forced (0).  GPU only.

    python scripts/tile_sort_classes.py [tiles]  ->  one JSON line per run length (us per launch, median of 20)"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))


def main():
    import torch
    import surfel_native as n
    dev = torch.device("cuda:0")
    tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 6700
    rng = np.random.default_rng(0)
    P = 2_000_000
    keys = torch.as_tensor(rng.uniform(0.2, 50.0, P).astype(np.float32).view(np.int32)).to(dev)
    for L in (64, 128, 192, 256, 320, 384, 512, 640, 768, 1024, 1280, 1536, 2048):
        total = tiles * L
        ids = np.sort(rng.integers(0, P - L, (tiles, L), dtype=np.int64), axis=1)
        ids += np.arange(L)[None, :]      # strictly ascending inside a run
        pl0 = torch.as_tensor(ids.astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
        start = np.arange(tiles, dtype=np.uint32) * L
        rg = torch.as_tensor(np.stack([start, start + L], axis=1).view(np.int32).reshape(-1)).to(dev)
        scratch = torch.empty(3 * total, dtype=torch.int32, device=dev)
        row = {"run_length": L, "tiles": tiles}
        for name, rmin in (("network_us", 2048), ("radix_us", 0)):
            n.call(None, "surfel_debug_set_tile_radix_min", rmin)
            ts = []
            for it in range(24):
                pl = pl0.clone()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                n.call(dev, "surfel_debug_tile_depth_sort", tiles, total, rg, pl, keys, scratch, 0)
                e1.record()
                torch.cuda.synchronize()
                if it >= 4:
                    ts.append(e0.elapsed_time(e1) * 1e3)
            row[name] = round(sorted(ts)[len(ts) // 2], 1)
        n.call(None, "surfel_debug_set_tile_radix_min", -1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
