#!/usr/bin/env python
"""Timing of the label pass (SELECT.md) on the trained states of helpers_bench, beside the contribution pass: one JSON line per state.

    python scripts/select_bench.py [--states trained,garden] [--views 8] [--rounds 3] [--trained-state PATH.ply] [--garden-state PATH.ply]

Per state and frame (medians and min-max over --views training views x --rounds rounds, all kinds interleaved view by view in one process,
each between two events on the stream, after a warm-up round):
  forward_ms         the forward the passes run behind (no gradient, exact binning, no tile stream)
  contribution_ms    surfel_rasterize_contribution on that forward's buffers: the yardstick, code this change leaves alone
  label_ms           surfel_rasterize_label_votes on the same buffers, per label image:
                       halves2     K = 2, label 0 left of the frame's middle column, 1 right of it (sub-tiles uniform but for one column of them)
                       checker2    K = 2, (x + y) % 2: every row of 16 lanes mixes labels
                       blocks32    K = 32, (x // 4 + y // 4) % 32: every sub-tile uniform, the large LDS bucket
  ratio              label_ms / contribution_ms
  atomics_per_frame  global atomics issued, counted by an instrumented, untimed run
The warm-up round checks every label run against the contribution pass: votes.sum(1) == sum_q, byte for byte.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from contrib_bench import timed  # noqa: E402


def label_images(W, H, dev):
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    return {"halves2": (2, (xs >= W // 2).to(torch.uint8).contiguous()),
            "checker2": (2, ((xs + ys) % 2).to(torch.uint8).contiguous()),
            "blocks32": (32, ((xs // 4 + ys // 4) % 32).to(torch.uint8).contiguous())}


def run_state(dev, name, model, cams, views, rounds):
    import diff_surfel_rasterization as dsr
    import surfel_native as n
    import surfel_prune as SP
    import surfel_select as SS
    import surfel_trainer as TR
    from surfel_render import rasterize_buffers
    pipe, bg = TR.pipeline_params(depth_ratio=1.0), torch.zeros(3, device=dev)
    dsr.set_grad_arena(None)
    cams = cams[:views]
    P = model.P
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    images = label_images(W, H, dev)

    def forward(cam):
        return rasterize_buffers(cam, model, pipe, bg, debug_bits=n.OPT_EXACT_BINNING)[3]

    t = {k: [] for k in ["forward", "contribution"] + list(images)}
    exact = True
    for r in range(rounds + 1):
        for cam in cams:
            c = SP.Contribution(P, dev)
            f_ms, buffers = timed(lambda: forward(cam))
            c_ms, _ = timed(lambda: c.add_view(buffers))
            ms = {}
            for kind, (K, L) in images.items():
                lv = SS.LabelVotes(P, K, dev)
                ms[kind], _ = timed(lambda: lv.add_view(buffers, L))
                if r == 0:      # warm-up round; its results check the pass against the contribution pass
                    exact = exact and bool(torch.equal(lv.votes.sum(1), c.sum_q))
            if r == 0:
                continue
            t["forward"].append(f_ms); t["contribution"].append(c_ms)
            for kind in images:
                t[kind].append(ms[kind])
    # global atomics: instrumented runs, not timed
    lib = n.load()

    def atomics(fn):
        stats = torch.zeros(8, dtype=torch.int64, device=dev)
        lib.surfel_debug_set_blend_stats(n.ptr(stats))
        try:
            for cam in cams:
                fn(forward(cam))      # (the forward counts its own figures into other slots; slot 7 is the passes')
            torch.cuda.synchronize()
        finally:
            lib.surfel_debug_set_blend_stats(None)
        return int(stats[7]) // len(cams)
    at = {"contribution": atomics(lambda b: SP.Contribution(P, dev).add_view(b))}
    for kind, (K, L) in images.items():
        at[kind] = atomics(lambda b, K=K, L=L: SS.LabelVotes(P, K, dev).add_view(b, L))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"state": name, "surfels": P, "res": [W, H], "views": len(cams), "rounds": rounds, "instances_per_frame": int(dsr.last_num_rendered),
           "forward_ms": round(med["forward"], 4), "forward_ms_min_max": [round(min(t["forward"]), 4), round(max(t["forward"]), 4)],
           "contribution_ms": round(med["contribution"], 4),
           "contribution_ms_min_max": [round(min(t["contribution"]), 4), round(max(t["contribution"]), 4)],
           "contribution_atomics_per_frame": at["contribution"], "row_sums_equal_sum_q": exact}
    for kind in images:
        out[kind] = {"label_ms": round(med[kind], 4), "label_ms_min_max": [round(min(t[kind]), 4), round(max(t[kind]), 4)],
                     "ratio": round(med[kind] / med["contribution"], 3), "atomics_per_frame": at[kind]}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--states", default="trained,garden")
    ap.add_argument("--views", default=8, type=int)
    ap.add_argument("--rounds", default=3, type=int)
    ap.add_argument("--trained-state", default=None, help="cached trained .ply (trained once, then loaded)")
    ap.add_argument("--garden-state", default=None, help="cached garden .ply (trained once, then loaded)")
    args = ap.parse_args(argv)
    import helpers_bench as HB
    dev = torch.device("cuda:0")
    for name in [s for s in args.states.split(",") if s]:
        state = args.garden_state if name == "garden" else args.trained_state
        model, train_cams, test_cams, extent, info = HB.trained_state(dev, name, state=state)
        res = run_state(dev, name, model, train_cams, args.views, args.rounds)
        res["workload"] = info["workload"]
        print(json.dumps(res), flush=True)
        del model, train_cams, test_cams
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
