#!/usr/bin/env python
"""Timing of the contribution pass (CONTRIB.md) on the trained states of helpers_bench: one JSON line per state.

    python scripts/contrib_bench.py [--states trained,garden] [--views 8] [--rounds 3] [--trained-state PATH.ply] [--garden-state PATH.ply]
                                    [--prune-study]

Per state and frame (medians over --views training views x --rounds rounds, the three kinds interleaved view by view in one process,
each between two events on the stream, after a warm-up round):
  forward_ms        the forward the pass runs behind (no gradient, exact binning, no tile stream)
  contribution_ms   surfel_rasterize_contribution on that forward's buffers (its read-back of the counting mode included)
  backward_route_ms forward + backward with colors_precomp and a constant image gradient: dL/dcolour[:, 0] is the sum of the blend
                    weights — the only route to it without the pass, through functions this change leaves alone
  pairs_per_s, flush_atomics_per_s   composited pairs, and global atomics issued (counted by an instrumented, untimed run), per second of the pass
and the largest relative difference between the pass' sums and the backward route's.

--prune-study (the trained state only): surfels removed by min_max_weight at 1e-3, 1e-2, 1e-1 over the training views, and the held-out
PSNR before pruning, right after it and after 1000 further iterations without densification.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "scripts")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def run_state(dev, name, model, cams, views, rounds):
    import diff_surfel_rasterization as dsr
    import surfel_native as n
    import surfel_prune as SP
    import surfel_trainer as TR
    from surfel_render import rasterize, rasterize_buffers
    pipe, bg = TR.pipeline_params(depth_ratio=1.0), torch.zeros(3, device=dev)
    dsr.set_grad_arena(None)
    cams = cams[:views]
    P = model.P
    ones = torch.ones((P, 3), device=dev)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    gC = torch.zeros((3, H, W), device=dev); gC[0] = 1.0

    def forward(cam):
        return rasterize_buffers(cam, model, pipe, bg, debug_bits=n.OPT_EXACT_BINNING)[3]

    def backward_route(cam):
        col = ones.clone().requires_grad_(True)
        image = rasterize(cam, model, pipe, bg, override_color=col)[0]
        image.backward(gC)
        return col.grad[:, 0]

    t = {"forward": [], "contribution": [], "backward_route": []}
    pairs, worst = [], 0.0
    for r in range(rounds + 1):
        for cam in cams:
            c = SP.Contribution(P, dev)
            f_ms, buffers = timed(lambda: forward(cam))
            c_ms, _ = timed(lambda: c.add_view(buffers))
            b_ms, ref = timed(lambda: backward_route(cam))
            if r == 0:      # warm-up round; its results check the pass against the route it replaces
                sw, hits = c.sum_w, c.hits.to(torch.float64)
                err = ((sw - ref.double()).abs() - hits * 2.0 ** -24).clamp(min=0) / ref.double().abs().clamp(min=1e-6)
                worst = max(worst, float(err.max()))
                pairs.append(int(c.hits.sum()))
                continue
            t["forward"].append(f_ms); t["contribution"].append(c_ms); t["backward_route"].append(b_ms)
    # global atomics of the pass: an instrumented run, not timed
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    lib = n.load()
    lib.surfel_debug_set_blend_stats(n.ptr(stats))
    try:
        for cam in cams:
            SP.Contribution(P, dev).add_view(forward(cam))
        torch.cuda.synchronize()
    finally:
        lib.surfel_debug_set_blend_stats(None)
    atomics = int(stats[7]) / len(cams)
    med = {k: statistics.median(v) for k, v in t.items()}
    mean_pairs = sum(pairs) / len(pairs)
    return {"state": name, "surfels": P, "res": [W, H], "views": len(cams), "rounds": rounds, "instances_per_frame": int(dsr.last_num_rendered),
            "forward_ms": round(med["forward"], 4), "contribution_ms": round(med["contribution"], 4), "backward_route_ms": round(med["backward_route"], 4),
            "contribution_ms_min_max": [round(min(t["contribution"]), 4), round(max(t["contribution"]), 4)],
            "backward_route_ms_min_max": [round(min(t["backward_route"]), 4), round(max(t["backward_route"]), 4)],
            "pairs_per_frame": int(mean_pairs), "pairs_per_s": round(mean_pairs / (med["contribution"] * 1e-3), 1),
            "flush_atomics_per_frame": int(atomics), "flush_atomics_per_s": round(atomics / (med["contribution"] * 1e-3), 1),
            "pairs_per_atomic": round(mean_pairs / max(atomics, 1), 2), "cheaper_than_backward_route": med["contribution"] < med["backward_route"],
            "max_rel_diff_vs_backward_route": worst}


def prune_study(dev, model, train_cams, test_cams, extent, trained_iters, thresholds=(1e-3, 1e-2, 1e-1), recover_iters=1000):
    import diff_surfel_rasterization as dsr
    import surfel_model
    import surfel_prune as SP
    import surfel_trainer as TR
    pipe, bg = TR.pipeline_params(depth_ratio=1.0), torch.zeros(3, device=dev)
    dsr.set_grad_arena(None)
    c = SP.contribution(model, train_cams, pipe, bg)
    out = {"study": "prune and recover", "surfels": model.P, "views": len(train_cams), "unseen": int(SP.unseen_mask(c).sum()), "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        ply = os.path.join(tmp, "state.ply")
        model.save_ply(ply)
        for thr in thresholds:
            m = surfel_model.GaussianModel(3, device=dev)
            m.load_ply(ply); m.active_sh_degree = 3; m.spatial_lr_scale = extent
            # the state's own schedule, continued: same loss weights, the learning-rate decay stretched to the new end, no densification
            end = trained_iters + recover_iters + 1
            opt = TR.optimization_params(iterations=end, lambda_dist=100.0, densify_until_iter=0, position_lr_max_steps=end)
            tr = TR.Trainer(m, train_cams, opt, pipe, extent=extent, solo=True, first_iter=trained_iters)
            before = tr.evaluate(test_cams)[0]
            removed = SP.prune_model(m, SP.prune_mask(c, min_max_weight=thr))
            after = tr.evaluate(test_cams)[0]
            for _ in range(recover_iters):
                tr.step()
            out["cases"].append({"min_max_weight": thr, "removed": removed, "kept": m.P, "psnr_heldout_before": round(before, 3),
                                 "psnr_heldout_pruned": round(after, 3), "psnr_heldout_recovered": round(tr.evaluate(test_cams)[0], 3)})
            del tr, m
            dsr.set_grad_arena(None)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--states", default="trained,garden")
    ap.add_argument("--views", default=8, type=int)
    ap.add_argument("--rounds", default=3, type=int)
    ap.add_argument("--trained-state", default=None, help="cached trained .ply (trained once, then loaded)")
    ap.add_argument("--garden-state", default=None, help="cached garden .ply (trained once, then loaded)")
    ap.add_argument("--prune-study", action="store_true")
    args = ap.parse_args(argv)
    import helpers_bench as HB
    dev = torch.device("cuda:0")
    for name in [s for s in args.states.split(",") if s]:
        state = args.garden_state if name == "garden" else args.trained_state
        model, train_cams, test_cams, extent, info = HB.trained_state(dev, name, state=state)
        res = run_state(dev, name, model, train_cams, args.views, args.rounds)
        res["workload"] = info["workload"]
        print(json.dumps(res), flush=True)
        if args.prune_study and name == "trained":
            print(json.dumps(prune_study(dev, model, train_cams, test_cams, extent, HB.TRAINED_PRESETS[name]["train_iters"])), flush=True)
        del model, train_cams, test_cams
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
