#!/usr/bin/env python
"""Timing of the image-quality evaluation (METRICS.md): one JSON line per image size.

    python scripts/metrics_bench.py [--sizes 800x800,1060x1600] [--repeat 3]

Seeded weights (tests/metrics_scenes.py), random image pairs.  Per size: ms for the preparation, each of the 13 convolutions, the pools,
the taps and the PSNR / SSIM part (LPIPS's `timings`: device events around every stage, the last of `repeat` runs); TFLOP/s from the
algorithmic count 2 * 9 * C_in * C_out * H * W per layer per image, and that as a fraction of the f32-input MFMA peak (157.3 TFLOP/s);
then the same stack (NCHW fp32) through torch.nn.functional.conv2d / max_pool2d on the device in the same process, as the yardstick.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def torch_stack(x2, convs, biases, M):
    """ms per convolution and per pool of the same 13 layers on a [2, 3, H, W] batch"""
    ms, x = {}, x2
    for k, (w, b) in enumerate(zip(convs, biases)):
        x, t = timed(lambda: F.relu(F.conv2d(x, w, b, padding=1)))
        ms["conv%d" % k] = t
        if k in M.POOL_AFTER:
            x, t = timed(lambda: F.max_pool2d(x, 2, 2))
            ms["pool"] = ms.get("pool", 0.0) + t
    return ms


def run(dev, H, W, repeat, yardstick=True):
    import metrics_scenes as S
    import surfel_metrics as M
    convs, biases, lins = ([torch.from_numpy(t) for t in ts] for ts in S.weights())
    crit = M.LPIPS(M.lpips_weights_from_tensors(convs, biases, lins), dev, budget_bytes=64 << 30)
    g = torch.Generator().manual_seed(1)
    x = torch.rand((3, H, W), generator=g).to(dev)
    y = (x * 0.9 + 0.05 * torch.rand((3, H, W), generator=g).to(dev)).clamp(0, 1)
    for _ in range(repeat):
        crit.timings = {}
        value = float(crit(x, y))
        ms = crit.timings
    crit.timings = None
    _, ms_plain = timed(lambda: crit(x, y))      # no per-stage synchronisation
    for _ in range(repeat):
        _, ms_psnr = timed(lambda: M.psnr(x[None], y[None]))
        _, ms_ssim = timed(lambda: M.ssim(x[None], y[None]))
    flops, h, w = {}, H, W
    for k, (ci, co) in enumerate(M.CHANNELS):
        flops["conv%d" % k] = 2 * (2 * 9 * ci * co * h * w)      # both images
        if k in M.POOL_AFTER:
            h, w = h // 2, w // 2
    conv_ms = sum(ms["conv%d" % k] for k in range(13))
    total_flop = sum(flops.values())
    line = {"H": H, "W": W, "lpips": value, "workspace_bytes": M.workspace_bytes(H, W, 1 << 40),
            "ms": {k: round(v, 3) for k, v in ms.items()}, "ms_stages_total": round(sum(ms.values()), 3), "ms_lpips_unsynchronised": round(ms_plain, 3),
            "ms_psnr": round(ms_psnr, 3), "ms_ssim": round(ms_ssim, 3),
            "tflops": {k: round(flops[k] / ms[k] * 1e-9, 2) for k in flops}, "conv_ms": round(conv_ms, 3),
            "conv_tflops": round(total_flop / conv_ms * 1e-9, 2), "conv_fraction_of_f32_mfma_peak": round(total_flop / conv_ms * 1e-9 / PEAK_TFLOPS, 3)}
    if yardstick:
        tw = [(w_.to(dev), b_.to(dev)) for w_, b_ in zip(convs, biases)]
        x2 = torch.stack([x, y])
        for _ in range(repeat):
            tms = torch_stack(x2, [a for a, _ in tw], [b for _, b in tw], M)
        torch_conv_ms = sum(tms["conv%d" % k] for k in range(13))
        line.update({"torch_ms": {k: round(v, 3) for k, v in tms.items()}, "torch_conv_ms": round(torch_conv_ms, 3),
                     "torch_conv_tflops": round(total_flop / torch_conv_ms * 1e-9, 2), "ours_over_torch": round(conv_ms / torch_conv_ms, 3)})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="800x800,1060x1600", help="HxW,...")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch yardstick (its first convolutions may spend minutes choosing kernels)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for s in args.sizes.split(","):
        H, W = (int(v) for v in s.split("x"))
        run(dev, H, W, args.repeat, not args.no_torch)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
