#!/usr/bin/env python
"""Timing of the live viewer's frame path (VIEWER.md): one JSON line per render mode at 1280 x 720 on a synthetic state.

    python scripts/view_bench.py [--surfels 200000] [--width 1280] [--height 720] [--repeat 50] [--warmup 10] [--frames 200]

Per mode: ms of the render (device events, the median of `repeat` after `warmup`), ms of surfel_view.net_image (the same way, and
`net_image_ms_stream`: the host clock around `frames` back-to-back calls that end in one synchronise, divided by `frames` — what a
launch-bound call costs in a stream of them), ms of the non-blocking copy of the finished bytes into pinned memory (events), frames per
second of the three together as Viewer.serve runs them (render, net_image, copy, one event wait per frame; host clock over `frames`
frames), and beside them the reference's way on the same device and the same render package: its op chain written with torch ops
(conv2d per channel, sqrt, norm, min / max, round, gather, clamp, byte, permute, .cpu(); host clock per frame, since .cpu() blocks)
and the frames per second with that chain in the place of net_image + copy.  `bytes_equal_torch_chain`: the share of bytes on which the
two agree (the chain sums its convolutions in another order: VIEWER.md).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def event_ms(fn, repeat, warmup):
    """median device time of fn() by events"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def host_ms(fn, frames, warmup):
    """host clock around `frames` calls and one synchronise, per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(frames):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / frames


class TorchChain:
    """utils/image_utils.py:23-61 and train.py:156 as torch ops on the package's device"""

    def __init__(self, dev):
        import path_oracle as PO
        self.sobel_x = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], device=dev).float()[None, None] / 4
        self.sobel_y = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], device=dev).float()[None, None] / 4
        self.colors = torch.from_numpy(PO.turbo_table().astype("float32") / 255).to(dev)      # (the bytes of the table: the same colours after * 255 and byte())

    def gradient_map(self, image):
        gx = torch.cat([F.conv2d(image[i].unsqueeze(0), self.sobel_x, padding=1) for i in range(image.shape[0])])
        gy = torch.cat([F.conv2d(image[i].unsqueeze(0), self.sobel_y, padding=1) for i in range(image.shape[0])])
        return torch.sqrt(gx ** 2 + gy ** 2).norm(dim=0, keepdim=True)

    def colormap(self, m):
        m = (m - m.min()) / (m.max() - m.min())
        m = (m * 255).round().long().squeeze()
        return self.colors[m].permute(2, 0, 1)

    def __call__(self, pkg, name):
        if name == "Alpha":
            img = pkg["rend_alpha"]
        elif name == "Normal":
            img = (pkg["rend_normal"] + 1) / 2
        elif name == "Depth":
            img = pkg["surf_depth"]
        elif name == "Edge":
            img = self.gradient_map(pkg["render"])
        elif name == "Curvature":
            img = self.gradient_map((pkg["rend_normal"] + 1) / 2)
        else:
            img = pkg["render"]
        if img.shape[0] == 1:
            img = self.colormap(img)
        return (torch.clamp(img, min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous().cpu()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfels", type=int, default=200_000)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=200)
    args = ap.parse_args(argv)
    if args.repeat < 20:
        ap.error("--repeat must be at least 20 (a median of fewer says little)")
    import surfel_trainer as TR
    import surfel_view as SV
    from surfel_render import render
    dev = torch.device("cuda:0")
    W, H = args.width, args.height
    model = TR.synthetic_object(args.surfels, dev, seed=0, px_scale=0.02)
    cam = TR.orbit_cameras(1, W, H, device=dev)[0]
    pipe, bg = TR.pipeline_params(), torch.zeros(3, device=dev)
    viewer = SV.Viewer(listener=False)
    chain = TorchChain(dev)
    out8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    pinned = torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True)
    with torch.no_grad():
        pkg = render(cam, model, pipe, bg)
        render_ms = event_ms(lambda: render(cam, model, pipe, bg), args.repeat, args.warmup)
        copy_ms = event_ms(lambda: pinned.copy_(out8, non_blocking=True), args.repeat, args.warmup)
        for mode, name in enumerate(SV.RENDER_ITEMS):
            def ours():
                return viewer._to_host(SV.net_image(render(cam, model, pipe, bg), mode))

            def theirs():
                return chain(render(cam, model, pipe, bg), name)
            line = {"mode": name, "size": "%dx%d" % (W, H), "surfels": int(model.P), "alpha_coverage": round(float((pkg["rend_alpha"] > 0.5).float().mean()), 3),
                    "render_ms": round(render_ms, 4),
                    "net_image_ms": round(event_ms(lambda: SV.net_image(pkg, mode, out=out8), args.repeat, args.warmup), 4),
                    "net_image_ms_stream": round(host_ms(lambda: SV.net_image(pkg, mode, out=out8), args.frames, args.warmup), 4),
                    "copy_ms": round(copy_ms, 4)}
            line["frame_ms"] = round(host_ms(ours, args.frames, args.warmup), 4)
            line["fps"] = round(1e3 / line["frame_ms"], 1)
            line["torch_chain_ms"] = round(host_ms(lambda: chain(pkg, name), args.frames, args.warmup), 4)
            line["torch_chain_frame_ms"] = round(host_ms(theirs, args.frames, args.warmup), 4)
            line["torch_chain_fps"] = round(1e3 / line["torch_chain_frame_ms"], 1)
            a, b = SV.net_image(pkg, mode).cpu(), chain(pkg, name)
            line["bytes_equal_torch_chain"] = round(float((a == b).float().mean()), 6)
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
