#!/usr/bin/env python
"""Timing of the PNG encoder (PNG.md): one JSON line per case.

    python scripts/png_bench.py [--frames 240] [--repeat 30] [--warmup 5] [--cases trained,garden] [--workers 4]

Cases: the trained 800 x 800 state and the garden 1600 x 1060 state of helpers_bench (trained in the same process, untimed), frame 0's
colour frame of the elliptical path.  Per case:
  png_ms            device time of one surfel_png_encode (the memset and all seven launches; output, size word and scratch reused),
                    by events, the median of `repeat` after `warmup`
  png_MBps_in       that time against the 3 bytes per pixel it reads
  png_bytes         the file's length; png_decodes: Pillow opens it to exactly the frame
  pillow_bytes, pillow_ms   the same frame through Image.save(..., "PNG") on one host thread (a host clock, the median of `repeat`)
  path_fps_pillow, path_fps_device   surfel_path.render_path's per-frame files (colour PNG, depth TIFF, turbo PNG) end to end, files on
                    disk included, the second pass of each arm in this process; the Pillow arm is the default
  encode_wait_ms_pillow, encode_wait_ms_device   per frame: the time submit() waited for a free slot plus the time close() waited for
                    the writers, as scripts/path_bench.py computes it
  path_MB_on_disk_pillow, path_MB_on_disk_device
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from path_bench import event_ms, folder_bytes  # noqa: E402


def case(dev, preset, frames, repeat, warmup, workers):
    from PIL import Image
    import helpers_bench as HB
    import surfel_path as SP
    import surfel_png as SG
    import surfel_trainer as TR
    from surfel_render import render
    model, cams, _, _, info = HB.trained_state(dev, preset)
    pipe, bg = TR.pipeline_params(depth_ratio=1.0), torch.zeros(3, device=dev)
    traj = SP.generate_path(cams, n_frames=frames)
    H, W = traj[0].image_height, traj[0].image_width
    out = {"case": "%s %dx%d, %d surfels, %d path frames" % (preset, W, H, int(model.P), frames), "workers": workers}
    with torch.no_grad():
        rgb8 = SP.quantize_u8(render(traj[0], model, pipe, bg)["render"].contiguous())
        buf, size = SG.encode_png(rgb8)
        scratch = torch.empty(SG.scratch_bytes(H, W, 3), dtype=torch.uint8, device=dev)
        out["png_ms"] = round(event_ms(lambda: SG.encode_png(rgb8, out=buf, scratch=scratch, size=size), repeat, warmup), 4)
        out["png_MBps_in"] = round(3 * H * W / out["png_ms"] / 1e3, 1)
        n = int(size.item())
        out["png_bytes"] = n
        host = rgb8.cpu().numpy()
        out["png_decodes"] = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(buf[:n].cpu().numpy().tobytes()))), host))
        del buf, scratch
        ms = []
        for _ in range(repeat):
            f = io.BytesIO()
            t = time.perf_counter()
            Image.fromarray(host).save(f, "PNG")
            ms.append((time.perf_counter() - t) * 1e3)
        out["pillow_ms"] = round(statistics.median(ms), 3)
        out["pillow_bytes"] = len(f.getvalue())
        out["bytes_vs_pillow"] = round(n / out["pillow_bytes"], 4)
        tmp = tempfile.mkdtemp(prefix="png_bench_")
        try:
            for mode in ("pillow", "device"):
                for name in ("warm", "timed"):      # (the first pass pins the ring, starts the threads, sizes the device buffers)
                    info_p = {}
                    shutil.rmtree(os.path.join(tmp, mode), ignore_errors=True)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    SP.render_path(model, cams, render, pipe, bg, os.path.join(tmp, mode), n_frames=frames, workers=workers, timings=info_p, png=mode)
                    torch.cuda.synchronize()
                    total = (time.perf_counter() - t) * 1e3
                out["path_fps_" + mode] = round(frames / total * 1e3, 2)
                out["path_total_ms_per_frame_" + mode] = round(total / frames, 3)
                out["path_loop_ms_per_frame_" + mode] = round(info_p["loop_ms"] / frames, 3)
                out["encode_wait_ms_" + mode] = round((info_p["submit_wait_ms"] + total - info_p["loop_ms"]) / frames, 3)
                out["path_MB_on_disk_" + mode] = round(folder_bytes(os.path.join(tmp, mode)) / 1e6, 1)
            same = all(np.array_equal(np.asarray(Image.open(os.path.join(tmp, "pillow", folder, "%05d.png" % k))),
                                      np.asarray(Image.open(os.path.join(tmp, "device", folder, "%05d.png" % k))))
                       for k in (0, frames // 2, frames - 1) for folder in ("renders", os.path.join("video", "depth")))
            out["path_frames_equal"] = bool(same)
            out["path_speedup"] = round(out["path_fps_device"] / out["path_fps_pillow"], 2)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    out["state"] = {k: info[k] for k in ("train_wall_s", "psnr_heldout") if k in info}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--cases", default="trained,garden")
    args = ap.parse_args(argv)
    if args.repeat < 20:
        ap.error("--repeat must be at least 20 (a median of fewer says little)")
    dev = torch.device("cuda:0")
    for preset in args.cases.split(","):
        print(json.dumps(case(dev, preset, args.frames, args.repeat, args.warmup, args.workers)), flush=True)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
