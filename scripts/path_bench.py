#!/usr/bin/env python
"""Timing of the trajectory renderer (RENDER.md): one JSON line per case.

    python scripts/path_bench.py [--frames 240] [--repeat 30] [--warmup 5] [--cases trained,garden] [--workers 4]

Cases: the trained 800 x 800 state and the garden 1600 x 1060 state of helpers_bench (trained in the same process, untimed).  Per case:
ms per frame of the render, of the three frame kernels (device events around the call, the median of `repeat` after `warmup`, on frame
0's maps), of the device-to-host copies of one frame's files and of the waits for the encoders; GB/s of the two conversion kernels
against the bytes each moves (planes read once + pixels written) beside the device-to-device copy rate of this device measured in the
same process; end-to-end frames per second of surfel_path.render_path, files on disk included; and the same path cameras exported the
parent's way in the same process: GaussianExtractor.reconstruction() + export_image() (every fp32 frame kept on the device, copied to the
host as fp32, quantised in numpy, encoded on one thread).  The two ways write different files per frame (render_path: colour PNG, depth
TIFF, turbo PNG; export_image: colour PNG, ground-truth PNG); both lists are in the line.
The video path (VIDEO.md) beside them: jpeg_ms, the device time of one surfel_jpeg_encode of frame 0's colour frame at quality 95 (all
its launches, scratch from the caching allocator), jpeg_MBps_in against the 3 bytes per pixel it reads, jpeg_bytes, the file's size,
and video_fps, the same loop with video_only=True and three streams (colour, depth, normal; no per-frame file), AVI files on disk
included.
"""
import argparse
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

import torch  # noqa: E402


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


def gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)


def folder_bytes(root):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, files in os.walk(root) for f in files)


def case(dev, preset, frames, repeat, warmup, workers, hbm):
    import helpers_bench as HB
    import surfel_mesh
    import surfel_path as SP
    import surfel_trainer as TR
    from surfel_render import render
    model, cams, _, _, info = HB.trained_state(dev, preset)
    pipe, bg = TR.pipeline_params(depth_ratio=1.0), torch.zeros(3, device=dev)
    traj = SP.generate_path(cams, n_frames=frames)
    H, W = traj[0].image_height, traj[0].image_width
    out = {"case": "%s %dx%d, %d surfels, %d path frames" % (preset, W, H, int(model.P), frames), "hbm_copy_GBps": hbm, "workers": workers}
    with torch.no_grad():
        # ---- stages, on their own
        def render_all():
            for cam in traj:
                render(cam, model, pipe, bg)
        render_all()                      # every view's buffer sizes seen once
        torch.cuda.synchronize()
        t = time.perf_counter()
        render_all()
        torch.cuda.synchronize()
        out["render_ms"] = round((time.perf_counter() - t) * 1e3 / frames, 4)
        pkg = render(traj[0], model, pipe, bg)
        rgb, depth = pkg["render"].contiguous(), pkg["surf_depth"][0].contiguous()
        hw = H * W
        rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        out["quantize_ms"] = round(event_ms(lambda: SP.quantize_u8(rgb, out=rgb8), repeat, warmup), 4)
        out["quantize_GBps"] = gbps(15 * hw, out["quantize_ms"])
        ranks = SP.percentile_ranks(hw, [3, 97])[0]
        out["select_ms"] = round(event_ms(lambda: SP.order_stats(depth, ranks), repeat, warmup), 4)
        out["select_ranks"] = len(ranks)
        limits = SP.depth_limits(depth)
        out["depth_limits_frame0"] = [repr(v) for v in limits]
        # (a frame that is more than 3 % empty has lo = -inf and comes out black; the kernel is timed with limits that index the table)
        lo, hi = limits if limits[0] > -float("inf") and limits[1] > limits[0] else (0.0, 2.0)
        out["colorize_ms"] = round(event_ms(lambda: SP.colorize_depth(depth, lo, hi, out=rgb8), repeat, warmup), 4)
        out["colorize_GBps"] = gbps(7 * hw, out["colorize_ms"])
        import surfel_video as SV
        SP.quantize_u8(rgb, out=rgb8)
        jbuf, jsize = SV.encode_jpeg(rgb8)
        out["jpeg_ms"] = round(event_ms(lambda: SV.encode_jpeg(rgb8, out=jbuf, size=jsize), repeat, warmup), 4)
        out["jpeg_MBps_in"] = round(3 * hw / out["jpeg_ms"] / 1e3, 1)
        out["jpeg_bytes"] = int(jsize.item())
        del jbuf
        pin8, pin32 = torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True), torch.empty((H, W), dtype=torch.float32, pin_memory=True)

        def copies():                     # one frame's files: colour, turbo (3 B / pixel each), depth (4 B / pixel)
            pin8.copy_(rgb8, non_blocking=True)
            pin8.copy_(rgb8, non_blocking=True)
            pin32.copy_(depth, non_blocking=True)
        out["copy_ms"] = round(event_ms(copies, repeat, warmup), 4)
        out["copy_GBps"] = gbps(10 * hw, out["copy_ms"])
        pin_f = torch.empty((3, H, W), dtype=torch.float32, pin_memory=True)
        out["copy_fp32_rgb_ms"] = round(event_ms(lambda: pin_f.copy_(rgb, non_blocking=True), repeat, warmup), 4)      # what the parent's way moves per colour frame
        # ---- end to end
        tmp = tempfile.mkdtemp(prefix="path_bench_")
        try:
            for name in ("warm", "timed"):      # (the first pass pins the ring and starts the threads)
                info_p = {}
                torch.cuda.synchronize()
                t = time.perf_counter()
                SP.render_path(model, cams, render, pipe, bg, os.path.join(tmp, name), n_frames=frames, workers=workers, timings=info_p)
                torch.cuda.synchronize()
                total = (time.perf_counter() - t) * 1e3
            out["path_total_ms_per_frame"] = round(total / frames, 3)
            out["path_fps"] = round(frames / total * 1e3, 2)
            out["path_loop_ms_per_frame"] = round(info_p["loop_ms"] / frames, 3)
            out["encode_wait_ms"] = round((info_p["submit_wait_ms"] + total - info_p["loop_ms"]) / frames, 3)
            out["path_files_per_frame"] = ["renders/*.png", "vis/depth_*.tiff", "video/depth/*.png"]
            out["path_MB_on_disk"] = round(folder_bytes(os.path.join(tmp, "timed")) / 1e6, 1)
            for name in ("video_warm", "video_timed"):
                info_v = {}
                torch.cuda.synchronize()
                t = time.perf_counter()
                SP.render_path(model, cams, render, pipe, bg, os.path.join(tmp, name), n_frames=frames, vis_normals=True, video_only=True, timings=info_v)
                torch.cuda.synchronize()
                total_v = (time.perf_counter() - t) * 1e3
            out["video_fps"] = round(frames / total_v * 1e3, 2)
            out["video_loop_ms_per_frame"] = round(info_v["loop_ms"] / frames, 3)
            out["video_wait_ms"] = round(info_v["video_wait_ms"] / frames, 3)
            out["video_files"] = ["render_traj_color.avi", "render_traj_depth.avi", "render_traj_normal.avi"]
            out["video_MB_on_disk"] = round(folder_bytes(os.path.join(tmp, "video_timed")) / 1e6, 1)
            # ---- the parent's way, same cameras
            ext = surfel_mesh.GaussianExtractor(model, render, pipe)
            torch.cuda.synchronize()
            t = time.perf_counter()
            ext.reconstruction(traj)
            torch.cuda.synchronize()
            t_rec = (time.perf_counter() - t) * 1e3
            held = sum(x.numel() * 4 for x in ext.rgbmaps + ext.depthmaps)
            t = time.perf_counter()
            ext.export_image(os.path.join(tmp, "parent"))
            t_exp = (time.perf_counter() - t) * 1e3
            out["parent_reconstruction_ms_per_frame"] = round(t_rec / frames, 3)
            out["parent_export_ms_per_frame"] = round(t_exp / frames, 3)
            out["parent_fps"] = round(frames / (t_rec + t_exp) * 1e3, 2)
            out["parent_frames_held_GB"] = round(held / 1e9, 2)
            out["parent_files_per_frame"] = ["renders/*.png", "gt/*.png"]
            out["parent_MB_on_disk"] = round(folder_bytes(os.path.join(tmp, "parent")) / 1e6, 1)
            from PIL import Image
            import numpy as np
            same = all(np.array_equal(np.asarray(Image.open(os.path.join(tmp, "timed", "renders", "%05d.png" % k))),
                                      np.asarray(Image.open(os.path.join(tmp, "parent", "renders", "%05d.png" % k)))) for k in (0, frames // 2, frames - 1))
            out["renders_equal_to_parent"] = bool(same)
            out["speedup_vs_parent"] = round(out["path_fps"] / out["parent_fps"], 2)
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
    import helpers_bench as HB
    dev = torch.device("cuda:0")
    hbm = HB.copy_bandwidth(dev)["GBps_read_plus_write"]
    for preset in args.cases.split(","):
        print(json.dumps(case(dev, preset, args.frames, args.repeat, args.warmup, args.workers, hbm)), flush=True)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
