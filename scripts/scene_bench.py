#!/usr/bin/env python
"""Timing of the capture loader's image path (SCENE.md): one JSON line per case.

    python scripts/scene_bench.py [--repeat 30] [--warmup 5]

Cases: 1200 x 1600 -> 600 x 800 RGB (a DTU frame at -r 2), 3361 x 5187 -> 1036 x 1600 RGB (a Mip-NeRF360 garden frame at -r -1) and the
800 x 800 RGBA composite (a NeRF-synthetic frame).  Per case: ms of the upload of the decoded bytes and of each kernel (device events
around the call, the median of `repeat` after `warmup`), GB/s against the bytes each moves (source bytes read once + result bytes written;
the taps' re-reads are cache traffic and not counted), the device-to-device copy rate of this device measured in the same process (the
bound a kernel that moves those bytes once could reach), and beside them the same image through the reference's host path on this host:
PIL.resize + torch.from_numpy(...) / 255 + .cuda() (the composite case: the fp64 numpy composite of scene/dataset_readers.py:204-210).
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

import numpy as np  # noqa: E402
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


def host_ms(fn, repeat):
    """median wall time of fn(), which ends synchronised"""
    ms = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def gbps(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)


def copy_rate(dev, repeat, warmup):
    """GB/s (read + write) of a 256 MiB device-to-device copy: the HBM rate a bytes-moved bound is stated against"""
    a = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    return gbps(2 * a.numel(), event_ms(lambda: b.copy_(a), repeat, warmup))


def resize_case(SC, dev, H, W, H2, W2, repeat, warmup, hbm):
    import surfel_native as n
    from PIL import Image
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    pinned = torch.from_numpy(src).pin_memory()
    d = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    out = {"case": "%dx%d->%dx%d RGB" % (H, W, H2, W2), "hbm_copy_GBps": hbm}
    out["upload_ms"] = round(event_ms(lambda: d.copy_(pinned, non_blocking=True), repeat, warmup), 4)
    out["upload_GBps"] = gbps(src.nbytes, out["upload_ms"])
    kh, bh, ch = SC._device_tables(W, W2, dev)
    kv, bv, cv = SC._device_tables(H, H2, dev)
    mid = torch.empty((H, W2, 3), dtype=torch.uint8, device=dev)
    planes = torch.empty((3, H2, W2), dtype=torch.float32, device=dev)
    out["ksize"] = [kh, kv]
    out["h_ms"] = round(event_ms(lambda: n.call(dev, "surfel_scene_resample_h", H, W, 3, W2, kh, d, bh, ch, mid, None, None), repeat, warmup), 4)
    out["v_ms"] = round(event_ms(lambda: n.call(dev, "surfel_scene_resample_v", H, W2, 3, H2, kv, mid, bv, cv, None, planes, None), repeat, warmup), 4)
    h_bytes, v_bytes = src.nbytes + mid.numel(), mid.numel() + 4 * planes.numel()
    out["h_GBps"], out["v_GBps"] = gbps(h_bytes, out["h_ms"]), gbps(v_bytes, out["v_ms"])
    out["kernels_ms"] = round(out["h_ms"] + out["v_ms"], 4)
    out["bytes_bound_ms"] = round((h_bytes + v_bytes) / (hbm * 1e6), 4)
    out["load_image_ms"] = round(event_ms(lambda: SC.load_image(d, (W2, H2)), repeat, warmup), 4)      # both passes + their allocations
    # the reference's path on this host
    pil = Image.fromarray(src)
    out["pil_resize_ms"] = round(host_ms(lambda: pil.resize((W2, H2)), max(3, repeat // 5)), 3)

    def reference():
        t = (torch.from_numpy(np.array(pil.resize((W2, H2)))) / 255.0).permute(2, 0, 1).to(dev)
        torch.cuda.synchronize()
        return t
    out["pil_path_ms"] = round(host_ms(reference, max(3, repeat // 5)), 3)
    image, _ = SC.load_image(d, (W2, H2))
    out["equal_to_pil_path"] = bool(torch.equal(image, reference()))
    return out


def composite_case(SC, dev, H, W, repeat, warmup, hbm):
    import surfel_native as n
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    pinned = torch.from_numpy(src).pin_memory()
    d = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    planes = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    out = {"case": "%dx%d RGBA composite" % (H, W), "hbm_copy_GBps": hbm}
    out["upload_ms"] = round(event_ms(lambda: d.copy_(pinned, non_blocking=True), repeat, warmup), 4)
    out["upload_GBps"] = gbps(src.nbytes, out["upload_ms"])
    out["composite_ms"] = round(event_ms(lambda: n.call(dev, "surfel_scene_composite", H, W, 1, d, rgb), repeat, warmup), 4)
    out["to_float_ms"] = round(event_ms(lambda: n.call(dev, "surfel_scene_to_float", H, W, 3, rgb, planes, None), repeat, warmup), 4)
    c_bytes, f_bytes = src.nbytes + rgb.numel(), rgb.numel() + 4 * planes.numel()
    out["composite_GBps"], out["to_float_GBps"] = gbps(c_bytes, out["composite_ms"]), gbps(f_bytes, out["to_float_ms"])
    out["kernels_ms"] = round(out["composite_ms"] + out["to_float_ms"], 4)
    out["bytes_bound_ms"] = round((c_bytes + f_bytes) / (hbm * 1e6), 4)

    def reference():
        norm = src / 255.0
        arr = norm[:, :, :3] * norm[:, :, 3:4] + np.array([1, 1, 1]) * (1 - norm[:, :, 3:4])
        u8 = np.array(arr * 255.0, dtype=np.byte).view(np.uint8)
        t = (torch.from_numpy(u8) / 255.0).permute(2, 0, 1).to(dev)
        torch.cuda.synchronize()
        return t
    out["numpy_path_ms"] = round(host_ms(reference, max(3, repeat // 5)), 3)
    n.call(dev, "surfel_scene_composite", H, W, 1, d, rgb)
    n.call(dev, "surfel_scene_to_float", H, W, 3, rgb, planes, None)
    out["equal_to_numpy_path"] = bool(torch.equal(planes, reference()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    if args.repeat < 20:
        ap.error("--repeat must be at least 20 (a median of fewer says little)")
    import surfel_scene as SC
    dev = torch.device("cuda:0")
    hbm = copy_rate(dev, args.repeat, args.warmup)
    for H, W, H2, W2 in ((1200, 1600, 600, 800), (3361, 5187, 1036, 1600)):
        print(json.dumps(resize_case(SC, dev, H, W, H2, W2, args.repeat, args.warmup, hbm)), flush=True)
    print(json.dumps(composite_case(SC, dev, 800, 800, args.repeat, args.warmup, hbm)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
