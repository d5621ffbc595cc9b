#!/usr/bin/env python
"""Timing of the undistortion kernel (UNDISTORT.md): one JSON line per case.

    python scripts/undistort_bench.py [--repeat 20] [--warmup 3] [--cases opencv-1600x1200,simple_radial-5187x3361] [--limit 300]

Cases: a 1600 x 1200 RGB image of an OPENCV camera and a 5187 x 3361 RGB image of a SIMPLE_RADIAL camera (seeded noise; real
photographs are not part of the repository), each undistorted into the camera the rule gives at blank = 0.  Per case: the kernel's ms
(device events around the launch alone, median of `repeat` after `warmup`), GB/s over (source + result bytes), the device-to-device
copy rate of the same run over the same bytes (a copy of the source plus a copy of the result: what moving those bytes costs with no
arithmetic), the upload's ms, and the ms of the numpy restatement (tests/undistort_oracle.py) on this host, whose bytes the kernel's
result must equal.  Every case runs in a child process of its own under a time limit (--limit seconds); the first one that fails or
runs out of time ends the run, and nothing more is started on the device.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

CASES = {
    "opencv-1600x1200": ("OPENCV", (1250.0, 1245.0, 802.3, 597.1, -0.2, 0.06, 0.002, -0.003), 1600, 1200),
    "simple_radial-5187x3361": ("SIMPLE_RADIAL", (4100.0, 2593.5, 1680.5, -0.08), 5187, 3361),
}


def event_ms(torch, fn, repeat, warmup):
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


def run_case(name, repeat, warmup):
    import numpy as np
    import torch
    import surfel_undistort as SU
    import undistort_oracle as UO
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench: no HIP device (timings are taken on the GPU only)")
    model, params, W, H = CASES[name]
    q = SU.distortion_params(model, params)
    W2, H2, fx, fy, cx2, cy2 = SU.undistorted_camera(q, W, H)
    pinhole, size = (fx, fy, cx2, cy2), (W2, H2)
    src = np.random.default_rng(7).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    t = time.perf_counter()
    want = UO.undistort(src, q, pinhole, size)
    numpy_ms = (time.perf_counter() - t) * 1e3
    host = torch.from_numpy(src)
    dev_src = host.cuda()
    got = SU.undistort(dev_src, q, pinhole, size)
    assert np.array_equal(got.cpu().numpy(), want), "the device's bytes are not the restatement's"
    nbytes = src.size + want.size
    src_copy, dst_copy = torch.empty_like(dev_src), torch.empty_like(got)

    def copies():
        src_copy.copy_(dev_src)
        dst_copy.copy_(got)
    kernel_ms = event_ms(torch, lambda: SU.undistort(dev_src, q, pinhole, size), repeat, warmup)
    copy_ms = event_ms(torch, copies, repeat, warmup)
    upload_ms = event_ms(torch, lambda: host.cuda(), repeat, warmup)
    return {"case": "%s %dx%d RGB -> %dx%d" % (model, W, H, W2, H2), "source_bytes": int(src.size), "result_bytes": int(want.size),
            "kernel_ms": round(kernel_ms, 4), "kernel_GBps": round(nbytes / kernel_ms / 1e6, 1), "d2d_copy_ms": round(copy_ms, 4),
            "d2d_copy_GBps": round(nbytes / copy_ms / 1e6, 1), "upload_ms": round(upload_ms, 4), "numpy_ms": round(numpy_ms, 1),
            "repeat": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--limit", type=int, default=300, help="seconds each case may take")
    ap.add_argument("--case", default=None, help="(internal) run this one case in this process")
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(args.case, args.repeat, args.warmup)), flush=True)
        return 0
    for name in args.cases.split(","):
        if name not in CASES:
            raise SystemExit("undistort_bench: unknown case %r (known: %s)" % (name, ", ".join(CASES)))
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--repeat", str(args.repeat), "--warmup", str(args.warmup)],
                               timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("undistort_bench: case %s ran out of its %d s; stopping" % (name, args.limit), file=sys.stderr)
            return 124
        if p.returncode != 0:
            print("undistort_bench: case %s failed (%d); stopping" % (name, p.returncode), file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
