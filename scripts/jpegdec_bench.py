#!/usr/bin/env python
"""Timing of the device JPEG decoder against Pillow on this host (JPEGDEC.md): one JSON line per case.

    python scripts/jpegdec_bench.py [--repeat 10] [--warmup 2] [--cases 1600x1200,5187x3361]

Cases: a 1600 x 1200 and a 5187 x 3361 synthetic "photo" (smooth ramp plus noise, 4:2:0, quality 92, Pillow's encoder; real photographs
are not part of the repository).  Per case: the file's bytes, ms of its upload, ms of every decoder stage (device events around a call
that runs that stage alone, in the scratch the stages before it left), the rounds used, and the wall time of a whole decode_jpeg
(read from memory, parse, upload, decode, the status word's wait).  Beside them Pillow's decode of the same file on this host: one
thread, and 8 threads decoding 16 files (per file).  Then the wall time of load_cameras on a folder of 16 such files, decode="host"
with 8 workers against decode="device".  All figures are medians of `repeat` after `warmup`.
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import jpegdec_scenes as JS  # noqa: E402
import scene_scenes as SS  # noqa: E402
import surfel_jpegdec as JD  # noqa: E402
import surfel_scene as SC  # noqa: E402


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


def host_ms(fn, repeat, warmup):
    """median wall time of fn(), which ends synchronised"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def pillow_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im)


def write_folder(root, data, w, h, count):
    """a COLMAP text model of `count` cameras that share one PINHOLE camera, every image the same file"""
    sparse = os.path.join(root, "sparse", "0")
    os.makedirs(sparse)
    os.makedirs(os.path.join(root, "images"))
    with open(os.path.join(sparse, "cameras.txt"), "w") as f:
        f.write("1 PINHOLE %d %d %r %r %r %r\n" % (w, h, 1.2 * w, 1.2 * w, w / 2.0, h / 2.0))
    with open(os.path.join(sparse, "images.txt"), "w") as f:
        for k in range(count):
            name = "%03d.jpg" % k
            with open(os.path.join(root, "images", name), "wb") as g:
                g.write(data)
            ang = 2 * np.pi * k / count
            R, t = SS.look_at_w2c((3.0 * float(np.cos(ang)), 0.2, 3.0 * float(np.sin(ang))))
            f.write("%d %s 1 %s\n\n" % (k + 1, " ".join(repr(float(v)) for v in list(SS.rotmat_to_qvec(R)) + list(t)), name))
    with open(os.path.join(sparse, "points3D.txt"), "w") as f:
        for p in range(8):
            f.write("%d %r %r %r 128 128 128 0.5 1 0\n" % (p + 1, 0.1 * p, -0.05 * p, 0.02 * p))
    return root


def run_case(w, h, repeat, warmup, dev):
    data = JS.photo(50, h, w, quality=92)
    desc = JD.parse(data)
    want = pillow_decode(data)
    got = JD.decode_jpeg(data, dev)
    info = JD.decode_info()
    assert np.array_equal(got.cpu().numpy(), want), "the device's pixels are not Pillow's"
    out = {"case": "%dx%d 4:2:0 q92" % (w, h), "file_bytes": len(data), "decoded_bytes": int(want.size), "rounds": info["rounds"],
           "subsequences": info["subsequences"], "blocks": info["blocks"], "max_rounds": JD.MAX_ROUNDS_DEFAULT,
           "scratch_bytes": JD.scratch_bytes(desc)}
    host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    out["upload_ms"] = round(event_ms(lambda: host.to(dev), repeat, warmup), 4)
    file = JD.upload(data, dev)
    pixels, status, scratch = JD.launch(desc, file)
    stages = {}
    for k, name in enumerate(JD.STAGE_NAMES):      # (in order: every stage finds what the stages before it left in the scratch)
        stages[name] = round(event_ms(lambda: JD.launch(desc, file, stages=1 << k, out=pixels, scratch=scratch, status=status), repeat, warmup), 4)
    out["stage_ms"] = stages
    out["decode_device_ms"] = round(event_ms(lambda: JD.launch(desc, file, out=pixels, scratch=scratch, status=status), repeat, warmup), 4)
    out["decode_jpeg_wall_ms"] = round(host_ms(lambda: JD.decode_jpeg(data, dev), repeat, warmup), 3)
    out["pillow_1_thread_ms"] = round(host_ms(lambda: pillow_decode(data), repeat, warmup), 3)
    with ThreadPoolExecutor(8) as pool:
        out["pillow_8_threads_16_files_ms_per_file"] = round(host_ms(lambda: list(pool.map(pillow_decode, [data] * 16)), repeat, warmup) / 16, 3)
    with tempfile.TemporaryDirectory() as tmp:
        infos = SC.read_scene_info(write_folder(os.path.join(tmp, "capture"), data, w, h, 16)).train_cameras

        def load(mode):
            cams = SC.load_cameras(infos, workers=8, data_device=dev, decode=mode)
            torch.cuda.synchronize()
            return cams
        a, b = load("host"), load("device")
        assert all(bool((x.original_image == y.original_image).all()) for x, y in zip(a, b)), "load_cameras: device != host"
        del a, b
        out["load_cameras_16_host_8_workers_ms"] = round(host_ms(lambda: load("host"), repeat, warmup), 2)
        out["load_cameras_16_device_ms"] = round(host_ms(lambda: load("device"), repeat, warmup), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="1600x1200,5187x3361")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpegdec_bench: no HIP device (timings are taken on the GPU only)")
    dev = "cuda:0"
    for case in args.cases.split(","):
        w, h = (int(v) for v in case.split("x"))
        print(json.dumps(run_case(w, h, args.repeat, args.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
