"""What the training log costs (LOG.md): the same synthetic training with and without the event writer, in alternating windows of one
Trainer — each round is without / with / with / without, so a drift of the step time that is linear over a round (the model keeps
training: its frames grow) cancels in the round's difference —, the host's time inside one append, and the time of one report panel
(conversion + PNG encode on the device + the compressed bytes to the host).  Prints one JSON line.
Usage: python scripts/log_bench.py [--workload C2] [--steps 150] [--rounds 8] [--block 256]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd")); sys.path.insert(0, REPO)
import surfel_log as SL  # noqa: E402
import surfel_png  # noqa: E402
from helpers_bench import make_trainer  # noqa: E402
from surfel_render import render  # noqa: E402


def window(tr, steps):
    """ms per step of `steps` steps: a host clock around work that ends in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--slots", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tr = make_trainer(dev, args.workload)
    logdir = tempfile.mkdtemp(prefix="log_bench_")
    writer = SL.EventWriter(logdir, block=args.block, slots=args.slots)
    for logger in (None, writer):      # warm both forms: code objects, allocator blocks, the writer's pinned slots
        tr.logger = logger
        window(tr, 60)
    without, with_log, delta = [], [], []
    for _ in range(args.rounds):       # without, with, with, without
        ms = []
        for logger in (None, writer, writer, None):
            tr.logger = logger
            if logger is not None:
                logger.mark()      # (the steps of the windows without the writer are no part of its next block)
            ms.append(window(tr, args.steps))
        without += [ms[0], ms[3]]
        with_log += [ms[1], ms[2]]
        delta.append(((ms[1] + ms[2]) - (ms[0] + ms[3])) / 2)
    tr.logger = None
    # the host's share of an append: the enqueue alone, no wait inside the window
    scalars = tr.last["scalars"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(1000):
        writer.append(tr.iteration, tr.last["points"], scalars, 0.05, 1000.0)
    append_host_us = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    writer.close()
    events = SL.read_events(writer.path)
    # one report panel: the map -> 8-bit pixels -> PNG on the device, then exactly the file's bytes to the host
    cam = tr.cams[0]
    with torch.no_grad():
        pkg = render(cam, tr.model, tr.pipe, tr.background)
        per_panel = {}
        for label, key, mode in SL.PANELS:
            times = []
            for _ in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pix = SL.panel(mode, pkg[key])
                buf, size = surfel_png.encode_png(pix)
                nbytes = len(buf[:int(size.item())].cpu().numpy().tobytes())
                times.append((time.perf_counter() - t0) * 1e3)
            per_panel[label] = {"ms": round(statistics.median(times[1:]), 4), "png_bytes": nbytes}
    a, b = statistics.median(without), statistics.median(with_log)
    print(json.dumps({
        "workload": args.workload, "height": int(cam.image_height), "width": int(cam.image_width), "points": int(tr.model.P),
        "steps_per_window": args.steps, "rounds": args.rounds, "block": args.block, "slots": args.slots,
        "ms_per_step_without": round(a, 5), "ms_per_step_with": round(b, 5),
        "delta_us_per_step": round(statistics.median(delta) * 1e3, 3), "delta_us_per_round": [round(x * 1e3, 3) for x in delta],
        "append_host_us": round(append_host_us, 3),
        "windows_without": [round(x, 5) for x in without], "windows_with": [round(x, 5) for x in with_log],
        "stalls": writer.stalls, "logged_steps": writer.steps, "events_read_back": len(events), "bytes_written": writer.bytes_written,
        "bytes_per_step": round(writer.bytes_written / max(writer.steps, 1), 1),
        "ms_per_report_panel": round(statistics.mean(v["ms"] for v in per_panel.values()), 4), "panels": per_panel}))


if __name__ == "__main__":
    main()
