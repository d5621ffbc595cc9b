#!/usr/bin/env python
"""Guard pages around the device entries of include/surfel_log.h (tests/guard_run.py and tests/path_guard_run.py helpers): the log
state, the ring, the six scalars, the panel's planes, its destination and its scratch each end EXACTLY at the end of their mapping,
with unmapped address space behind them — the record store into the ring's last slot, the 16-byte loads at the planes' last pixels and
the dword / byte stores at the destination's tail all run next to a guard.  Results are compared with tests/log_oracle.py.

    python tests/log_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_log.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from path_guard_run import alloc_end, download, upload_end
import log_oracle as LO

vp = C.c_void_p


def ring_case(lib, capacity, appends):
    rng = np.random.default_rng(capacity)
    state, ring = upload_end(np.zeros(32, np.uint8)), upload_end(np.zeros(capacity * 32, np.uint8))
    steps = []
    for k in range(appends):
        s = rng.uniform(0, 1, size=6).astype(np.float32)
        steps.append((k + 1, 1000 + k, s, 0.05 if k % 3 else 0.0, 100.0))
        scalars = upload_end(s)      # 24 bytes, ending at the guard
        assert lib.surfel_log_append(vp(state), vp(ring), capacity, k + 1, 1000 + k, vp(scalars), 0.05 if k % 3 else 0.0, 100.0, None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after log_append")
    want = LO.records(steps)
    got = download(ring, (capacity,), LO.RECORD)
    for k in range(max(0, appends - capacity), appends):
        assert got[k % capacity].tobytes() == want[k].tobytes(), (capacity, k, got[k % capacity], want[k])
    st = download(state, (4,), np.int64)
    assert int(st[2]) == appends
    print("ok ring capacity %d, %d appends, last slot written: %s" % (capacity, appends, appends >= capacity), flush=True)


def panel_case(lib, mode, H, W):
    rng = np.random.default_rng(H * 131 + W)
    Cn = 3 if mode in ("rgb", "normal") else 1
    x = rng.normal(0.5, 0.6, size=(Cn, H, W)).astype(np.float32)
    if H * W > 4:
        x[0, H // 2, W // 3] = np.nan
    src, dst, scratch = upload_end(x), alloc_end(H * W * 3), alloc_end(64)
    code = {"rgb": 0, "gray": 1, "normal": 2, "turbo_max": 3, "jet_minmax": 4}[mode]
    assert lib.surfel_log_panel(code, H, W, vp(src), vp(dst), vp(scratch), 64, None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after log_panel")
    assert np.array_equal(download(dst, (H, W, 3), np.uint8), LO.panel(mode, x)), (mode, H, W)
    print("ok panel %s %dx%d, planes at %d mod 16, pixels at %d mod 4" % (mode, H, W, src % 16, dst % 4), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    ring_case(lib, 8, 19)
    ring_case(lib, 1, 3)
    for mode in ("rgb", "gray", "normal", "turbo_max", "jet_minmax"):
        for H, W in ((1, 1), (37, 53), (64, 65)):
            panel_case(lib, mode, H, W)


if __name__ == "__main__":
    main()
