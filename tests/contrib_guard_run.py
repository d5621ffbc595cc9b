#!/usr/bin/env python
"""Overrun hunt for the contribution pass, in the manner of tests/guard_run.py (whose guarded allocator and Frame it uses): the six
accumulator arrays and dominant_id end exactly at the end of their mapped pages with unmapped address space behind them, and the slack
in front of each (the start of its mapping) holds a byte pattern that must survive.  A write past an array faults, a write in front of
it shows in the pattern.

    python tests/contrib_guard_run.py          (driven by tests/test_gpu_contrib.py; a fault kills the process)
"""
import ctypes as C
import sys

import numpy as np

import guard_run as G      # (initialises HIP's virtual-memory API for device 0 at import)

n, hip, chk = G.n, G.hip, G.chk
PATTERN = 0xA5


def patterned(nbytes):
    """a guarded array of nbytes zero bytes; returns (pointer, start of its mapping, slack bytes in front)"""
    p = G.guard_alloc(nbytes)
    va, _, size = G.keep[-1]
    chk(hip.hipMemset(va, PATTERN, C.c_size_t(size)), "memset pattern")
    chk(hip.hipMemset(C.c_void_p(p), 0, C.c_size_t(max(nbytes, 1))), "memset zero")
    return p, va.value, p - va.value


def slack_intact(start, slack):
    if slack == 0:
        return True
    h = np.empty(slack, np.uint8)
    chk(hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(start), C.c_size_t(slack), 2), "D2H")
    return bool((h == PATTERN).all())


def read(p, count, dtype):
    h = np.empty(count, dtype)
    chk(hip.hipMemcpy(h.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(h.nbytes), 2), "D2H")
    return h


def run(lib, P, W, H, rad, **kw):
    fr = G.Frame(lib, P, W, H, rad, **kw)
    R = fr.forward(n.OPT_EXACT_BINNING | n.OPT_NO_STREAM)
    chk(hip.hipDeviceSynchronize(), "sync after forward")
    sizes = [8 * P, 8 * P, 4 * P, 4 * P, 4 * P, 4 * P, 4 * W * H]      # sum_q, hits, max_bits, dominant, views, stamp, dominant_id
    arrs = [patterned(s) for s in sizes]
    vp = C.c_void_p
    for tag in (1, 2):
        rc = lib.surfel_rasterize_contribution(P, R, W, H, vp(fr.bufs["geom"][0]), vp(fr.bufs["bin"][0]), vp(fr.bufs["img"][0]), tag,
                                               *[vp(a[0]) for a in arrs], 0, None)
        assert rc == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after the contribution pass")
    assert all(slack_intact(a[1], a[2]) for a in arrs), "bytes in front of an array were written"
    hits, views, dom = read(arrs[1][0], P, np.uint64), read(arrs[4][0], P, np.uint32), read(arrs[6][0], W * H, np.int32)
    assert hits.sum() > 0 and views.max() == 2 and dom.min() >= -1 and dom.max() < P
    print("P=%d %dx%d ok: R=%d pairs=%d granularity=%d" % (P, W, H, R, int(hits.sum()) // 2, G.G), flush=True)


def main():
    G.torch.cuda.init(); G.torch.zeros(1, device="cuda:0")
    lib = n.load()
    run(lib, 3000, 200, 120, 4.0)                                                    # partial tiles on both edges, short lists
    run(lib, 20000, 80, 64, 6.0, seed=12, opacity=0.015, z_near=1.0, z_far=9.0)      # lists of several staging batches
    return 0


if __name__ == "__main__":
    sys.exit(main())
