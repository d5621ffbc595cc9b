#!/usr/bin/env python
"""Guard pages around the frame kernels of include/surfel_vis.h (tests/guard_run.py helpers): inputs, scratch and outputs each end
EXACTLY at the end of their mapping, with unmapped address space behind them, at the odd shapes of tests/test_gpu_path.py — so the
float inputs start at every 4-byte offset of a 16-byte line and the byte outputs at every offset mod 4, and the 16-byte loads, the
dword stores and their byte-wise heads and tails all run next to the guard.  Results are compared with tests/path_oracle.py.

    python tests/path_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_path.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, guard_alloc, hip, n, torch
import path_oracle as PO
import path_scenes as PS

vp = C.c_void_p


def download(p, shape, dtype):
    a = np.empty(shape, dtype)
    chk(hip.hipMemcpy(a.ctypes.data_as(vp), vp(p), C.c_size_t(a.nbytes), 2), "D2H")
    return a


def alloc_end(nbytes):
    """device pointer whose nbytes end EXACTLY at the end of the mapping (guard_alloc rounds the size up to 16 and returns the start of that)"""
    return guard_alloc(nbytes) + (-int(nbytes)) % 16


def upload_end(arr):
    a = np.ascontiguousarray(arr)
    p = alloc_end(a.nbytes)
    chk(hip.hipMemcpy(vp(p), a.ctypes.data_as(vp), C.c_size_t(a.nbytes), 1), "H2D")
    return p


def quantize_case(lib, Cn, H, W):
    for seed, (scale, bias) in enumerate(((1.0, 0.0), (0.5, 0.5))):
        a = PS.frame(60 + seed, Cn, H, W, normal=bias != 0.0)
        src, dst = upload_end(a), alloc_end(H * W * Cn)
        assert lib.surfel_vis_quantize(Cn, H, W, vp(src), scale, bias, vp(dst), None) == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after quantize")
        assert np.array_equal(download(dst, (H, W, Cn), np.uint8), PO.quantize(a, scale, bias)), (Cn, H, W, scale)
    print("ok quantize %dx%dx%d, planes at %d mod 16, pixels at %d mod 4" % (Cn, H, W, src % 16, dst % 4), flush=True)


def order_case(lib, count):
    x = PS.order_data("mixed", count, seed=9)
    ranks = PS.order_ranks(count)
    src, out, scratch = upload_end(x), alloc_end(4 * len(ranks)), alloc_end(8448)
    arr = (C.c_int64 * len(ranks))(*ranks)
    assert lib.surfel_vis_order_stats(count, vp(src), len(ranks), arr, vp(out), vp(scratch), 8448, None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after order_stats")
    got, want = download(out, (len(ranks),), np.float32), PO.order_stats(x, ranks)
    assert np.all(got == want), (count, got, want)
    print("ok order_stats n = %d, data at %d mod 16" % (count, src % 16), flush=True)


def turbo_case(lib, H, W):
    d = PS.depth_frame(H + W, H, W, zero_frac=0.009)
    with np.errstate(divide="ignore"):
        lo, hi = np.log(np.percentile(d, [3, 97]))
    src, dst = upload_end(d), alloc_end(H * W * 3)
    assert lib.surfel_vis_depth_turbo(H, W, vp(src), float(lo), float(hi), vp(dst), None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after depth_turbo")
    got = download(dst, (H, W, 3), np.uint8).astype(np.int64)
    tab = PO.turbo_table().astype(np.int64)
    code = {int(c): k for k, c in enumerate(tab[:, 0] | tab[:, 1] << 8 | tab[:, 2] << 16)}
    gb = np.vectorize(lambda c: code.get(c, -1000))(got[..., 0] | got[..., 1] << 8 | got[..., 2] << 16)
    idx, black = PO.turbo_index(d, lo, hi)
    assert not black.any() and np.abs(gb - idx).max() <= 1 and int((gb != idx).sum()) <= max(2, int(0.001 * H * W)), (H, W)
    print("ok depth_turbo %dx%d, depth at %d mod 16, pixels at %d mod 4" % (H, W, src % 16, dst % 4), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    for shape in ((3, 1, 1), (3, 5, 7), (1, 3, 129), (3, 33, 65), (3, 16, 260)):
        quantize_case(lib, *shape)
    for count in (1, 65, 257, 4097):
        order_case(lib, count)
    for H, W in ((37, 53), (48, 80)):
        turbo_case(lib, H, W)


if __name__ == "__main__":
    main()
