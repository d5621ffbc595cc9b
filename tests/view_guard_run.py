#!/usr/bin/env python
"""Guard pages around the viewer's image kernels of include/surfel_view.h (tests/guard_run.py helpers): inputs, scratch and outputs
each end EXACTLY at the end of their mapping, with unmapped address space behind them, at the odd shapes of tests/test_gpu_view.py —
so the halo loads of the last tile row and column, the 16-byte loads of the map, the dword stores and their byte-wise heads and tails
all run next to the guard.  Results are compared with tests/view_oracle.py.

    python tests/view_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_view.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from path_guard_run import alloc_end, download, upload_end
import view_oracle as VO
import view_scenes as VS

vp = C.c_void_p
SHAPES = ((1, 1), (1, 5), (7, 1), (23, 37), (33, 130))


def check(got, m, what):
    want, t255 = VO.colour(m)
    loose = VO.indeterminate(t255)
    differ = (got != want).any(axis=2)
    assert not (differ & ~loose).any() and loose.mean() <= 0.01, (what, int(differ.sum()), int(loose.sum()))


def scalar_case(lib, H, W):
    m = VS.package(H, W)["surf_depth"][0]
    nbytes = 64 + 4 * H * W
    src, dst, scratch = upload_end(m), alloc_end(H * W * 3), alloc_end(nbytes)
    assert lib.surfel_view_scalar(H, W, vp(src), vp(dst), vp(scratch), nbytes, None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after view_scalar")
    check(download(dst, (H, W, 3), np.uint8), m, ("scalar", H, W))
    print("ok scalar %dx%d, map at %d mod 16, pixels at %d mod 4, scratch at %d mod 16" % (H, W, src % 16, dst % 4, scratch % 16), flush=True)


def gradient_case(lib, H, W):
    pkg = VS.package(H, W)
    nbytes = 64 + 4 * H * W
    for key, scale, bias in (("render", 1.0, 0.0), ("rend_normal", 0.5, 0.5)):
        src, dst, scratch = upload_end(pkg[key]), alloc_end(H * W * 3), alloc_end(nbytes)
        assert lib.surfel_view_gradient(H, W, vp(src), scale, bias, vp(dst), vp(scratch), nbytes, None) == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after view_gradient")
        check(download(dst, (H, W, 3), np.uint8), VO.gradient(pkg[key], scale, bias), (key, H, W))
    print("ok gradient %dx%d, planes at %d mod 16, pixels at %d mod 4, scratch at %d mod 16" % (H, W, src % 16, dst % 4, scratch % 16), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    for H, W in SHAPES:
        scalar_case(lib, H, W)
        gradient_case(lib, H, W)


if __name__ == "__main__":
    main()
