#!/usr/bin/env python
"""Guard pages around the undistortion kernel (tests/guard_run.py helpers): source and result each end EXACTLY at the end of their
mapping, with unmapped address space behind them, and the sources start at every offset mod 4.  The cases put invalid pixels on all
four sides, taps on the source's last column and row, and coordinates that are NaN or infinite; the kernel's validity test is the only
thing between those and a read outside the source.  Results are compared with tests/undistort_oracle.py to the byte.

    python tests/undistort_guard_run.py        (one process; driven by tests/test_gpu_undistort.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from scene_guard_run import alloc_end, download, upload_end
import scene_scenes as SS
import undistort_oracle as UO


def case(lib, H, W, Cn, q, pinhole, size, tag):
    vp = C.c_void_p
    src = SS.noise_image(11 + W + Cn, H, W, Cn)
    src[src == 0] = 1
    want, valid = UO.undistort(src, q, pinhole, size, return_valid=True)
    d_src, d_dst = upload_end(src), alloc_end(size[0] * size[1] * Cn)
    qa, pa = (C.c_double * 12)(*[float(v) for v in q]), (C.c_double * 4)(*[float(v) for v in pinhole])
    rc = lib.surfel_scene_undistort(H, W, Cn, size[1], size[0], qa, pa, vp(d_src), vp(d_dst), None)
    assert rc == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after the undistortion")
    assert np.array_equal(download(d_dst, (size[1], size[0], Cn), np.uint8), want), tag
    print("ok %s: %dx%dx%d -> %dx%d, %d invalid, source at %d mod 4" % (tag, H, W, Cn, size[1], size[0], int((~valid).sum()), d_src % 4), flush=True)
    return valid


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    for W in (53, 54, 55, 56):              # 37 x W x 3 bytes ending at the end of the mapping: the source starts at 1, 2, 3, 0 mod 4
        q = UO.distortion_params("SIMPLE_RADIAL", (60, W / 2.0, 18.5, -0.08))
        # wider than the valid region: invalid pixels on all four sides, taps on the last column and the last row
        valid = case(lib, 37, W, 3, q, (60.0, 60.0, (W + 23) / 2.0, 29.0), (W + 23, 58), "forced wide")
        assert not valid[0].any() and not valid[-1].any() and not valid[:, 0].any() and not valid[:, -1].any() and valid.any()
        W2, H2, fx, fy, cx2, cy2 = UO.undistorted_camera(q, W, 37)
        assert case(lib, 37, W, 3, q, (fx, fy, cx2, cy2), (W2, H2), "blank 0").all()
    for Cn in (1, 4):
        q = UO.distortion_params("OPENCV", (61.25, 60.5, 26.2, 18.9, -0.15, 0.05, 0.002, -0.003))
        case(lib, 37, 53, Cn, q, (61.25, 60.5, 40.0, 30.0), (81, 59), "forced wide")
    # coordinates that overflow: NaN (infinite over infinite) and infinite; every pixel is invalid and nothing is read
    for k3, k6, tag in ((1e300, 1e300, "nan"), (1e300, 0.0, "inf")):
        q = UO.distortion_params("FULL_OPENCV", (60, 60, 26.5, 18.5, 0.1, 0, 0, 0, k3, 0, 0, k6))
        assert not case(lib, 37, 53, 3, q, (1e-3, 1e-3, -10.0, -10.0), (70, 9), tag).any()
    # a source one pixel wide has no pair of columns to blend: all invalid
    q = UO.distortion_params("SIMPLE_RADIAL", (60, 0.5, 16.5, 0.01))
    assert not case(lib, 33, 1, 3, q, (60.0, 60.0, 0.5, 16.5), (3, 33), "one column").any()


if __name__ == "__main__":
    main()
