#!/usr/bin/env python
"""Guard pages around the capture loader's kernels (tests/guard_run.py helpers): source, intermediate, tables and outputs each end exactly
EXACTLY at the end of their mapping, with unmapped address space behind them; the sources start at every offset mod 4, so the
horizontal pass's byte-wise head and tail are exercised.  Results are compared with tests/scene_oracle.py to the byte.

    python tests/scene_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_scene.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, guard_alloc, hip, n, torch
import scene_oracle as SO
import scene_scenes as SS
import surfel_scene


def download(p, shape, dtype):
    a = np.empty(shape, dtype)
    chk(hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(a.nbytes), 2), "D2H")
    return a


def alloc_end(nbytes):
    """device pointer whose nbytes end EXACTLY at the end of the mapping (guard_alloc rounds the size up to 16 and returns the start of that)"""
    return guard_alloc(nbytes) + (-int(nbytes)) % 16


def upload_end(arr):
    a = np.ascontiguousarray(arr)
    p = alloc_end(a.nbytes)
    chk(hip.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1), "H2D")
    return p


def tables(i, o):
    ksize, bounds, coeffs = surfel_scene.resample_tables(i, o)
    return ksize, upload_end(bounds), upload_end(coeffs)


def case(lib, H, W, Cn, H2, W2):
    vp = C.c_void_p
    src = SS.noise_image(7 + W, H, W, Cn)
    want, mid = SO.resize(src, W2, H2)
    planes_want, mask_want = SO.to_float(want)
    d_src = upload_end(src)
    d_planes, d_mask = alloc_end(4 * min(Cn, 3) * H2 * W2), (alloc_end(4 * H2 * W2) if Cn == 4 else None)
    cur, curW = d_src, W
    if W2 != W:
        k, b, c = tables(W, W2)
        last = H2 == H
        d_mid = None if last else alloc_end(H * W2 * Cn)
        rc = lib.surfel_scene_resample_h(H, W, Cn, W2, k, vp(cur), vp(b), vp(c), vp(d_mid) if d_mid else None, vp(d_planes), vp(d_mask) if d_mask else None, None)
        assert rc == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after the horizontal pass")
        if not last:
            assert np.array_equal(download(d_mid, (H, W2, Cn), np.uint8), mid)
            cur, curW = d_mid, W2
    if H2 != H:
        k, b, c = tables(H, H2)
        rc = lib.surfel_scene_resample_v(H, curW, Cn, H2, k, vp(cur), vp(b), vp(c), None, vp(d_planes), vp(d_mask) if d_mask else None, None)
        assert rc == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after the vertical pass")
    assert np.array_equal(download(d_planes, planes_want.shape, np.float32), planes_want)
    if Cn == 4:
        assert np.array_equal(download(d_mask, mask_want.shape, np.float32), mask_want)
        # the composite and the conversion alone, on the same guarded source
        d_rgb = alloc_end(H * W * 3)
        assert lib.surfel_scene_composite(H, W, 1, vp(d_src), vp(d_rgb), None) == 0, n.last_error()
        d_f = alloc_end(4 * 3 * H * W)
        assert lib.surfel_scene_to_float(H, W, 3, vp(d_rgb), vp(d_f), None, None) == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after composite + to_float")
        rgb = SO.composite(src, True)
        assert np.array_equal(download(d_rgb, (H, W, 3), np.uint8), rgb) and np.array_equal(download(d_f, (3, H, W), np.float32), SO.to_float(rgb)[0])
    print("ok %dx%dx%d -> %dx%d, source at %d mod 4" % (H, W, Cn, H2, W2, d_src % 4), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    for W in (53, 54, 55, 56):              # 37 x W x 3 bytes ending at the end of the mapping: the source starts at 1, 2, 3, 0 mod 4
        case(lib, 37, W, 3, 13, 20)
    case(lib, 33, 1, 1, 7, 1)
    case(lib, 33, 1, 3, 7, 1)
    case(lib, 37, 53, 4, 13, 20)
    case(lib, 17, 19, 3, 17, 9)             # horizontal pass only, float output straight from it
    case(lib, 9, 301, 3, 5, 300)            # more than one strip of 64 columns, ragged last strip


if __name__ == "__main__":
    main()
