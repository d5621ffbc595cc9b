#!/usr/bin/env python
"""Guard pages around the JPEG encoder of include/surfel_jpeg.h (tests/guard_run.py and tests/path_guard_run.py helpers): the input
frame, the output at exactly surfel_jpeg_capacity, the scratch at exactly surfel_jpeg_scratch_bytes and the size word each end
EXACTLY at the end of their mapping, with unmapped address space behind them — the byte loads at the last pixel, the row buffers' dword
traffic at the end of the scratch and the byte stores of the compaction all run next to a guard.  The files are compared with
tests/video_oracle.py.

    python tests/video_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_video.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from path_guard_run import alloc_end, download, upload_end
import video_oracle as VO
import video_scenes as VS

vp = C.c_void_p


def encode_case(lib, name, H, W, quality):
    img = VS.content(name, H, W, seed=3)
    cap, nscratch = lib.surfel_jpeg_capacity(H, W), lib.surfel_jpeg_scratch_bytes(H, W)
    assert cap == VO.capacity(H, W) and nscratch > 0
    src, dst, scratch, size = upload_end(img), alloc_end(cap), alloc_end(nscratch), alloc_end(8)
    assert lib.surfel_jpeg_encode(H, W, vp(src), quality, vp(dst), cap, vp(size), vp(scratch), nscratch, None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after jpeg_encode")
    want = VO.encode(img, quality)
    got_size = int(download(size, (1,), np.int64)[0])
    assert got_size == len(want), (name, H, W, got_size, len(want))
    assert download(dst, (got_size,), np.uint8).tobytes() == want, (name, H, W)
    print("ok jpeg %s %dx%d q%d: %d bytes of %d, pixels at %d mod 4, file at %d mod 4" % (name, H, W, quality, got_size, cap, src % 4, dst % 4), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    encode_case(lib, "edges", 17, 33, 95)
    encode_case(lib, "noise", 17, 33, 100)
    encode_case(lib, "noise", 16, 1040, 100)
    encode_case(lib, "checker", 16, 1040, 75)


if __name__ == "__main__":
    main()
