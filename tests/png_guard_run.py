#!/usr/bin/env python
"""Guard pages around the PNG encoder of include/surfel_png.h (tests/guard_run.py and tests/path_guard_run.py helpers): the input
frame, the output at exactly surfel_png_capacity, the scratch at exactly surfel_png_scratch_bytes and the size word each end EXACTLY
at the end of their mapping, with unmapped address space behind them — the byte loads at the last pixel, the bit buffers' dword
traffic at the end of the scratch and the byte stores of the compaction all run next to a guard.  A noise frame fills the output
closest to its capacity, a constant one is all matches.  The files are compared with tests/png_oracle.py.

    python tests/png_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_png.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from path_guard_run import alloc_end, download, upload_end
import png_oracle as PO

vp = C.c_void_p


def encode_case(lib, name, img):
    H, W, Cn = img.shape
    cap, nscratch = lib.surfel_png_capacity(H, W, Cn), lib.surfel_png_scratch_bytes(H, W, Cn)
    assert cap == PO.capacity(H, W, Cn) and nscratch > 0 and nscratch % 16 == 0
    src, dst, scratch, size = upload_end(img), alloc_end(cap), alloc_end(nscratch), alloc_end(8)
    assert lib.surfel_png_encode(H, W, Cn, vp(src), vp(dst), cap, vp(size), vp(scratch), nscratch, None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after png_encode")
    want = PO.encode(img)
    got_size = int(download(size, (1,), np.int64)[0])
    assert got_size == len(want), (name, H, W, Cn, got_size, len(want))
    assert download(dst, (got_size,), np.uint8).tobytes() == want, (name, H, W, Cn)
    print("ok png %s %dx%dx%d: %d bytes of %d, pixels at %d mod 4, file at %d mod 4" % (name, H, W, Cn, got_size, cap, src % 4, dst % 4), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    rng = np.random.default_rng(3)
    encode_case(lib, "noise", rng.integers(0, 256, size=(17, 33, 3), dtype=np.uint8))
    encode_case(lib, "noise", rng.integers(0, 256, size=(35, 1001, 1), dtype=np.uint8))      # two stripes, the last of two rows
    encode_case(lib, "constant", np.full((5, 300, 1), 113, np.uint8))
    encode_case(lib, "constant", np.full((23, 501, 3), 255, np.uint8))                       # two stripes of matches


if __name__ == "__main__":
    main()
