#!/usr/bin/env python
"""Guard pages around the JPEG decoder of include/surfel_jpegdec.h (tests/guard_run.py and tests/path_guard_run.py helpers): the file's
bytes, the scratch at exactly surfel_jpegdec_scratch_bytes, the output pixels and the status word each end EXACTLY at the end of their
mapping, with unmapped address space behind them — the byte loads at the file's last byte, the two-word reads at the end of the clean
stream, the scans' tiles and the plane stores all run next to a guard.  Valid files only, at odd file offsets mod 4.  The pixels are
compared with Pillow's, the status word with tests/jpegdec_oracle.py.

    python tests/jpegdec_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_jpegdec.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from path_guard_run import alloc_end, download, upload_end
import jpegdec_oracle as JO
import jpegdec_scenes as JS
import surfel_jpegdec as JD

vp = C.c_void_p
CODES = {"ok": 0, "not converged": 1, "damaged": 2}


def decode_case(lib, name, bits, pad):
    data = JS.jpeg(name) + bytes(pad)      # (bytes behind EOI move the file's first byte to another offset mod 4)
    desc = JD.parse(data)
    want = JS.pixels(name)
    _, info = JO.decode(data, bits, JD.MAX_ROUNDS_DEFAULT)
    nscratch = lib.surfel_jpegdec_scratch_bytes(C.byref(desc.c), bits)
    assert nscratch > 0 and nscratch % 16 == 0
    src, dst, scratch, status = upload_end(np.frombuffer(data, np.uint8)), alloc_end(want.size), alloc_end(nscratch), alloc_end(16)
    rc = lib.surfel_jpegdec_decode(C.byref(desc.c), vp(src), len(data), vp(dst), vp(scratch), nscratch, bits, JD.MAX_ROUNDS_DEFAULT, JD.ALL_STAGES,
                                   vp(status), None)
    assert rc == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after jpegdec_decode")
    st = [int(v) for v in download(status, (4,), np.int32)]
    assert st == [CODES[info["status"]], info["rounds"], info["subsequences"], info["blocks"]] and st[0] == 0, (name, bits, st, info)
    assert np.array_equal(download(dst, want.shape, np.uint8), want), (name, bits)
    print("ok jpegdec %s at %d bits: %d bytes at %d mod 4, pixels at %d mod 4, %d rounds" % (name, bits, len(data), src % 4, dst % 4, st[1]), flush=True)


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    for k, name in enumerate(("rgb-33x17-420", "rgb-17x33-420", "rgb-40x56-422-q90", "rgb-40x56-444-q100", "gray-40x56", "rgb-40x56-420-blocks2",
                              "noise-64x64-q100", "rgb-1x1-420")):
        for bits in (128, 1024):
            decode_case(lib, name, bits, (-len(JS.jpeg(name)) - 1 - 2 * (k % 2)) % 4)      # the file starts at 1 or 3 mod 4


if __name__ == "__main__":
    main()
