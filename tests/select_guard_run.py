#!/usr/bin/env python
"""Overrun hunt for the label pass, in the manner of tests/contrib_guard_run.py (whose helpers it uses, with the guarded allocator and
Frame of tests/guard_run.py): `votes` and the label image end exactly at the end of their mapped pages with unmapped address space
behind them, and the slack in front of each holds a byte pattern that must survive.  The frame is 50 x 37: 1850 label bytes, no multiple
of 4, partial tiles on both edges — a label load past the image's last byte faults, a write in front of `votes` shows in the pattern.

    python tests/select_guard_run.py          (driven by tests/test_gpu_select.py; a fault kills the process)
"""
import ctypes as C
import sys

import numpy as np

import contrib_guard_run as CG      # (initialises HIP's virtual-memory API for device 0 at import, through guard_run)
import select_scenes as S

G, n, hip, chk = CG.G, CG.n, CG.hip, CG.chk


def run(lib, fr, R, K, labels):
    P, W, H = fr.P, fr.W, fr.H
    votes = CG.patterned(8 * P * K)
    assert (8 * P * K) % 16 == 0                       # guard_alloc ends a multiple of 16 bytes at the mapping's end: votes end exactly there
    lab, lab_va, lab_slack = CG.patterned(W * H)
    pad = -(W * H) % 16                                # ... and the label image is moved up so that its last byte is the mapping's last
    lab, lab_slack = lab + pad, lab_slack + pad
    chk(hip.hipMemset(C.c_void_p(lab - pad), CG.PATTERN, C.c_size_t(pad)), "memset pattern")
    a = np.ascontiguousarray(labels, np.uint8)
    assert a.shape == (H, W)
    chk(hip.hipMemcpy(C.c_void_p(lab), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1), "H2D labels")
    vp = C.c_void_p
    for _ in range(2):
        rc = lib.surfel_rasterize_label_votes(P, R, W, H, vp(fr.bufs["geom"][0]), vp(fr.bufs["bin"][0]), vp(fr.bufs["img"][0]), vp(lab), K, vp(votes[0]), 0, None)
        assert rc == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after the label pass")
    assert CG.slack_intact(votes[1], votes[2]) and CG.slack_intact(lab_va, lab_slack), "bytes in front of an array were written"
    assert np.array_equal(CG.read(lab, W * H, np.uint8).reshape(H, W), a), "the label image was written"
    v = CG.read(votes[0], P * K, np.uint64).reshape(P, K)
    used = np.unique(a[a < K])
    assert v.sum() > 0 and v.max() < 2 * W * H * (1 << 24) and not v[:, [k for k in range(K) if k not in used]].any()
    print("P=%d %dx%d K=%d ok: R=%d votes=%d granularity=%d" % (P, W, H, K, R, int(v.sum()) // 2, G.G), flush=True)


def main():
    G.torch.cuda.init(); G.torch.zeros(1, device="cuda:0")
    lib = n.load()
    W, H = 50, 37
    fr = G.Frame(lib, 2000, W, H, 4.0)
    R = fr.forward(n.OPT_EXACT_BINNING | n.OPT_NO_STREAM)
    chk(hip.hipDeviceSynchronize(), "sync after forward")
    run(lib, fr, R, 2, S.checker(W, H, 2))            # every row mixed, the binary bucket
    run(lib, fr, R, 6, S.random(W, H, 5))             # ignored pixels, a label that never occurs, the middle bucket
    run(lib, fr, R, 32, S.blocks4(W, H, 32))          # the widest rows of votes, the large bucket
    return 0


if __name__ == "__main__":
    sys.exit(main())
