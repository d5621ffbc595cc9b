#!/usr/bin/env python
"""Guard pages around the buffers of include/surfel_cull.h (tests/guard_run.py helpers): the vertices, the triangles, the cameras, the
queue scratch, the depth images and the counts each end EXACTLY at the end of their mapping, with unmapped address space behind them,
on the scene of tests/cull_scenes.py at its odd size — the out-of-range indices, the NaN vertex, the whole-image box and the clamped
boxes at the image border all run next to the guard.  Results are compared with tests/cull_oracle.py.

    python tests/cull_guard_run.py        (one process: a fault kills it; driven by tests/test_gpu_cull.py)
"""
import ctypes as C

import numpy as np

from guard_run import chk, hip, n, torch
from path_guard_run import alloc_end, download, upload_end
import cull_oracle as O
import cull_scenes as S

vp = C.c_void_p


def main():
    torch.cuda.init(); torch.zeros(1, device="cuda:0")
    lib = n.load()
    ref = O.scene_reference(S.FIXTURE_SIZE)
    v, t, H, W = ref["verts"], ref["tris"], ref["H"], ref["W"]
    nv = len(ref["w2c"])
    w2c = np.ascontiguousarray(ref["w2c"][:, :3, :].reshape(nv, 12), np.float32)
    intr = np.asarray([ref["intr"]], np.float32)
    taken = []

    def alloc(user, size):
        taken.append(size)
        return alloc_end(size)

    cb = n.ALLOC_FN(alloc)
    pv, pt, pw, pk = upload_end(v), upload_end(t), upload_end(w2c), upload_end(intr)
    depth = alloc_end(4 * nv * H * W)
    for small in (-1, 0, 1 << 30):
        rc = lib.surfel_cull_mesh_depth(cb, None, len(v), len(t), vp(pv), vp(pt), nv, vp(pw), vp(pk), 1, H, W, S.SCENE["znear"], S.SCENE["zfar"], small,
                                        vp(depth), None, None)
        assert rc == 0, n.last_error()
        chk(hip.hipDeviceSynchronize(), "sync after cull_mesh_depth")
        got = download(depth, (nv, H, W), np.float32)
        ok = ~ref["und"]
        assert np.array_equal((got > 0)[ok], (ref["d64"] > 0)[ok]), small
        hit = ok & (ref["d64"] > 0)
        assert np.max(np.abs(got[hit] - ref["d64"][hit]) / ref["d64"][hit]) <= 4 * ref["deviation"], small
        print("ok depth %dx%dx%d small_pixels %d, scratch %d B, depth ends at %d mod 16" % (nv, H, W, small, taken[-1], (depth + 4 * nv * H * W) % 16), flush=True)
    counts = upload_end(np.zeros(len(v), np.int32))
    assert lib.surfel_cull_visibility(len(v), vp(pv), nv, vp(pw), vp(pk), 1, H, W, vp(depth), S.SCENE["eps"], vp(counts), None) == 0, n.last_error()
    chk(hip.hipDeviceSynchronize(), "sync after cull_visibility")
    c = download(counts, (len(v),), np.int32)
    m = O.point_masks(v, got, ref["w2c"], ref["intr"], S.SCENE["eps"], 20)
    clear = ~m["undecided_pairs"].any(0)
    assert np.array_equal(c[clear], m["counts"][clear]) and clear.mean() > 0.98
    print("ok visibility %d points, counts end at %d mod 16" % (len(v), (counts + 4 * len(v)) % 16), flush=True)


if __name__ == "__main__":
    main()
