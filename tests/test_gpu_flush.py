"""The per-round flush of blend_bwd (scan walk: csrc/surfel_backward_scan.hip, flush_round; rows walk: the `item` loop of
csrc/surfel_backward.hip) on hand-built 32x32 frames whose first tile holds the cases the flush can get wrong:

  all16    three splats that cover the whole frame: every instance is on all sixteen sub-tile lists (sixteen real slots per flush)
  hidden   a small instance behind eight dense splats that saturate its sub-tile, in front of a deeper one elsewhere in the tile: it is
           staged, lies on no live list and must get an all-zero gradient record (sixteen zero-slot reads)
  chunks   sub-tile lists of 33, 15, 16 and 17 small instances, one list per wave: rank -> round arithmetic over 1, 1, 2 and 3 rounds
  batches  150 small instances, the longest list 16 + 4 with its 17th entry at staged index 100: the first batch of 128 is cut to 100
           (keep < mb), so rounds are flushed on both sides of a batch boundary
  masks    two thin ellipses over five sub-tiles: all four of wave 0 and the first of wave 1 (rows walk: overlap mask 15 and 1)

What a frame holds is derived on the CPU from the fp64 oracle alone (test_frames_hold_their_cases: every surfel rendered by itself gives
the sub-tiles it is composited in) and asserted again on the device from the instrumented kernels' counters, so a frame that stops
exercising its case fails instead of passing by default."""
import functools

import numpy as np
import pytest

from helpers import HipRun, check_grads, oracle_forward, scene_args

W = H = 32
Z0 = 3.0
TINY = (0.5, 0.5, 0.05)      # 1-sigma radii (px), opacity: reaches <= 1.9 px from the centre of its sub-tile, i.e. that sub-tile only
KINDS = ["all16", "hidden", "chunks", "batches", "masks"]


def _frame(splats):
    """splats: (centre x, centre y, sigma x, sigma y, opacity) in pixels, DEEPEST FIRST; discs facing an untilted camera."""
    import synthetic
    cam = synthetic.look_at_camera(W, H)
    f = 1.2 * W
    n = len(splats)
    rng = np.random.default_rng(5)
    z = Z0 - 0.004 * np.arange(n)
    s = np.asarray(splats, np.float64)
    means = np.stack([(s[:, 0] - W / 2 + 0.5) * z / f, (s[:, 1] - H / 2 + 0.5) * z / f, z], 1)
    sh = np.zeros((n, 16, 3), np.float32)
    sh[:, 0] = rng.normal(0.0, 1.0, (n, 3)); sh[:, 1:] = rng.normal(0.0, 0.1, (n, 15, 3))
    sc = dict(means3D=means.astype(np.float32), scales=(s[:, 2:4] * z[:, None] / f).astype(np.float32),
              rotations=np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1)), opacities=s[:, 4:5].astype(np.float32),
              shs=sh, sh_degree=3, bg=np.zeros(3, np.float32), scale_modifier=1.0)
    sc.update(cam)
    return sc


def _tiny(bx, by):
    return (4 * bx + 1.5, 4 * by + 1.5) + TINY


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(scene, expect): expect["lists"] = the sub-tile lists' lengths of tile 0 as a {(bx, by): n} dict (absent: 0)."""
    if kind == "all16":
        return _frame([(7.5 + k, 7.5 - k, 40.0, 40.0, 0.05) for k in range(3)]), dict(lists={(bx, by): 3 for bx in range(4) for by in range(4)})
    if kind == "hidden":
        # deepest first: F (sub-tile (2, 2)), H (the hidden one, sub-tile (0, 0)), eight blockers over sub-tile (0, 0): alpha 0.77 .. 0.8 on its
        # pixels, so T falls below 1e-4 behind the sixth or seventh of them and never comes near the threshold (0.2^5 = 3.2e-4, 0.2^6 = 6.4e-5)
        sp = [_tiny(2, 2), _tiny(0, 0)] + [(1.5, 1.5, 8.0, 8.0, 0.8)] * 8
        return _frame(sp), dict(hidden=1)
    if kind == "chunks":
        want = {(0, 0): 33, (2, 0): 15, (0, 2): 16, (2, 2): 17}
        sp = [_tiny(0, 0)] * 33
        for k in range(17):
            sp += [_tiny(*b) for b in ((2, 0), (0, 2), (2, 2)) if k < want[b]]
        return _frame(sp), dict(lists=want, wave_rounds=3 + 1 + 1 + 2, entries=81)
    if kind == "batches":
        others = [(bx, by) for by in range(4) for bx in range(4) if (bx, by) != (0, 0)]
        sp, k = [], 0
        for t in range(150):
            if t < 16 or 100 <= t < 104:
                sp.append(_tiny(0, 0))
            else:
                sp.append(_tiny(*others[k % 15])); k += 1
        want = {b: 0 for b in others}
        for i in range(130):
            want[others[i % 15]] += 1
        want[(0, 0)] = 20
        # batch one is cut in front of staged instance 100 (one round, four waves), batch two holds the other 50 (one round, four waves);
        # uncut, batch one would take a second round for sub-tile (0, 0): 9 wave rounds
        return _frame(sp), dict(lists=want, wave_rounds=8, entries=150)
    if kind == "masks":
        # alpha >= 1/255 out to 3.11 sigma at opacity 0.5: semi-axes 4 x 2 px around (4.5, 2.3) — pixel rows 0 .. 3: x in [0.5, 8.5] (blocks 0, 1, 2),
        # rows 4 .. 7: x in [2.4, 6.6] (blocks 0, 1)
        sp = [(4.5, 2.3, 4.0 / 3.114, 2.0 / 3.114, 0.5)] * 2
        return _frame(sp), dict(lists={(0, 0): 2, (1, 0): 2, (2, 0): 2, (0, 1): 2, (1, 1): 2}, entries=10)
    raise KeyError(kind)


def _oracle_alone(kind):
    """Per surfel, rendered by itself with the fp64 oracle: the boolean (H, W) map of the pixels it is composited in."""
    from oracle.surfel_oracle import Oracle
    sc, _ = _case(kind)
    o = Oracle("f64")
    maps = []
    for i in range(sc["means3D"].shape[0]):
        one = dict(sc)
        for k in ("means3D", "scales", "rotations", "opacities", "shs"):
            one[k] = np.ascontiguousarray(sc[k][i:i + 1])
        st = oracle_forward(o, scene_args(one))[4]
        maps.append(np.asarray(st.n_contrib[0]) > 0)
    return np.stack(maps)


def _subtiles(m):
    """{(tile, bx, by)} of the 4x4-pixel sub-tiles that hold a set pixel of the (H, W) map m."""
    ys, xs = np.nonzero(m)
    return {((y // 16) * (W // 16) + x // 16, (x % 16) // 4, (y % 16) // 4) for x, y in zip(xs, ys)}


@pytest.mark.parametrize("kind", KINDS)
def test_frames_hold_their_cases(kind):
    """CPU, oracle only: the frames hold the list lengths, the hidden instance and the batch cut they were built for."""
    from oracle.surfel_oracle import Oracle
    sc, ex = _case(kind)
    a = scene_args(sc)
    o = Oracle("f64")
    R, col, oth, radii, st = oracle_forward(o, a)
    final_T = np.asarray(st.final_T[0])
    alone = _oracle_alone(kind)
    n = alone.shape[0]
    subs = [_subtiles(m) for m in alone]
    if "lists" in ex:
        assert final_T.min() > 1e-3          # nothing saturates: composited alone = composited in the frame
        got = {}
        for s in subs:
            for (tile, bx, by) in s:
                if tile == 0:
                    got[(bx, by)] = got.get((bx, by), 0) + 1
        assert got == {b: c for b, c in ex["lists"].items() if c}, got
        if kind != "all16":
            assert all(tile == 0 for s in subs for (tile, _, _) in s)       # the other tiles stay empty: the counters speak of tile 0
    if kind == "all16":
        assert all(len(s) == 16 * 4 for s in subs)                          # every instance on all sixteen lists of every tile
    if kind == "chunks":
        # staged order = deepest first = surfel order; the 33-list's last entry is staged instance 32: 32 x 7 <= 81 x 5, the batch is not cut
        assert [i for i in range(n) if (0, 0, 0) in subs[i]] == list(range(33))
    if kind == "batches":
        on = [i for i in range(n) if (0, 0, 0) in subs[i]]
        assert on[:16] == list(range(16)) and on[16] == 100 and len([i for i in on if i < 128]) == 20
        assert max(c for b, c in ex["lists"].items() if b != (0, 0)) < 16
        assert 100 * (2 * 1 + 3) > 128 * (2 * 1 + 1)                        # the cost rule cuts batch one at keep = 100 < mb = 128
    if kind == "hidden":
        h = ex["hidden"]
        assert subs[h] == {(0, 0, 0)}                                       # alone it is composited, in sub-tile (0, 0) of tile 0 only
        lo, hi = (int(v) for v in st.ranges[0])
        pos = list(st.point_list[lo:hi]).index(h) + 1                       # 1-based, front to back
        last = np.asarray(st.n_contrib[0])
        assert last[:4, :4].max() < pos <= last[:16, :16].max()             # behind the last contributor of its sub-tile, staged by the tile
        gC = np.ones((3, H, W), np.float32); gO = np.ones((7, H, W), np.float32)
        og = o.rasterize_backward(st, gC, gO)
        assert not np.any(og.dL_dmeans3D[h]) and not np.any(og.dL_dopacity[h])
    if kind == "masks":
        # row order (surfel_common.h: thread_pixel): wave 0 = blocks (0..1, 0..1) -> mask 15, wave 1 = blocks (2..3, 0..1), its row 0 = (2, 0) -> mask 1
        assert all(s == {(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (0, 2, 0)} for s in subs)


def _stats(run, flag, gC, gO):
    import torch
    import surfel_native as n
    lib = n.load()
    st = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    try:
        assert lib.surfel_debug_set_blend_stats(n.ptr(st)) == 0
        run.debug = flag
        g = run.backward(gC, gO)
    finally:
        lib.surfel_debug_set_blend_stats(None)
        run.debug = 0
    return st.cpu().numpy().copy(), g


def _same(x, y, what):
    for k in x:
        assert np.isfinite(x[k]).all(), (what, k)
        assert np.array_equal(x[k], y[k]), "%s: dL/d%s differs in %d elements" % (what, k, int((x[k] != y[k]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_flush_cases(kind):
    """(a) scan walk with and without the tile stream: same bits; (b) rows and quad: same bits; (c) every walk twice: same bits;
    (d) every walk meets the oracle bars of the parity tests (helpers.check_grads).  The instrumented kernels (which keep the flush with
    a branch per sub-tile) give the product kernels' bits as well, and their counters show the case: list entries walked
    (stats[3]), wave steps = 16 per (wave, round) with a list entry (stats[2])."""
    import surfel_native as n
    from oracle.surfel_oracle import Oracle
    sc, ex = _case(kind)
    a = scene_args(sc)
    rng = np.random.default_rng(23)
    gC = rng.normal(size=(3, H, W)).astype(np.float32); gO = rng.normal(size=(7, H, W)).astype(np.float32)
    run = HipRun(a).forward()
    res = {}
    for name, flag in (("rows", n.OPT_BWD_ROWS), ("quad", n.OPT_BWD_QUAD), ("scan", n.OPT_BWD_SCAN),
                       ("rows_gather", n.OPT_BWD_ROWS | n.OPT_BWD_GATHER), ("scan_gather", n.OPT_BWD_SCAN | n.OPT_BWD_GATHER)):
        run.debug = flag
        res[name] = run.backward(gC, gO)
        res[name + "/again"] = run.backward(gC, gO)
    run.debug = 0
    _same(res["scan"], res["scan_gather"], kind + ": scan walk, tile stream vs gather")            # (a)
    _same(res["rows"], res["rows_gather"], kind + ": rows walk, tile stream vs gather")
    _same(res["rows"], res["quad"], kind + ": rows vs quad")                                       # (b)
    for name in ("rows", "quad", "scan", "rows_gather", "scan_gather"):                            # (c)
        _same(res[name], res[name + "/again"], kind + ": %s walk, run to run" % name)
    o = Oracle("f64")
    st = oracle_forward(o, a, depth_key=run.depths())[4]
    og = o.rasterize_backward(st, gC, gO)
    for name in ("rows", "quad", "scan"):                                                          # (d)
        check_grads(res[name], og)
    # the cases, from the device's own counters
    s_scan, g_scan = _stats(run, n.OPT_BWD_SCAN, gC, gO)
    s_scan_g, g_scan_g = _stats(run, n.OPT_BWD_SCAN | n.OPT_BWD_GATHER, gC, gO)
    s_rows, g_rows = _stats(run, n.OPT_BWD_ROWS, gC, gO)
    _same(res["scan"], g_scan, kind + ": scan walk, instrumented vs product")
    _same(res["scan"], g_scan_g, kind + ": scan walk (gather), instrumented vs product")
    _same(res["rows"], g_rows, kind + ": rows walk, instrumented vs product")
    print("%s: scan stats %s, rows stats %s" % (kind, s_scan[:4].tolist(), s_rows[:5].tolist()))
    assert s_scan[:4].tolist() == s_scan_g[:4].tolist()
    if kind == "all16":
        assert s_scan[3] == 3 * 16 * 4 and s_rows[3] == 3 * 16 * 4          # three instances on all sixteen lists of all four tiles
    if "entries" in ex:
        assert s_scan[3] == ex["entries"] and s_rows[3] == ex["entries"], (s_scan[3], s_rows[3])
    if "wave_rounds" in ex:
        assert s_scan[2] == 16 * ex["wave_rounds"], s_scan[2]
    if kind == "hidden":
        h = ex["hidden"]
        for name in ("rows", "quad", "scan", "scan_gather"):
            for k in ("means3D", "opacity", "sh", "means2D", "scales", "rots", "transMat", "normal", "colors"):
                assert not np.any(res[name][k][h]), "%s walk: the hidden instance's dL/d%s is not zero" % (name, k)
        # without the hidden instance the walk steps through exactly the same list entries: it is on no live list
        keep = [i for i in range(sc["means3D"].shape[0]) if i != h]
        sc2 = dict(sc)
        for k in ("means3D", "scales", "rotations", "opacities", "shs"):
            sc2[k] = np.ascontiguousarray(sc[k][keep])
        run2 = HipRun(scene_args(sc2)).forward()
        assert run2.R == run.R - 1                                          # ... though the tile lists it (one instance more)
        s2, _ = _stats(run2, n.OPT_BWD_SCAN, gC, gO)
        assert s2[:4].tolist() == s_scan[:4].tolist(), (s2[:4], s_scan[:4])
