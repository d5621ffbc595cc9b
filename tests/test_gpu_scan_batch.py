"""The per-batch bookkeeping of blend_bwd's scan walk (csrc/surfel_backward_scan.hip) on hand-built 32x32 frames whose first tile holds
the cases it can get wrong: every thread (staged instance, half) ranks its instance on the lists of eight sub-tiles (rows 0-7 = waves
0-1 = pixel rows 0 .. 7 of the tile, rows 8-15 = waves 2-3 = pixel rows 8 .. 15), the flush joins the two halves' first / last rounds,
and it skips the four sub-tiles of a wave whose lists ended before the round.

  both_halves     one instance is the 18th entry of a list of the upper half (round 1) and the first entry of a list of the lower
                  half (round 0): its first and last round come from different threads
  high_only       instances on lists of rows 8-15 only: the other half's thread must leave "on no list" (ranks 0xff, rounds 255 | 0)
  low_only        ... and on lists of rows 0-7 only
  rank127         128 small instances on one sub-tile: eight full rounds, rank 127 next to the 0xff marker; the other three waves sit
                  out every round, so every flush skips three groups
  late_idle       lists of 17 on a sub-tile of wave 0 and of 1 on a sub-tile of wave 3, nothing on waves 1-2: 3 wave rounds.  (With 18
                  staged instances the cost rule cuts the batch in front of the 17th entry: waves 0 and 3 walk the first batch's round,
                  wave 0 alone the second batch's.)
  late_idle_deep  the same with 11 on wave 3's sub-tile: 28 staged instances, no cut — waves 0 and 3 walk round 0, only wave 0 round 1
  cut_then_idle   the `batches` construction of test_gpu_flush.py (the first batch of 128 cut to 100) with the second batch's lists all
                  on wave 0: skipping and truncation meet across a batch boundary

What a frame holds is derived on the CPU from the fp64 oracle alone (test_frames_hold_their_cases: every surfel rendered by itself gives
the sub-tiles it is composited in; the batches, rounds and walking waves follow from those lists by the kernel's documented rules) and
asserted again on the device from the instrumented kernel's counters, so a frame that stops exercising its case fails instead of
passing by default."""
import functools

import numpy as np
import pytest

from helpers import HipRun, check_grads, oracle_forward, scene_args

W = H = 32
Z0 = 3.0
TINY = (0.5, 0.5, 0.05)      # 1-sigma radii (px), opacity: stays inside the sub-tile it is centred in
SB, CH = 128, 16             # staged instances per batch, instances per chunk (surfel_backward_scan.hip)
KINDS = ["both_halves", "high_only", "low_only", "rank127", "late_idle", "late_idle_deep", "cut_then_idle"]


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


def _row(bx, by):
    """DPP row (= list index, flush sub-tile) of block (bx, by): wave = the 8x8 quad, row of the wave = the block inside it
    (surfel_common.h: thread_pixel)."""
    return 4 * (((by >> 1) << 1) | (bx >> 1)) + (((by & 1) << 1) | (bx & 1))


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(scene, expect): lists = the sub-tile lists' lengths of tile 0 as {(bx, by): n}; wave_rounds = (wave, round) pairs that walk,
    over all batches; entries = list entries walked; keeps = staged instances walked per batch."""
    if kind == "both_halves":
        # X spans pixel rows 5 .. 10 of column block 0: blocks (0, 1) (row 2, wave 0) and (0, 2) (row 8, wave 2)
        sp = [_tiny(0, 1)] * 17 + [(1.5, 7.5, 0.5, 1.2, 0.05)] + [_tiny(0, 2)] * 2 + [_tiny(3, 3)] * 10
        return _frame(sp), dict(lists={(0, 1): 18, (0, 2): 3, (3, 3): 10}, wave_rounds=2 + 1 + 1, entries=31, keeps=[30], x=17)
    if kind == "high_only":
        # wide splats over blocks (0, 2) and (1, 2) (rows 8, 9), two small ones in block (3, 3) (row 15)
        sp = [(3.5, 9.5, 1.2, 0.5, 0.05)] * 3 + [_tiny(3, 3)] * 2
        return _frame(sp), dict(lists={(0, 2): 3, (1, 2): 3, (3, 3): 2}, wave_rounds=2, entries=8, keeps=[5])
    if kind == "low_only":
        sp = [(3.5, 1.5, 1.2, 0.5, 0.05)] * 3 + [_tiny(3, 1)] * 2
        return _frame(sp), dict(lists={(0, 0): 3, (1, 0): 3, (3, 1): 2}, wave_rounds=2, entries=8, keeps=[5])
    if kind == "rank127":
        return _frame([_tiny(1, 1)] * 128), dict(lists={(1, 1): 128}, wave_rounds=8, entries=128, keeps=[128])
    if kind == "late_idle":
        sp = [_tiny(3, 3)] + [_tiny(0, 0)] * 17
        return _frame(sp), dict(lists={(0, 0): 17, (3, 3): 1}, wave_rounds=3, entries=18, keeps=[17, 1])
    if kind == "late_idle_deep":
        sp = [_tiny(0, 0)] * 17 + [_tiny(3, 3)] * 11
        return _frame(sp), dict(lists={(0, 0): 17, (3, 3): 11}, wave_rounds=3, entries=28, keeps=[28])
    if kind == "cut_then_idle":
        others = [(bx, by) for by in range(4) for bx in range(4) if (bx, by) != (0, 0)]
        wave0 = [(1, 0), (0, 1), (1, 1)]
        sp, want, k = [], {}, 0
        for t in range(150):
            if t < 16 or 100 <= t < 104:
                b = (0, 0)
            elif t < 100:
                b = others[k % 15]; k += 1
            else:
                b = wave0[(t - 104) % 3]
            sp.append(_tiny(*b)); want[b] = want.get(b, 0) + 1
        # batch one is cut in front of staged instance 100 (one round, four waves); batch two holds the other 50: lists of 4, 16, 15, 15 on
        # wave 0's four sub-tiles, nothing on waves 1-3 (one round, one wave)
        return _frame(sp), dict(lists=want, wave_rounds=4 + 1, entries=150, keeps=[100, 50])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
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


def _plan(rows):
    """rows[i] = the set of DPP rows whose list holds instance i of tile 0, deepest first (= staged order).  The walk of the tile by the
    kernel's rules: batches of up to 128 staged instances, a batch cut in front of the instance that opens the longest list's partial
    chunk where (r + 1/2) / ms < (r + 3/2) / mb, chunks of 16, a wave walks a round while one of its four lists has a chunk left.
    -> per batch: dict(keep, lists = [staged indices] per row, ranks = {instance: {row: rank}})."""
    out, start, n = [], 0, len(rows)
    while start < n:
        mb = min(SB, n - start)
        lists = [[t for t in range(mb) if r in rows[start + t]] for r in range(16)]
        nm = max(len(l) for l in lists)
        keep = mb
        full, rem = nm & ~(CH - 1), nm & (CH - 1)
        if full > 0 and rem > 0:
            ms = min(l[full] for l in lists if len(l) > full)
            r = full // CH
            if ms * (2 * r + 3) > mb * (2 * r + 1):
                keep = ms
        lists = [[t for t in l if t < keep] for l in lists]
        ranks = {}
        for r, l in enumerate(lists):
            for k, t in enumerate(l):
                ranks.setdefault(start + t, {})[r] = k
        out.append(dict(keep=keep, lists=lists, ranks=ranks))
        start += keep
    return out


def _wave_rounds(plan):
    return sum(-(-max(len(b["lists"][4 * w + r]) for r in range(4)) // CH) for b in plan for w in range(4))


def _idle_pairs(plan):
    """(wave, round) pairs of a batch's rounds in which the wave walks nothing: the groups the flush skips."""
    return sum(4 * (-(-max(len(l) for l in b["lists"]) // CH)) for b in plan) - _wave_rounds(plan)


@pytest.mark.parametrize("kind", KINDS)
def test_frames_hold_their_cases(kind):
    """CPU, oracle only: the frames hold the lists, the halves, the ranks, the batch cuts and the idle waves they were built for."""
    from oracle.surfel_oracle import Oracle
    sc, ex = _case(kind)
    o = Oracle("f64")
    st = oracle_forward(o, scene_args(sc))[4]
    assert np.asarray(st.final_T[0]).min() > 1e-3            # nothing saturates: composited alone = composited in the frame
    subs = [_subtiles(m) for m in _oracle_alone(kind)]
    n = len(subs)
    assert all(s and all(tile == 0 for (tile, _, _) in s) for s in subs)      # every instance is composited, in tile 0 only
    got = {}
    for s in subs:
        for (_, bx, by) in s:
            got[(bx, by)] = got.get((bx, by), 0) + 1
    assert got == ex["lists"], got
    rows = [{_row(bx, by) for (_, bx, by) in s} for s in subs]
    plan = _plan(rows)
    assert [b["keep"] for b in plan] == ex["keeps"]
    assert _wave_rounds(plan) == ex["wave_rounds"]
    assert sum(len(l) for b in plan for l in b["lists"]) == ex["entries"]
    lo = [any(r < 8 for r in rw) for rw in rows]
    hi = [any(r >= 8 for r in rw) for rw in rows]
    if kind == "both_halves":
        x = ex["x"]
        assert rows[x] == {_row(0, 1), _row(0, 2)} == {2, 8}
        assert plan[0]["ranks"][x] == {2: 17, 8: 0}          # round 1 by its upper half's thread, round 0 by the lower half's
        assert [i for i in range(n) if lo[i] and hi[i]] == [x]
        assert 16 * (2 * 1 + 3) <= 30 * (2 * 1 + 1)          # the cost rule leaves the batch whole
        assert _idle_pairs(plan) == 2 * 4 - 4
    if kind == "high_only":
        assert not any(lo) and all(hi)
        assert max(len(rw) for rw in rows) == 2              # ... on more than one list of that half
        assert _idle_pairs(plan) == 2
    if kind == "low_only":
        assert all(lo) and not any(hi)
        assert max(len(rw) for rw in rows) == 2
        assert _idle_pairs(plan) == 2
    if kind == "rank127":
        assert plan[0]["ranks"][127] == {_row(1, 1): 127} and len(plan) == 1
        assert _idle_pairs(plan) == 8 * 3                    # three groups skipped in each of the eight flushes
    if kind == "late_idle":
        assert {w for b in plan[:1] for w in range(4) if any(b["lists"][4 * w + r] for r in range(4))} == {0, 3}
        assert {w for b in plan[1:] for w in range(4) if any(b["lists"][4 * w + r] for r in range(4))} == {0}
        assert 17 * (2 * 1 + 3) > 18 * (2 * 1 + 1)           # the cost rule cuts in front of the 17th entry (staged instance 17)
    if kind == "late_idle_deep":
        b = plan[0]
        assert len(plan) == 1 and max(len(b["lists"][r]) for r in range(4)) == 17 and max(len(b["lists"][12 + r]) for r in range(4)) == 11
        assert not any(b["lists"][r] for r in range(4, 12))
        assert 16 * (2 * 1 + 3) <= 28 * (2 * 1 + 1)
        assert _idle_pairs(plan) == 2 + 2 + 1                # waves 1, 2 in both rounds, wave 3 in round 1
    if kind == "cut_then_idle":
        on = [i for i in range(n) if 0 in rows[i]]
        assert on[:16] == list(range(16)) and on[16] == 100 and len([i for i in on if i < 128]) == 20
        assert 100 * (2 * 1 + 3) > 128 * (2 * 1 + 1)         # the cost rule cuts batch one at keep = 100 < mb = 128
        assert all(len(l) <= 16 for l in plan[0]["lists"]) and all(any(plan[0]["lists"][4 * w + r] for r in range(4)) for w in range(4))
        assert sorted(len(l) for l in plan[1]["lists"][:4]) == [4, 15, 15, 16] and not any(plan[1]["lists"][4:])
        assert _idle_pairs(plan) == 3


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
def test_scan_batch_cases(kind):
    """Scan walk: (a) with and without the tile stream: same bits; (b) the instrumented kernels (which keep the flush with a branch per
    sub-tile and skip nothing): the product kernels' bits; (c) twice: same bits; (d) the oracle bars of the parity tests
    (helpers.check_grads); (e) the device's counters show the case: list entries walked (stats[3]), wave steps = 16 per (wave, round)
    that walks (stats[2])."""
    import surfel_native as n
    from oracle.surfel_oracle import Oracle
    sc, ex = _case(kind)
    a = scene_args(sc)
    rng = np.random.default_rng(23)
    gC = rng.normal(size=(3, H, W)).astype(np.float32); gO = rng.normal(size=(7, H, W)).astype(np.float32)
    run = HipRun(a).forward()
    res = {}
    for name, flag in (("scan", n.OPT_BWD_SCAN), ("scan_gather", n.OPT_BWD_SCAN | n.OPT_BWD_GATHER)):
        run.debug = flag
        res[name] = run.backward(gC, gO)
        res[name + "/again"] = run.backward(gC, gO)
    run.debug = 0
    _same(res["scan"], res["scan_gather"], kind + ": tile stream vs gather")                         # (a)
    s_scan, g_scan = _stats(run, n.OPT_BWD_SCAN, gC, gO)
    s_scan_g, g_scan_g = _stats(run, n.OPT_BWD_SCAN | n.OPT_BWD_GATHER, gC, gO)
    _same(res["scan"], g_scan, kind + ": instrumented vs product")                                  # (b)
    _same(res["scan"], g_scan_g, kind + ": instrumented (gather) vs product")
    for name in ("scan", "scan_gather"):                                                            # (c)
        _same(res[name], res[name + "/again"], kind + ": %s, run to run" % name)
    o = Oracle("f64")
    st = oracle_forward(o, a, depth_key=run.depths())[4]
    check_grads(res["scan"], o.rasterize_backward(st, gC, gO))                                      # (d)
    print("%s: scan stats %s" % (kind, s_scan[:4].tolist()))
    assert s_scan[:4].tolist() == s_scan_g[:4].tolist()                                             # (e)
    assert s_scan[3] == ex["entries"], s_scan[3]
    assert s_scan[2] == 16 * ex["wave_rounds"], s_scan[2]
