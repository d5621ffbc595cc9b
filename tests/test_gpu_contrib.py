"""-m gpu: the contribution pass (CONTRIB.md, include/surfel_contrib.h) against the fp64 oracle of tests/contrib_oracle.py, against the
library's own forward and backward, and end to end: accumulation over views, determinism, the unseen-surfel invariant, guards and
the trainer's opt-in flag.  The smallest shapes at which the kernel can go wrong: partial tiles, several workgroups per surfel, lists
longer than a staging batch.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import contrib_oracle as O
import contrib_scenes as S
from helpers import HipRun, scene_args

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _flags():
    import surfel_native as n
    return n.OPT_EXACT_BINNING | n.OPT_NO_STREAM


def render(sc, cols=None, flags=None):
    """one exactly counted forward; returns (HipRun, the buffers dict add_view takes)"""
    run = HipRun(scene_args(sc), colors_precomp=cols, debug=_flags() if flags is None else flags).forward()
    return run, dict(geom=run.ga.last(), binning=run.ba.last(), image=run.ia.last(), num_rendered=run.R, P=run.P, width=run.W, height=run.H)


def accumulate(views, P, tags=None, dominant_id=False):
    import surfel_prune as SP
    c = SP.Contribution(P, "cuda:0")
    for k, v in enumerate(views):
        c.add_view(v, tag=None if tags is None else tags[k], dominant_id=dominant_id)
    return c


def host(c, dominant_id=True):
    d = dict(sum_w=c.sum_w.cpu().numpy(), max_w=c.max_w.cpu().numpy(), hits=c.hits.cpu().numpy(), dominant=c.dominant.cpu().numpy().astype(np.int64),
             views=c.views.cpu().numpy().astype(np.int64))
    d["dominant_id"] = c.dominant_ids[-1].cpu().numpy().astype(np.int64) if (dominant_id and c.dominant_ids) else None
    return d


def raw(c):
    """the accumulator bytes, `stamp` excepted"""
    return {name: getattr(c, name).cpu().numpy().tobytes() for name in ("sum_q", "hits_q", "max_bits", "dominant_q", "views_q")}


_oracle = {}


def oracle_case(name):
    if name not in _oracle:
        sc, cols, n_theta = S.ORACLE_SCENES[name]()
        _oracle[name] = (sc, S.colors_of(sc, cols), O.walk(sc, n_theta))
    return _oracle[name]


def device_stats(name):
    sc, cols, o = oracle_case(name)
    run, view = render(sc, cols)
    c = accumulate([view], run.P, dominant_id=True)
    return sc, o, run, c, host(c)


# ------------------------------------------------------------------------------------------------ 1 - 3: against the oracle
@pytest.mark.parametrize("name", ["random14", "random40"])
def test_matches_the_oracle_on_tilted_random_surfels(name):
    """72 x 56: partial tiles on both edges, 5 x 4 workgroups"""
    sc, o, run, c, st = device_stats(name)
    print(name, "pairs", int(st["hits"].sum()), "oracle lo/hi", int(o["lo"]["hits"].sum()), int(o["hi"]["hits"].sum()))
    O.check_device(st, o)


@pytest.mark.parametrize("name", ["stacked035", "stacked085", "tiny"])
def test_matches_closed_forms_on_axis_discs(name):
    """no pixel of these scenes is undetermined, so lo == hi == the closed forms (tests/test_contrib_cpu.py holds the oracle to them); the
    big disc of the stacked pair spans several tiles: its sums are assembled from as many workgroups"""
    sc, o, run, c, st = device_stats(name)
    assert not o["undetermined"].any()
    O.check_device(st, o)
    assert np.array_equal(st["hits"], o["lo"]["hits"]) and np.array_equal(st["dominant"], o["lo"]["dominant"])
    if name != "tiny":      # the big disc (index 1) is the heaviest surfel of pixels in several tiles
        assert len({(y // 16, x // 16) for y, x in zip(*np.nonzero(st["dominant_id"] == 1))}) >= 4


def test_lists_longer_than_a_batch_that_end_inside_it():
    """48 x 48, 700 surfels in every tile list (three staging batches); every pixel saturates inside the second batch"""
    sc, o, run, c, st = device_stats("long")
    assert run.R == 9 * S.LONG_P
    O.check_device(st, o)
    deepest = int(np.nonzero(st["hits"])[0].max())
    print("deepest composited surfel", deepest, "oracle", int(np.nonzero(o["hi"]["hits"])[0].max()))
    assert 256 < deepest < 512
    assert not st["hits"][512:].any() and not st["views"][512:].any() and not st["hits"][deepest + 1:].any()
    assert st["views"][:S.LONG_FAINT].all()


# ------------------------------------------------------------------------------------------------ 4: ties to the existing library
def test_exact_ties_to_the_forward_and_the_backward():
    import torch
    import surfel_native as n
    sc, cols, o = oracle_case("random40")
    lib = n.load()
    stats = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    assert lib.surfel_debug_set_blend_stats(n.ptr(stats)) == 0
    try:
        run, view = render(sc, cols)
        c = accumulate([view], run.P)
        torch.cuda.synchronize()
    finally:
        lib.surfel_debug_set_blend_stats(None)
    s = stats.cpu().numpy()
    hits = c.hits.cpu().numpy()
    print("pairs: forward", int(s[6]), "pass", int(hits.sum()), "global atomics", int(s[7]))
    assert int(hits.sum()) == int(s[6]) > 0      # the forward's composited pairs, pair for pair
    assert 0 < int(s[7]) < int(s[6])             # far fewer global atomics than pairs
    # sum of all weights = sum over pixels of the alpha image 1 - T: each weight is quantised to 2^-25 and the fp32 recurrence loses
    # at most an ulp per pair
    total = float(c.sum_q.sum().item()) / 2.0 ** 24
    alpha = float(run.others[1].double().sum().item())
    print("sum of weights", total, "alpha image", alpha, "bound", hits.sum() * 2.0 ** -23)
    assert abs(total - alpha) <= hits.sum() * 2.0 ** -23
    # the only route to the sum at the parent commit: a backward with ones on channel 0 of dL/dcolour
    gC = np.zeros((3, run.H, run.W), np.float32); gC[0] = 1.0
    g = run.backward(gC, np.zeros((7, run.H, run.W), np.float32))
    ref = g["colors"][:, 0].astype(np.float64)
    sw = c.sum_w.cpu().numpy()
    assert np.all(np.abs(sw - ref) <= 1e-4 * np.abs(ref) + hits * 2.0 ** -24), np.abs(sw - ref).max()


# ------------------------------------------------------------------------------------------------ 5: accumulation and determinism
def test_accumulation_is_order_free_and_deterministic():
    P = 40
    (ra, va), (rb, vb) = (render(*S.random_scene(6, P, view_index=k)[:2]) for k in (0, 2))
    ab, ba, a, b = accumulate([va, vb], P), accumulate([vb, va], P), accumulate([va], P), accumulate([vb], P)
    assert raw(ab) == raw(ba) == raw(accumulate([va, vb], P))      # the order of views does not matter; the same calls give the same bytes
    for k in ("sum_q", "hits_q", "dominant_q"):
        assert np.array_equal(getattr(ab, k).cpu().numpy(), getattr(a, k).cpu().numpy() + getattr(b, k).cpu().numpy()), k
    assert np.array_equal(ab.max_bits.cpu().numpy(), np.maximum(a.max_bits.cpu().numpy(), b.max_bits.cpu().numpy()))
    va_, vb_ = a.views.cpu().numpy(), b.views.cpu().numpy()
    assert set(np.unique(va_)) <= {0, 1} and np.array_equal(ab.views.cpu().numpy(), va_ + vb_)
    both = (va_ == 1) & (vb_ == 1)
    assert both.any() and np.array_equal(ab.views.cpu().numpy() == 2, both)
    assert not np.array_equal(a.sum_q.cpu().numpy(), b.sum_q.cpu().numpy())      # (two different views)
    twice = accumulate([va, va], P, tags=[1, 1])      # the same tag twice: one view
    assert np.array_equal(twice.views.cpu().numpy(), va_) and np.array_equal(twice.hits.cpu().numpy(), 2 * a.hits.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 6: the end-to-end invariant
def e2e_scene(view_index, seed=11, W=96, H=80):
    """260 large opaque surfels in front, 140 small ones far behind them (many hidden, some only ever END a pixel), every sixth surfel
    moved out of every frustum"""
    import synthetic
    a = synthetic.make_scene(260, W, H, seed=seed, px_radius=6.0, z_near=2.5, z_far=4.0, tilt=True, view_index=view_index)
    b = synthetic.make_scene(140, W, H, seed=seed + 100, px_radius=1.2, z_near=6.0, z_far=7.0, tilt=True, view_index=view_index)
    sc = dict(a)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        sc[k] = np.concatenate([a[k], b[k]], 0)
    sc["opacities"] = np.random.default_rng(seed).uniform(0.85, 0.99, (400, 1)).astype(np.float32)
    sc["means3D"][::6, 0] += 12.0
    return sc


def test_removing_unseen_surfels_changes_no_bit_of_any_view():
    """why terminators count as seen: a surfel that only ever ended a pixel must stay, or the next one comes through"""
    import surfel_prune as SP
    P, K = 400, 3
    scenes = [e2e_scene(k) for k in range(K)]
    runs = [render(sc) for sc in scenes]
    c = accumulate([v for _, v in runs], P)
    unseen = SP.unseen_mask(c).cpu().numpy()
    enders = int(((c.views.cpu().numpy() > 0) & (c.hits.cpu().numpy() == 0)).sum())
    print("unseen %d of %d, seen without ever being composited %d" % (unseen.sum(), P, enders))
    assert 0.1 * P <= unseen.sum() <= 0.9 * P
    keep = ~unseen
    for sc, (run, _) in zip(scenes, runs):
        cut = dict(sc)
        for k in ("means3D", "scales", "rotations", "opacities", "shs"):
            cut[k] = sc[k][keep]
        again, _ = render(cut)
        assert again.P == int(keep.sum())
        assert np.array_equal(again.color.cpu().numpy().view(np.uint32), run.color.cpu().numpy().view(np.uint32))
        assert np.array_equal(again.others.cpu().numpy().view(np.uint32), run.others.cpu().numpy().view(np.uint32))


def test_a_surfel_that_only_ends_pixels_is_kept():
    """the stacked scene has such a surfel (the oracle finds it: seen, never composited): it counts as seen, and with every unseen surfel
    gone — more than half of the scene — the image keeps its bits"""
    import surfel_prune as SP
    sc, cols, o = oracle_case("long")
    enders = np.nonzero(o["lo"]["seen"] & (o["hi"]["hits"] == 0))[0]
    assert enders.size >= 1
    run, view = render(sc, cols)
    c = accumulate([view], run.P)
    unseen = SP.unseen_mask(c).cpu().numpy()
    assert not unseen[enders].any() and unseen[512:].all()

    def image_without(drop):
        cut = dict(sc)
        for k in ("means3D", "scales", "rotations", "opacities", "shs"):
            cut[k] = sc[k][~drop]
        return render(cut, cols[~drop])[0].color.cpu().numpy().view(np.uint32)
    before = run.color.cpu().numpy().view(np.uint32)
    assert np.array_equal(image_without(unseen), before)


# ------------------------------------------------------------------------------------------------ 7: edges and guards
def test_edges_empty_frames_null_map_and_lazy_frames():
    import torch
    import surfel_native as n
    import surfel_prune as SP
    sc, cols, _ = S.random_scene(1, 14)
    # R == 0: every surfel behind the camera
    gone = dict(sc); gone["means3D"] = sc["means3D"].copy(); gone["means3D"][:, 2] -= 50.0
    run, view = render(gone, cols)
    assert run.R == 0
    c = SP.Contribution(14, "cuda:0")
    dom = c.add_view(view, dominant_id=True)
    assert all(not getattr(c, name).any() for name, _ in SP._FIELDS) and bool((dom == -1).all())      # nothing is touched
    # P == 0
    z = SP.Contribution(0, "cuda:0")
    z.add_view(dict(view, P=0))
    # dominant_id = NULL gives the same accumulators as with the map
    run, view = render(sc, cols)
    assert raw(accumulate([view], 14)) == raw(accumulate([view], 14, dominant_id=True))
    with pytest.raises(ValueError, match="accumulators hold"):
        SP.Contribution(13, "cuda:0").add_view(view)
    # a capacity-binned, lazily counted frame is refused: its num_rendered is a capacity
    lib = n.load()
    lazy = None
    for _ in range(3):      # the first frame of a size teaches the capacity
        lazy, lview = render(sc, cols, flags=n.opt_tile_sort(2) | n.OPT_LAZY_COUNT | n.OPT_NO_STREAM)
        binning = lib.surfel_debug_last_binning()
        n.forward_count()
    assert binning == 4, binning
    before = SP.launches
    with pytest.raises(RuntimeError, match=r"\(-1\): .*SURFEL_OPT_EXACT_BINNING"):
        SP.Contribution(14, "cuda:0").add_view(lview)
    assert SP.launches == before
    torch.cuda.synchronize()


def test_nothing_is_written_outside_the_arrays():
    """guard pages behind the six arrays and dominant_id, a byte pattern in front of them (tests/contrib_guard_run.py, its own process)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "contrib_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "contrib_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count(" ok: ") == 2, p.stdout


# ------------------------------------------------------------------------------------------------ 8: the trainer's flag
def _train(iterations, **kw):
    import torch
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gt = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    cams = TR.capture_views(gt, TR.orbit_cameras(3, 64, 48, device=dev), torch.zeros(3, device=dev))
    gt.spatial_lr_scale = 1.0
    tr = TR.Trainer(gt, cams, TR.optimization_params(), TR.pipeline_params(depth_ratio=1.0), **kw)
    counts, losses = [], []
    for _ in range(iterations):
        tr.step()
        counts.append(tr.model.P); losses.append(tr.last["scalars"].clone())
    torch.cuda.synchronize()
    return tr, counts, torch.stack(losses).cpu().numpy()


def test_trainer_prunes_only_when_asked():
    import surfel_prune as SP
    before = SP.launches
    t0, c0, l0 = _train(60)
    t1, c1, l1 = _train(60)
    assert SP.launches == before and t0.pruned == []      # no flags: no contribution launch ...
    assert c0 == [800] * 60 and np.array_equal(t0.model.theta.cpu().numpy().view(np.uint32), t1.model.theta.cpu().numpy().view(np.uint32))      # ... and the same bits
    tr, counts, losses = _train(60, prune_at=[40], prune_min_max_weight=0.05)
    print("pruned", tr.pruned)
    assert SP.launches == before + 3      # one pass per training camera, once
    assert counts[:39] == [800] * 39 and counts[39] < 800 and counts[39:] == [counts[39]] * 21 and counts[39] > 0
    assert tr.pruned == [(40, 800, counts[39])] and np.isfinite(losses).all()
    assert np.array_equal(losses[:39], l0[:39])      # identical until the prune
    assert tr.model.m.numel() == tr.model.theta.numel() == tr.model.grad.numel()
    import surfel_trainer as TR
    with pytest.raises(ValueError, match="prune_min"):
        TR.Trainer(tr.model, tr.cams, prune_at=[5])
