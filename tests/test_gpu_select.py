"""-m gpu: the label pass (SELECT.md, include/surfel_select.h) against the fp64 oracle of tests/select_oracle.py, against the
contribution pass byte for byte, against itself (decomposition, permutation, order), at its edges, behind guard pages, and end to end
through surfel_select.py.  The scenes are those of tests/test_gpu_contrib.py: partial tiles, several workgroups per surfel, lists
longer than a staging batch.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

import contrib_scenes as CS
import select_oracle as O
import select_scenes as S
from helpers import HipRun, scene_args

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
NAME = "surfel_rasterize_label_votes"


def _flags():
    import surfel_native as n
    return n.OPT_EXACT_BINNING | n.OPT_NO_STREAM


def render(sc, cols=None, flags=None):
    """one exactly counted forward; returns (HipRun, the buffers dict add_view takes)"""
    run = HipRun(scene_args(sc), colors_precomp=cols, debug=_flags() if flags is None else flags).forward()
    return run, dict(geom=run.ga.last(), binning=run.ba.last(), image=run.ia.last(), num_rendered=run.R, P=run.P, width=run.W, height=run.H)


_frames, _traces = {}, {}


def frame(name):
    """(scene, HipRun, view, the contribution pass's sum_q as int64 numpy) of a named scene, rendered once"""
    if name not in _frames:
        import surfel_prune as SP
        if name == "frame50x37":
            sc, cols, _ = CS.random_scene(6, 40, W=50, H=37)
        else:
            sc, cols, _ = CS.ORACLE_SCENES[name]()
        run, view = render(sc, CS.colors_of(sc, cols))
        c = SP.Contribution(run.P, DEV)
        c.add_view(view)
        _frames[name] = (sc, run, view, c.sum_q.cpu().numpy())
    return _frames[name]


def trace(name):
    if name not in _traces:
        sc, cols, n_theta = CS.ORACLE_SCENES[name]()
        _traces[name] = O.trace(sc, n_theta)
    return _traces[name]


def votes_of(view, L, K, into=None):
    """the votes of one view under label image L as int64 numpy [P, K]"""
    import torch
    import surfel_select as SS
    lv = into if into is not None else SS.LabelVotes(view["P"], K, DEV)
    lv.add_view(view, torch.from_numpy(np.ascontiguousarray(L, np.uint8)).to(DEV))
    return lv.votes.cpu().numpy()


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", sorted(CS.ORACLE_SCENES))
def test_votes_lie_within_the_oracles_bounds(name):
    sc, run, view, sum_q = frame(name)
    W, H = run.W, run.H
    tr = trace(name)
    for what, L, K in (("halves", S.halves(W, H), 2), ("checker", S.checker(W, H, 2), 2), ("random", S.random(W, H, 5), 5)):
        o = O.route(tr, L, K)
        v = votes_of(view, L, K)
        w = v.astype(np.float64) / 2.0 ** 24
        print(name, what, "mass", w.sum(0), "oracle lo", o["lo"]["sum_w"].sum(0), "hi", o["hi"]["sum_w"].sum(0))
        assert v.sum() > 0
        O.check_device(w, o)


# ------------------------------------------------------------------------------------------------ exact tie to the contribution pass
@pytest.mark.parametrize("K", [1, 2, 5, 8, 9, 32])
@pytest.mark.parametrize("name", ["random40", "long", "frame50x37"])
def test_row_sums_are_the_contribution_pass_byte_for_byte(name, K):
    """no pixel ignored: votes.sum(1) == Contribution.sum_q of the same buffers — uniform rows (blocks4), mixed rows (checker, random),
    a cut through rows (halves), on both sides of every bucket edge (K = 2 | 5, 8 | 9, 32); frame50x37: 1850 label bytes, partial
    tiles on both edges"""
    sc, run, view, sum_q = frame(name)
    assert sum_q.sum() > 0
    for what, make in S.PATTERNS.items():
        L = make(run.W, run.H, K)
        assert (L < K).all()
        v = votes_of(view, L, K)
        assert v.shape == (run.P, K) and np.array_equal(v.sum(1), sum_q), (what, np.abs(v.sum(1) - sum_q).max())
        if K >= 2:
            assert (v.sum(0) > 0).sum() >= 2, what      # the weight really is spread over labels
    for k in sorted({0, K // 2, K - 1}):
        v = votes_of(view, S.constant(run.W, run.H, k), K)
        assert np.array_equal(v[:, k], sum_q) and not np.delete(v, k, axis=1).any(), k


# ------------------------------------------------------------------------------------------------ exact decomposition
@pytest.mark.parametrize("name", ["random40", "long"])
def test_decomposition_ignoring_and_permutation_are_exact(name):
    sc, run, view, sum_q = frame(name)
    W, H = run.W, run.H
    for K in (5, 8):      # (8: the K + 1 run below lands in the next bucket)
        L = S.PATTERNS["random"](W, H, K)
        v = votes_of(view, L, K)
        # column k of the K-label run = column 1 of the binary run on (L == k)
        for k in range(K):
            b = votes_of(view, (L == k).astype(np.uint8), 2)
            assert np.array_equal(b[:, 1], v[:, k]) and np.array_equal(b[:, 0], sum_q - v[:, k]), (K, k)
        # ignoring a set of pixels = giving them label K in a K + 1 run and dropping that column
        drop = S.random(W, H, 2, seed=9, ignored=0.0).astype(bool) | (S.halves(W, H) == 1)
        vi = votes_of(view, np.where(drop, S.IGNORE, L), K)
        vk = votes_of(view, np.where(drop, K, L), K + 1)
        assert np.array_equal(vi, vk[:, :K]) and vk[:, K].sum() > 0 and np.array_equal(vk.sum(1), sum_q)
        assert np.array_equal(vi, votes_of(view, np.where(drop, K, L), K))      # any label >= K is ignored, not only 255
        # permuting labels permutes columns
        perm = np.random.default_rng(K).permutation(K)
        vp = votes_of(view, perm[L].astype(np.uint8), K)
        assert np.array_equal(vp[:, perm], v)


def test_all_ignored_touches_nothing_and_votes_accumulate():
    import torch
    import surfel_select as SS
    sc, run, view, sum_q = frame("random40")
    lv = SS.LabelVotes(run.P, 3, DEV)
    lv.votes += torch.arange(run.P * 3, dtype=torch.int64, device=DEV).reshape(run.P, 3) * 7 + 1
    before = lv.votes.cpu().numpy().copy()
    assert np.array_equal(votes_of(view, S.all_ignored(run.W, run.H), 3, into=lv), before)
    L = S.checker(run.W, run.H, 3)
    once = votes_of(view, L, 3)
    assert np.array_equal(votes_of(view, L, 3, into=lv), before + once) and lv.views == 2


def test_accumulation_is_order_free_and_deterministic():
    import surfel_select as SS
    P, K = 40, 5
    (ra, va), (rb, vb) = (render(*CS.random_scene(6, P, view_index=k)[:2]) for k in (0, 2))
    La, Lb = S.random(72, 56, K, seed=1), S.checker(72, 56, K)

    def acc(order):
        lv = SS.LabelVotes(P, K, DEV)
        for view, L in order:
            votes_of(view, L, K, into=lv)
        return lv.votes.cpu().numpy()
    ab, ba = acc([(va, La), (vb, Lb)]), acc([(vb, Lb), (va, La)])
    assert ab.tobytes() == ba.tobytes() == acc([(va, La), (vb, Lb)]).tobytes()
    a, b = acc([(va, La)]), acc([(vb, Lb)])
    assert np.array_equal(ab, a + b) and not np.array_equal(a, b) and a.sum() > 0 and b.sum() > 0


# ------------------------------------------------------------------------------------------------ edges and guards
def test_edges_empty_frames_bad_label_counts_null_pointers_and_lazy_frames():
    import torch
    import surfel_native as n
    import surfel_select as SS
    sc, cols, _ = CS.random_scene(1, 14)
    dev = torch.device(DEV)
    L = torch.from_numpy(S.checker(72, 56, 2)).to(DEV)
    # R == 0: every surfel behind the camera
    gone = dict(sc); gone["means3D"] = sc["means3D"].copy(); gone["means3D"][:, 2] -= 50.0
    run, view = render(gone, cols)
    assert run.R == 0
    lv = SS.LabelVotes(14, 2, DEV)
    lv.add_view(view, L)
    assert not lv.votes.any()
    # P == 0
    SS.LabelVotes(0, 2, DEV).add_view(dict(view, P=0), L)
    run, view = render(sc, cols)
    votes = torch.zeros((14, 2), dtype=torch.int64, device=DEV)
    args = lambda labels, K, v: (14, run.R, run.W, run.H, view["geom"], view["binning"], view["image"], labels, K, v, 0)
    for K in (0, 33, -1):
        with pytest.raises(RuntimeError, match=r"\(-1\): .*num_labels must be in 1 \.\. 32"):
            n.call(dev, NAME, *args(L, K, votes))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*labels pointer is NULL"):
        n.call(dev, NAME, *args(None, 2, votes))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*votes pointer is NULL"):
        n.call(dev, NAME, *args(L, 2, None))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*buffer is NULL"):
        n.call(dev, NAME, 14, run.R, run.W, run.H, None, view["binning"], view["image"], L, 2, votes, 0)
    assert not votes.any()
    for bad, msg in ((L.to(torch.int32), "labels must be uint8"), (L[:, :-1], r"labels must be \[56, 72\]"), (L.cpu(), "HIP device")):
        with pytest.raises((ValueError, RuntimeError), match="surfel_select: .*" + msg):
            SS.LabelVotes(14, 2, DEV).add_view(view, bad)
    with pytest.raises(ValueError, match="votes hold"):
        SS.LabelVotes(13, 2, DEV).add_view(view, L)
    # a capacity-binned, lazily counted frame is refused with the contribution pass's code: its num_rendered is a capacity
    lib = n.load()
    for _ in range(3):      # the first frame of a size teaches the capacity
        lazy, lview = render(sc, cols, flags=n.opt_tile_sort(2) | n.OPT_LAZY_COUNT | n.OPT_NO_STREAM)
        binning = lib.surfel_debug_last_binning()
        n.forward_count()
    assert binning == 4, binning
    before = SS.launches
    with pytest.raises(RuntimeError, match=r"\(-1\): .*SURFEL_OPT_EXACT_BINNING"):
        SS.LabelVotes(14, 2, DEV).add_view(lview, L)
    assert SS.launches == before
    torch.cuda.synchronize()


def test_nothing_is_read_or_written_outside_the_arrays():
    """guard pages behind votes and behind the 50 x 37 label image, a byte pattern in front of both (tests/select_guard_run.py, its own
    process)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "select_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "select_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count(" ok: ") == 3, p.stdout


# ------------------------------------------------------------------------------------------------ end to end
PIPE = argparse.Namespace(depth_ratio=0.0, debug=0, compute_cov3D_python=False, convert_SHs_python=False)


def _separable():
    scenes = [S.separable_scene(v) for v in range(S.SEP_VIEWS)]
    cams = [S.camera_of(sc, "view_%d" % v, DEV) for v, sc in enumerate(scenes)]
    return scenes[0], cams


def test_masks_to_labels_to_two_models_and_back_to_masks():
    """tests/test_select_cpu.py proves the scene separable, so every assertion here is exact"""
    import torch
    import surfel_model
    import surfel_prune as SP
    import surfel_select as SS
    sc, cams = _separable()
    model = S.model_of(sc, DEV)
    bg = torch.zeros(3, device=DEV)
    L = S.separable_labels()
    masks = {cam.image_name: L for cam in cams[:-1]}
    masks[cams[-1].image_name] = torch.from_numpy(L)      # (numpy or torch, host or device)
    extra = S.camera_of(sc, "no_mask", DEV)
    lv = SS.label_votes(model, cams + [extra], masks, 2, PIPE, bg)
    assert (lv.views, lv.skipped) == (len(cams), 1)
    labels = SS.assign(lv)
    c = SP.contribution(model, cams, PIPE, bg, dominant_ids=True)
    assert np.array_equal(lv.votes.sum(1).cpu().numpy(), c.sum_q.cpu().numpy())
    hit = c.hits.cpu().numpy() > 0
    lab, cluster = labels.cpu().numpy(), S.separable_cluster()
    print("surfels composited", int(hit.sum()), "of", model.P, "per label", [(lab == k).sum() for k in (-1, 0, 1)])
    assert hit.sum() >= model.P // 2 and np.array_equal(lab[hit], cluster[hit]) and (lab[~hit] == -1).all()
    # two models: sizes add up, rows are the original's bit for bit
    keep = labels == 1
    theta = {name: model._pv[name].clone() for name, _ in surfel_model.SECTIONS}
    one, rest = S.model_of(sc, DEV), S.model_of(sc, DEV)
    assert SS.split_model(one, labels, keep=[1]) == int((~keep).sum()) and SS.split_model(rest, labels, remove=[1]) == int(keep.sum())
    assert one.P + rest.P == model.P and one.P == int((lab == 1).sum()) > 0 and rest.P > 0
    for name, _ in surfel_model.SECTIONS:
        assert torch.equal(one._pv[name].view(torch.int32), theta[name][keep].view(torch.int32)), name
        assert torch.equal(rest._pv[name].view(torch.int32), theta[name][~keep].view(torch.int32)), name
    # back to masks: wherever a surfel was composited, the re-rendered label is the side of the cut
    for v, cam in enumerate(cams):
        li = SS.label_image(model, cam, labels, 2, PIPE).cpu().numpy()
        dom = c.dominant_ids[v].cpu().numpy()
        assert li.dtype == np.uint8 and li.shape == L.shape and (dom >= 0).sum() > 100
        assert np.array_equal(li[dom >= 0], L[dom >= 0]) and set(np.unique(li)) <= {0, 1, 255}
    # more labels than one render holds (three per render): label k + 3 lands where label k did
    li5 = SS.label_image(model, cams[0], labels + 3 * (labels >= 0).to(labels.dtype), 5, PIPE).cpu().numpy()
    li2 = SS.label_image(model, cams[0], labels, 2, PIPE).cpu().numpy()
    assert np.array_equal(li5, np.where(li2 == 255, 255, li2 + 3))


def test_cli_writes_the_selection_and_a_model_directory(tmp_path, capsys):
    import torch
    from PIL import Image
    import surfel_model
    import surfel_select as SS
    sc, cams = _separable()
    model = S.model_of(sc, DEV)
    src, out, mdir = str(tmp_path / "model"), str(tmp_path / "object"), str(tmp_path / "masks")
    SS.write_model_dir(src, str(tmp_path / "nowhere"), cams, model, 7)
    os.makedirs(mdir)
    L = S.separable_labels()
    for cam in cams[:-1]:      # the last camera has no mask
        Image.fromarray(L * 255).resize((2 * S.SEP_W, 2 * S.SEP_H), Image.NEAREST).save(os.path.join(mdir, cam.image_name + ".png"))
    assert SS.main(["-m", src, "--masks", mdir, "--binary", "--keep", "1", "--as_model", out]) == 0
    assert "(1 cameras without a mask)" in capsys.readouterr().out
    folder = os.path.join(src, "point_cloud", "iteration_7")
    lv = SS.LabelVotes.load(os.path.join(folder, "labels.npz"))
    with np.load(os.path.join(folder, "labels.npz")) as z:
        lab = z["labels"]
    assert (lv.P, lv.K, lv.views) == (model.P, 2, len(cams) - 1) and np.array_equal(lab, SS.assign(lv).numpy())
    cluster = S.separable_cluster()
    assert np.array_equal(lab[lab >= 0], cluster[lab >= 0]) and (lab == 1).sum() >= S.SEP_PER_CLUSTER // 2
    want = int((lab == 1).sum())
    for ply in (os.path.join(folder, "point_cloud_selected.ply"), os.path.join(out, "point_cloud", "iteration_7", "point_cloud.ply")):
        g = surfel_model.GaussianModel(3, device=DEV)
        g.load_ply(ply)
        assert g.P == want
        assert torch.equal(g._pv["xyz"], model._pv["xyz"][torch.from_numpy(lab == 1).to(DEV)])
    assert os.path.exists(os.path.join(out, "cfg_args")) and os.path.exists(os.path.join(out, "cameras.json"))
    import surfel_io
    assert [c.image_name for c in surfel_io.read_cameras_json(os.path.join(out, "cameras.json"), device=DEV)] == [c.image_name for c in cams]
    # --report writes nothing
    before = sorted(os.listdir(folder))
    assert SS.main(["-m", src, "--masks", mdir, "--binary", "--report"]) == 0
    rep = capsys.readouterr().out
    assert "label 1:" in rep and "IoU" in rep and sorted(os.listdir(folder)) == before
