"""CPU tests of the label pass (SELECT.md): the library surface, the oracle (tests/select_oracle.py) against the contribution oracle,
the condition on the GPU tests' scenes, the arg-max rule, the file format, the mask reader and the argument checks.  No device is
touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import contrib_oracle as CO
import contrib_scenes as CS
import select_oracle as O
import select_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_select.h"
NAME = "surfel_rasterize_label_votes"

_traces = {}


def trace(name):
    """the oracle's trace of a named scene of the contribution tests, computed once"""
    if name not in _traces:
        sc, cols, n_theta = CS.ORACLE_SCENES[name]()
        _traces[name] = (sc, O.trace(sc, n_theta))
    return _traces[name]


# ------------------------------------------------------------------------------------------------ library surface
def test_select_header_exported_and_signature_matches():
    """include/surfel_select.h <-> SIGNATURES["surfel_select.h"] <-> SELECT_EXPORTS <-> the library's export"""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib_path = os.path.join(PKG, "lib", "libsurfel_hip.so")
    assert os.path.exists(lib_path), "libsurfel_hip.so not built: run __graft_entry__.build()"
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 1
    assert [p[0] for p in protos] == list(n.SIGNATURES[HEADER]) == n.SELECT_EXPORTS == [NAME]
    others = [name for h, group in n.SIGNATURES.items() if h != HEADER for name in group]
    assert NAME not in others and NAME not in n.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    assert NAME in set(re.findall(r" T (\w+)$", out, re.M))
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64}
    name, ret, params = protos[0]
    fn = getattr(lib, name)
    assert ret == "int" and fn.restype is C.c_int
    assert fn.argtypes is not None and len(fn.argtypes) == len(params) == 12
    for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
        where = (k, ctype, pname, at)
        if ctype in scalars:
            assert at is scalars[ctype], where
        else:
            assert ctype.endswith("*"), where
            assert (at is n.DevPtr) == (pname != "stream"), where      # every pointer of this header is a device pointer
        assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
    assert [p for p in params][7:10] == [("uint8_t*", "labels"), ("int", "num_labels"), ("uint64_t*", "votes")]
    import surfel_select as SS
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    assert int(re.search(r"#define SURFEL_SELECT_FRAC_BITS (\d+)", hdr).group(1)) == SS.FRAC_BITS == 24
    assert int(re.search(r"#define SURFEL_SELECT_MAX_LABELS (\d+)", hdr).group(1)) == SS.MAX_LABELS == 32
    assert int(re.search(r"#define SURFEL_SELECT_UNLABELLED (\d+)", hdr).group(1)) == SS.UNLABELLED == S.IGNORE == 255


def test_select_source_is_built_with_the_forwards_flags_and_leaves_the_walk_alone():
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_select", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "surfel_select.hip" in mod.SOURCES and mod.EXTRA["surfel_select.hip"] == mod.EXTRA["surfel_forward.hip"] == mod.EXTRA["surfel_contrib.hip"]
    assert any(h.endswith(HEADER) for h in mod.HEADERS) and "surfel_select_kernel.h" in mod.HEADERS and "surfel_tile_walk.h" in mod.HEADERS
    csrc = os.path.join(PKG, "csrc")
    for f in ("surfel_forward.hip", "surfel_backward.hip", "surfel_backward_scan.hip", "surfel_preprocess.hip", "surfel_sort.hip", "surfel_contrib.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert "surfel_select" not in txt and "SelectArgs" not in txt, f
    # the walk is surfel_tile_walk.h's: its definitions occur there, and no private copy of it in either pass
    walk = open(os.path.join(csrc, "surfel_tile_walk.h")).read()
    for shared in ("pair_hit(", "make_foot(", "subtile_overlap(", "thread_pixel(", "block_tile("):
        assert shared in walk, shared
    for f in ("surfel_select.hip", "surfel_contrib.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "surfel_tile_walk.h"' in txt and "tile_walk(" in txt, f
        for private in ("pair_hit(", "make_foot(", "subtile_overlap(", "thread_pixel(", "block_tile(", "T_EPS"):
            assert private not in txt, (f, private)
    src = open(os.path.join(csrc, "surfel_select.hip")).read()
    body = src.split("select_kernel(SelectArgs a)")[1]
    assert "atomicAdd(&dst[k], (unsigned long long)v)" in body and "float*" not in body      # integer accumulators only


# ------------------------------------------------------------------------------------------------ the oracle and the scenes
@pytest.mark.parametrize("name", ["random14", "long"])
def test_per_label_sums_add_up_to_the_contribution_oracle(name):
    """with nothing ignored, the labels partition the determined pixels: the per-label sums and pair counts add up to
    contrib_oracle.walk's, and the undetermined pixels are its own"""
    sc, tr = trace(name)
    ref = CO.walk(sc, CS.ORACLE_SCENES[name]()[2])
    assert np.array_equal(tr["undetermined"], ref["undetermined"]) and np.array_equal(tr["covered"], ref["covered"])
    W, H = int(sc["W"]), int(sc["H"])
    for L, K in ((S.halves(W, H), 2), (S.checker(W, H, 5), 5), (S.blocks4(W, H, 32), 32), (S.random(W, H, 5, ignored=0.0), 5)):
        o = O.route(tr, L, K)
        for side in ("lo", "hi"):
            assert np.allclose(o[side]["sum_w"].sum(1), ref[side]["sum_w"], rtol=1e-12, atol=1e-15), (name, K, side)
            assert np.array_equal(o[side]["pairs"].sum(1), ref[side]["hits"]), (name, K, side)
    # an ignored pixel votes for nothing and is never undetermined
    L = S.random(W, H, 5)
    o = O.route(tr, L, 5)
    assert (L == S.IGNORE).any() and not o["undetermined"][L == S.IGNORE].any()
    assert np.all(o["lo"]["sum_w"].sum(1) <= ref["lo"]["sum_w"] + 1e-12) and o["lo"]["sum_w"].sum() < ref["lo"]["sum_w"].sum()
    o0 = O.route(tr, S.all_ignored(W, H), 2)
    assert not o0["hi"]["sum_w"].any() and not o0["hi"]["pairs"].any()


@pytest.mark.parametrize("name", sorted(CS.ORACLE_SCENES))
def test_gpu_scenes_keep_their_cap(name):
    """the condition on the inputs of tests/test_gpu_select.py, which are those of tests/test_gpu_contrib.py: at most 1 % of the covered
    pixels hold a marginal pair"""
    sc, tr = trace(name)
    und, cov = int(tr["undetermined"].sum()), int(tr["covered"].sum())
    assert cov > 0 and und <= 0.01 * cov, (und, cov)


def test_label_images():
    W, H = 72, 56
    h = S.halves(W, H)
    assert h.dtype == np.uint8 and h.shape == (H, W) and (h[:, :37] == 0).all() and (h[:, 37:] == 1).all() and not S.halves(W, H, 1).any()
    c, b = S.checker(W, H, 2), S.blocks4(W, H, 5)
    for y0 in range(0, H, 4):
        for x0 in range(0, W, 4):
            assert len(np.unique(c[y0:y0 + 4, x0:x0 + 4])) == 2 and len(np.unique(b[y0:y0 + 4, x0:x0 + 4])) == 1
    r = S.random(W, H, 5)
    assert set(np.unique(r)) == {0, 1, 2, 3, 4, 255} and 0.05 < (r == 255).mean() < 0.15 and np.array_equal(r, S.random(W, H, 5))
    assert (S.constant(W, H, 3) == 3).all() and (S.all_ignored(W, H) == 255).all()
    assert set(np.unique(S.PATTERNS["random"](W, H, 32))) == set(range(32))


def test_the_separable_scene_is_separable():
    """what the end-to-end GPU test's exact assertions rest on: in every view, no pixel on one side of the cut holds a live pair of a
    surfel of the other cluster whose alpha reaches (1/255)(1 - 1e-3) — and every cluster is seen"""
    L = S.separable_labels()
    cluster = S.separable_cluster()
    assert L.shape == (S.SEP_H, S.SEP_W) and set(np.unique(L)) == {0, 1}
    for view in range(S.SEP_VIEWS):
        sc = S.separable_scene(view)
        tr = O.trace(sc, 20_000)
        seen = np.zeros(2, np.int64)
        for i, in_rect, comp, w, cand in tr["pairs"]:
            assert not (cand & (L != cluster[i])).any(), (view, i)
            seen[cluster[i]] += bool(comp.any())
        assert seen.min() >= S.SEP_PER_CLUSTER // 2, (view, seen)


# ------------------------------------------------------------------------------------------------ assign, files
def _assign_numpy(v, bias=None, min_share=0.0):
    v = np.asarray(v, np.int64)
    score = v if bias is None else np.asarray(bias, np.float64)[None, :] * v.astype(np.float64)
    out = np.full(v.shape[0], -1, np.int32)
    for p in range(v.shape[0]):
        k = [j for j in range(v.shape[1]) if score[p, j] == score[p].max()][0]      # the lowest k among the maxima
        total = int(v[p].sum())
        if total != 0 and not float(v[p, k]) < min_share * float(total):
            out[p] = k
    return out


def test_assign_matches_its_restatement():
    import torch
    import surfel_select as SS
    v = np.array([[5, 3, 1], [0, 0, 0], [2, 2, 1], [0, 7, 7], [1, 0, 0], [4, 5, 4], [1 << 40, (1 << 40) + 1, 0], [10, 9, 9]], np.int64)
    tv = torch.from_numpy(v)
    assert SS.assign(tv).tolist() == [0, -1, 0, 1, 0, 1, 1, 0] and SS.assign(tv).dtype == torch.int32
    cases = [dict(), dict(bias=[1.0, 1.0, 1.0]), dict(bias=[0.5, 1.0, 1.0]), dict(bias=[1.0, 0.0, 3.0]), dict(min_share=0.5), dict(min_share=0.4, bias=[0.2, 1.0, 1.0]),
             dict(min_share=1.0)]
    for kw in cases:
        assert np.array_equal(SS.assign(tv, **kw).numpy(), _assign_numpy(v, **kw)), kw
    assert SS.assign(tv, bias=[0.5, 1.0, 1.0]).tolist() == [1, -1, 1, 1, 0, 1, 1, 1]      # the bias softens label 0; ties still go to the lowest k
    assert SS.assign(tv, min_share=0.5).tolist() == [0, -1, -1, 1, 0, -1, 1, -1]
    rng = np.random.default_rng(0)
    r = rng.integers(0, 4, (500, 5)).astype(np.int64) << 20
    for kw in (dict(), dict(bias=[1.0, 0.3, 2.0, 1.0, 0.0]), dict(min_share=0.35)):
        assert np.array_equal(SS.assign(torch.from_numpy(r), **kw).numpy(), _assign_numpy(r, **kw)), kw
    lv = SS.LabelVotes(8, 3, "cpu")
    lv.votes = tv
    assert SS.assign(lv).tolist() == SS.assign(tv).tolist()
    assert np.allclose(lv.weights.numpy()[0], [5 / 2.0 ** 24, 3 / 2.0 ** 24, 1 / 2.0 ** 24]) and lv.weights.dtype == torch.float64
    for bad in (dict(bias=[1.0, 1.0]), dict(bias=[1.0, -1.0, 1.0]), dict(bias=[1.0, float("nan"), 1.0]), dict(min_share=1.5), dict(min_share=-0.1)):
        with pytest.raises(ValueError, match="surfel_select"):
            SS.assign(tv, **bad)
    with pytest.raises(ValueError, match="surfel_select"):
        SS.assign(tv.double())
    labels = SS.assign(tv)
    assert SS.select_mask(labels, keep=[0]).tolist() == [True, False, True, False, True, False, False, True]
    assert SS.select_mask(labels, remove=[1, -1]).tolist() == [True, False, True, False, True, False, False, True]
    for bad in (dict(), dict(keep=[0], remove=[1])):
        with pytest.raises(ValueError, match="surfel_select"):
            SS.select_mask(labels, **bad)


def test_npz_round_trip(tmp_path):
    import torch
    import surfel_select as SS
    lv = SS.LabelVotes(6, 4, "cpu")
    lv.votes = torch.arange(24, dtype=torch.int64).reshape(6, 4) << 30
    lv.views = 3
    p = str(tmp_path / "labels.npz")
    lv.save(p, labels=SS.assign(lv))
    assert os.path.exists(p)
    d = SS.LabelVotes.load(p)
    assert (d.P, d.K, d.views) == (6, 4, 3) and d.votes.dtype == torch.int64 and torch.equal(d.votes, lv.votes)
    with np.load(p) as z:
        assert sorted(z.files) == ["labels", "num_labels", "views", "votes"] and z["labels"].dtype == np.int32 and z["labels"].tolist() == [3] * 6
    lv.save(p)
    with np.load(p) as z:
        assert sorted(z.files) == ["num_labels", "views", "votes"]


# ------------------------------------------------------------------------------------------------ masks
def test_mask_reader_and_missing_masks(tmp_path):
    from types import SimpleNamespace
    from PIL import Image
    import surfel_select as SS
    rng = np.random.default_rng(2)
    gray = rng.integers(0, 4, (6, 8)).astype(np.uint8); gray[0, 0] = 255
    Image.fromarray(gray).save(str(tmp_path / "a.png"))
    pal = Image.fromarray(gray % 3); pal.putpalette([255, 0, 0, 0, 255, 0, 0, 0, 255] + [0] * 759); assert pal.mode == "P"; pal.save(str(tmp_path / "b.png"))
    soft = rng.integers(0, 256, (6, 8)).astype(np.uint8); soft[0, :2] = [127, 128]
    Image.fromarray(soft).save(str(tmp_path / "c.png"))
    Image.fromarray(np.stack([soft] * 3, -1)).save(str(tmp_path / "d.png"))
    a = SS.read_mask(str(tmp_path / "a.png"), 8, 6)
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"] and np.array_equal(a, gray)
    assert np.array_equal(SS.read_mask(str(tmp_path / "b.png"), 8, 6), gray % 3)      # a palette image: the index is the label, not its colour
    assert np.array_equal(SS.read_mask(str(tmp_path / "c.png"), 8, 6, binary=True), (soft > 127).astype(np.uint8))
    assert np.array_equal(SS.read_mask(str(tmp_path / "d.png"), 8, 6, binary=True), (soft > 127).astype(np.uint8))
    with pytest.raises(ValueError, match="surfel_select"):
        SS.read_mask(str(tmp_path / "d.png"), 8, 6)
    # nearest neighbour: an integer factor repeats pixels, and no label is invented
    big = SS.read_mask(str(tmp_path / "a.png"), 16, 12)
    assert big.shape == (12, 16) and np.array_equal(big, np.repeat(np.repeat(gray, 2, 0), 2, 1))
    odd = SS.read_mask(str(tmp_path / "a.png"), 11, 7)
    assert odd.shape == (7, 11) and set(np.unique(odd)) <= set(np.unique(gray))
    cams = [SimpleNamespace(image_name=n, image_width=8, image_height=6) for n in ("a", "missing", "b", "gone")]
    masks, missing = SS.load_masks(str(tmp_path), cams)
    assert sorted(masks) == ["a", "b"] and missing == ["missing", "gone"]
    # label_votes skips and counts the cameras without a mask before it renders anything
    model = SimpleNamespace(P=5, device="cpu")
    lv = SS.label_votes(model, [cams[1], cams[3]], masks, 3, None, None)
    assert lv.skipped == 2 and lv.views == 0 and not lv.votes.any() and tuple(lv.votes.shape) == (5, 3)
    b = SS.build_parser().parse_args(["-m", "y", "--masks", "d", "--binary", "--keep", "1", "--min_share", "0.6", "--as_model", "o"])
    assert b.binary and b.keep == [1] and b.remove is None and b.min_share == 0.6 and b.as_model == "o" and b.num_labels is None and not b.report
    with pytest.raises(SystemExit):
        SS.build_parser().parse_args(["-m", "y", "--masks", "d", "--keep", "1", "--remove", "0"])


# ------------------------------------------------------------------------------------------------ refusals
def test_wrapper_argument_errors_need_no_device():
    import torch
    import surfel_native as n
    import surfel_select as SS
    for P, K in ((-1, 2), (4, 0), (4, 33)):
        with pytest.raises(ValueError, match="surfel_select"):
            SS.LabelVotes(P, K, "cpu")
    lv = SS.LabelVotes(4, 2, "cpu")
    buf = torch.zeros(256, dtype=torch.uint8)
    view = dict(geom=buf, binning=buf, image=buf, num_rendered=1, width=16, height=16)
    with pytest.raises(RuntimeError, match=r"surfel_select: tensors must live on a HIP device \(the votes are on cpu\)"):
        lv.add_view(view, buf.view(16, 16))
    with pytest.raises(ValueError, match=r"surfel_select: the view's buffers lack 'binning'"):
        lv.add_view(dict(geom=buf), buf.view(16, 16))
    # the entry itself: checked before any device is touched
    p = n.C.c_void_p(256)
    for args, msg in (((4, 1, 0, 16, p, p, p, p, 2, p, 0), "bad sizes"), ((4, -1, 16, 16, p, p, p, p, 2, p, 0), "bad sizes"),
                      ((4, 1, 16, 16, p, p, p, p, 0, p, 0), r"num_labels must be in 1 \.\. 32"), ((4, 1, 16, 16, p, p, p, p, 33, p, 0), r"num_labels must be in 1 \.\. 32"),
                      ((4, 1, 16, 16, None, p, p, p, 2, p, 0), "buffer is NULL"), ((4, 1, 16, 16, p, p, p, None, 2, p, 0), "labels pointer is NULL"),
                      ((4, 1, 16, 16, p, p, p, p, 2, None, 0), "votes pointer is NULL")):
        with pytest.raises(RuntimeError, match=r"surfel_rasterize_label_votes failed \(-1\): .*" + msg):
            n.call(None, NAME, *args)
    assert n.call(None, NAME, 0, 5, 16, 16, None, None, None, None, 2, None, 0) == 0      # P == 0
    assert n.call(None, NAME, 4, 0, 16, 16, None, None, None, None, 2, None, 0) == 0      # R == 0
    with pytest.raises(RuntimeError, match="HIP device"):      # a host tensor never reaches a device-pointer parameter
        n.call(None, NAME, 4, 1, 16, 16, buf, buf, buf, buf, 2, torch.zeros(8, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="surfel_select: labels must be a tensor of the model's 4 surfels"):
        SS.split_model(type("M", (), {"P": 4})(), torch.zeros(3, dtype=torch.int32), keep=[0])
    with pytest.raises(ValueError, match="surfel_select: a label image holds integers in 0 .. 255"):
        SS._label_tensor(np.array([[0, 300]]), "cpu")
