"""CPU tests of the contribution pass (CONTRIB.md): the oracle (tests/contrib_oracle.py) against closed forms and against the C fp64
oracle, the condition on the GPU tests' scenes, the pruning rules, the file format and the library surface.  No device is touched."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import analytic
import contrib_oracle as O
import contrib_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_contrib.h"

_walks = {}


def walk(name):
    """the oracle's result for a named scene, computed once"""
    if name not in _walks:
        sc, cols, n_theta = S.ORACLE_SCENES[name]()
        _walks[name] = (sc, cols, O.walk(sc, n_theta))
    return _walks[name]


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", ["stacked035", "stacked085", "tiny"])
def test_oracle_matches_closed_forms_on_axis_discs(name):
    """fronto-parallel discs on the axis: the per-disc weight maps are closed-form (the construction of analytic.stacked_discs)"""
    sc, _, o = walk(name)
    if name == "tiny":      # off the axis by a fraction of a pixel: the closed form does not apply; one disc, so w = alpha wherever it is composited
        assert o["lo"]["hits"][0] == 18 and o["lo"]["dominant"][0] == 18 and not o["undetermined"].any()
        assert 0 < o["lo"]["max_w"][0] <= 0.9 and o["lo"]["max_w"][0] <= o["lo"]["sum_w"][0]
        return
    assert not o["undetermined"].any()
    order = np.argsort(sc["means3D"][:, 2], kind="stable")
    H, W = int(sc["H"]), int(sc["W"])
    T = np.ones((H, W)); ws = {}
    for i in order:
        alpha, hit, _, _, _ = analytic.disc_alpha(sc, i)
        ws[i] = np.where(hit, alpha * T, 0.0)
        T = np.where(hit, T * (1 - alpha), T)
    stack = np.stack([ws[i] for i in order])
    dom = np.where(stack.max(0) > 0, order[stack.argmax(0)], -1)      # argmax: the first (nearest) of equal weights
    for i in order:
        assert np.isclose(o["lo"]["sum_w"][i], ws[i].sum(), rtol=1e-9) and np.isclose(o["lo"]["max_w"][i], ws[i].max(), rtol=1e-9)
        assert o["lo"]["hits"][i] == int((ws[i] > 0).sum()) and o["lo"]["dominant"][i] == int((dom == i).sum())
        for k in ("sum_w", "max_w", "hits", "dominant"):
            assert o["hi"][k][i] == o["lo"][k][i]
    assert np.array_equal(o["dominant_id"], dom)


@pytest.mark.parametrize("name", ["random14", "random40"])
def test_oracle_sum_matches_the_c_oracle_colour_gradient(name):
    """with colors_precomp and a gradient of ones on channel 0, dL/dcolour[:, 0] of the C fp64 oracle IS the sum of the blend weights"""
    from helpers import oracle_forward, scene_args
    from oracle.surfel_oracle import Oracle
    sc, cols, o = walk(name)
    orc = Oracle("f64")
    R, col, oth, radii, st = oracle_forward(orc, scene_args(sc), colors_precomp=cols)
    gC = np.zeros_like(col); gC[0] = 1.0
    g = orc.rasterize_backward(st, gC, np.zeros_like(oth))
    ref = np.asarray(g.dL_dcolors, np.float64)[:, 0]
    lo, hi = o["lo"]["sum_w"], o["hi"]["sum_w"]
    assert np.all(ref >= lo * (1 - 1e-6) - 1e-9) and np.all(ref <= hi * (1 + 1e-6) + 1e-9), np.abs(ref - lo).max()
    # ... and over all pixels, undetermined ones included, two fp64 formulations decide alike
    assert np.allclose(ref, o["full_sum_w"], rtol=1e-6, atol=1e-9), np.abs(ref - o["full_sum_w"]).max()


@pytest.mark.parametrize("name", sorted(S.ORACLE_SCENES))
def test_gpu_scenes_are_determined(name):
    """a condition on the inputs of tests/test_gpu_contrib.py: at most 1 % of the covered pixels hold a marginal pair"""
    sc, _, o = walk(name)
    und, cov = int(o["undetermined"].sum()), int(o["covered"].sum())
    assert cov > 0 and und <= 0.01 * cov, (und, cov)
    if name == "long":      # what the scene is for: lists of three batches that end inside the second one
        deepest = int(np.nonzero(o["hi"]["hits"])[0].max())
        assert 256 < deepest < 512 and not o["hi"]["seen"][512:].any() and o["lo"]["seen"][:S.LONG_FAINT].all()


# ------------------------------------------------------------------------------------------------ masks, ranking, files
def _contrib(P=8):
    import torch
    import surfel_prune as SP
    c = SP.Contribution(P, "cpu")
    w = np.array([0.5, 0.002, 0.0, 0.25, 0.25, 0.0005, 0.9, 0.25], np.float32)[:P]
    c.max_bits = torch.from_numpy(w.view(np.int32).copy())
    c.sum_q = torch.tensor([900, 3, 0, 50, 50, 1, 4000, 50], dtype=torch.int64)[:P] << 20
    c.hits_q = torch.tensor([90, 3, 0, 5, 5, 1, 400, 5], dtype=torch.int64)[:P]
    c.dominant_q = torch.tensor([7, 0, 0, 1, 1, 0, 30, 0], dtype=torch.int32)[:P]
    c.views_q = torch.tensor([3, 1, 0, 2, 2, 1, 3, 1], dtype=torch.int32)[:P]
    c.next_tag = 4
    return c


def test_prune_mask_rules_compose_and_ties_go_to_the_lower_index():
    import surfel_prune as SP
    c = _contrib()
    m = lambda **kw: SP.prune_mask(c, **kw).tolist()
    assert m() == [True] * 8
    assert m(min_max_weight=0.001) == [True, True, False, True, True, False, True, True]
    assert m(min_views=2) == [True, False, False, True, True, False, True, False]
    assert m(min_max_weight=0.001, min_views=2) == [True, False, False, True, True, False, True, False]
    # ranking by sum: 6, 0, then the three-way tie 3 = 4 = 7 in index order
    assert m(keep=3) == [True, False, False, True, False, False, True, False]
    assert m(keep=4) == [True, False, False, True, True, False, True, False]
    assert m(keep_ratio=0.5) == m(keep=4) and m(keep=8) == [True] * 8 and m(keep=0) == [False] * 8
    assert m(keep=4, score="max") == [True, False, False, True, True, False, True, False]
    assert m(keep=3, score="dominant") == [True, False, False, True, False, False, True, False]
    # the budget ranks ALL surfels, then the thresholds apply: AND
    assert m(keep=4, min_views=3) == [True, False, False, False, False, False, True, False]
    assert SP.unseen_mask(c).tolist() == [False, False, True, False, False, False, False, False]
    assert np.allclose(c.sum_w.numpy()[:2], [900 / 16.0, 3 / 16.0]) and c.sum_w.dtype.is_floating_point and c.sum_w.element_size() == 8
    assert c.max_w.numpy()[6] == np.float32(0.9) and c.max_w.numpy()[2] == 0
    for bad in (dict(keep=1, keep_ratio=0.5), dict(keep=-1), dict(keep_ratio=1.5), dict(score="volume"), dict(min_views=-1), dict(min_max_weight=-0.1)):
        with pytest.raises(ValueError):
            SP.prune_mask(c, **bad)


def test_npz_round_trip(tmp_path):
    import torch
    import surfel_prune as SP
    c = _contrib()
    p = str(tmp_path / "contribution.npz")
    c.save(p)
    assert os.path.exists(p)
    d = SP.Contribution.load(p)
    assert d.P == c.P and d.next_tag == 4
    for name, dt in SP._FIELDS:
        assert getattr(d, name).dtype == dt and torch.equal(getattr(d, name), getattr(c, name)), name
    with np.load(p) as z:
        assert sorted(z.files) == sorted([n for n, _ in SP._FIELDS] + ["next_tag"])


def test_wrapper_argument_errors_need_no_device():
    import torch
    import surfel_prune as SP
    import surfel_native as n
    c = SP.Contribution(4, "cpu")
    buf = torch.zeros(256, dtype=torch.uint8)
    view = dict(geom=buf, binning=buf, image=buf, num_rendered=1, width=16, height=16)
    with pytest.raises(RuntimeError, match="HIP device"):
        c.add_view(view)
    with pytest.raises(ValueError, match="lack"):
        c.add_view(dict(geom=buf))
    with pytest.raises(ValueError):
        SP.Contribution(-1, "cpu")
    # the entry itself: checked before any device is touched
    p = n.C.c_void_p(256)
    for args, msg in (((4, 1, 0, 16, p, p, p, 1, p, p, p, p, p, p, None, 0), "bad sizes"), ((4, -1, 16, 16, p, p, p, 1, p, p, p, p, p, p, None, 0), "bad sizes"),
                      ((4, 1, 16, 16, p, p, p, 0, p, p, p, p, p, p, None, 0), "view_tag"), ((4, 1, 16, 16, None, p, p, 1, p, p, p, p, p, p, None, 0), "buffer is NULL"),
                      ((4, 1, 16, 16, p, p, p, 1, p, None, p, p, p, p, None, 0), "accumulator")):
        with pytest.raises(RuntimeError, match=r"\(-1\): .*" + msg):
            n.call(None, "surfel_rasterize_contribution", *args)
    assert n.call(None, "surfel_rasterize_contribution", 0, 5, 16, 16, None, None, None, 1, None, None, None, None, None, None, None, 0) == 0      # P == 0
    assert n.call(None, "surfel_rasterize_contribution", 4, 0, 16, 16, None, None, None, 1, None, None, None, None, None, None, None, 0) == 0      # R == 0
    with pytest.raises(RuntimeError, match="HIP device"):      # a host tensor never reaches a device-pointer parameter
        n.call(None, "surfel_rasterize_contribution", 4, 1, 16, 16, buf, buf, buf, 1, buf, buf, buf, buf, buf, buf, None, 0)
    with pytest.raises(ValueError):
        SP.prune_model(type("M", (), {"P": 4})(), torch.ones(3, dtype=torch.bool))


def test_trainer_flags_are_opt_in():
    import surfel_trainer as TR
    a = TR.parse_args(["-s", "x", "-m", "y"])
    assert a.prune_at == [] and a.prune_min_max_weight is None and a.prune_min_views is None
    a = TR.parse_args(["-s", "x", "-m", "y", "--prune_at", "40", "80", "--prune_min_max_weight", "0.01", "--prune_min_views", "2"])
    assert a.prune_at == [40, 80] and a.prune_min_max_weight == 0.01 and a.prune_min_views == 2
    import surfel_prune as SP
    b = SP.build_parser().parse_args(["-m", "y", "--keep_ratio", "0.5", "--score", "max", "--report"])
    assert b.keep_ratio == 0.5 and b.score == "max" and b.report and b.out is None and b.source_path is None


# ------------------------------------------------------------------------------------------------ library surface
def test_contrib_header_exported_and_signature_matches():
    """include/surfel_contrib.h <-> SIGNATURES["surfel_contrib.h"] <-> the library's export (as test_abi_cpu does for its headers)"""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib_path = os.path.join(PKG, "lib", "libsurfel_hip.so")
    assert os.path.exists(lib_path), "libsurfel_hip.so not built: run __graft_entry__.build()"
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 1
    assert [p[0] for p in protos] == list(n.SIGNATURES[HEADER]) == n.CONTRIB_EXPORTS == ["surfel_rasterize_contribution"]
    others = [name for h, group in n.SIGNATURES.items() if h != HEADER for name in group]
    assert "surfel_rasterize_contribution" not in others
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    assert "surfel_rasterize_contribution" in set(re.findall(r" T (\w+)$", out, re.M))
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    name, ret, params = protos[0]
    fn = getattr(lib, name)
    assert ret == "int" and fn.restype is C.c_int
    assert fn.argtypes is not None and len(fn.argtypes) == len(params) == 17
    for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
        where = (k, ctype, pname, at)
        if ctype in scalars:
            assert at is scalars[ctype], where
        else:
            assert ctype.endswith("*"), where
            assert (at is n.DevPtr) == (pname != "stream"), where      # every pointer of this header is a device pointer
        assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
    assert [p[1] for p in params][7:15] == ["view_tag", "sum_q", "hits", "max_bits", "dominant", "views", "stamp", "dominant_id"]
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_contrib", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "surfel_contrib.hip" in mod.SOURCES and mod.EXTRA["surfel_contrib.hip"] == mod.EXTRA["surfel_forward.hip"] and any(h.endswith(HEADER) for h in mod.HEADERS)
    import surfel_prune as SP
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    assert int(re.search(r"#define SURFEL_CONTRIB_FRAC_BITS (\d+)", hdr).group(1)) == SP.FRAC_BITS == 24


def test_existing_rasterizer_sources_are_untouched_by_the_pass():
    """the pass adds nothing to the rasterizer's own files; the walk's definitions reach it through surfel_tile_walk.h alone, which
    takes them from surfel_common.h: no private copy of the walk in either pass"""
    csrc = os.path.join(PKG, "csrc")
    for f in ("surfel_forward.hip", "surfel_backward.hip", "surfel_backward_scan.hip", "surfel_preprocess.hip", "surfel_sort.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert "surfel_contrib" not in txt and "ContribArgs" not in txt and "surfel_tile_walk" not in txt, f
    walk = open(os.path.join(csrc, "surfel_tile_walk.h")).read()
    for shared in ("pair_hit(", "make_foot(", "subtile_overlap(", "thread_pixel(", "block_tile("):
        assert shared in walk, shared
    assert "T_EPS" in walk and '#include "surfel_common.h"' in walk
    for f in ("surfel_contrib.hip", "surfel_select.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "surfel_tile_walk.h"' in src and "tile_walk(" in src, f
        for private in ("pair_hit(", "make_foot(", "subtile_overlap(", "thread_pixel(", "block_tile(", "T_EPS"):
            assert private not in src, (f, private)
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_walk", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "surfel_tile_walk.h" in mod.HEADERS
    src = open(os.path.join(csrc, "surfel_contrib.hip")).read()
    assert "atomicAdd(&a.sum_q" in src and "float*" not in src.split("contrib_kernel(ContribArgs a)")[1]      # integer accumulators only
