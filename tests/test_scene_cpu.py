"""CPU tests of the capture loader (SCENE.md): the numpy oracle against Pillow, the library's host tables against the oracle, the
resolution rule, the COLMAP / Blender readers against what the reference's readers returned on the same captures (tests/golden/ref_scene.npz,
minted by tests/golden/make_golden_scene.py), the C ABI, and the training CLI's arguments.  Nothing here touches a device."""
import argparse
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import scene_oracle as SO
import scene_scenes as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# H, W -> H2, W2 (shared with tests/test_gpu_scene.py)
SHAPES = [(37, 53, 13, 20), (64, 64, 32, 32), (101, 77, 50, 77), (17, 19, 17, 9), (40, 30, 55, 47), (2, 3, 9, 11), (67, 131, 8, 16),
          (9, 1601, 5, 1600), (33, 1, 7, 1), (1, 40, 1, 7), (5, 5, 1, 1)]


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(REPO, "tests", "golden", "ref_scene.npz"))


# ------------------------------------------------------------------------------------------------ 1. the oracle is Pillow
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_oracle_is_bit_equal_to_pillow(shape):
    Image = pytest.importorskip("PIL.Image")
    H, W, H2, W2 = shape
    for Cn in (1, 3, 4):
        a = SS.noise_image(1000 + Cn, H, W, Cn)
        got, _ = SO.resize(a, W2, H2)
        if Cn == 3:
            want = np.asarray(Image.fromarray(a).resize((W2, H2)))                  # no filter given: BICUBIC, as the reference calls it
        else:                                                                         # independent "L" images, as the reference splits RGBA
            want = np.stack([np.asarray(Image.fromarray(a[:, :, c]).resize((W2, H2))) for c in range(Cn)], axis=2)
        assert got.shape == want.shape and np.array_equal(got, want), (shape, Cn)


# ------------------------------------------------------------------------------------------------ 2. host tables
def test_host_tables_equal_the_oracle():
    import surfel_scene
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 41)] + [(1600, 800), (5187, 1600), (1601, 1599)]
    for i, o in pairs:
        ksize, bounds, coeffs = surfel_scene.resample_tables(i, o)
        k2, b2, c2 = SO.tables(i, o)
        assert ksize == k2 and np.array_equal(bounds, b2) and np.array_equal(coeffs.T, c2), (i, o)
    assert surfel_scene.resample_tables(1600, 800)[0] == 9 and surfel_scene.resample_tables(30, 47)[0] == 5


def test_table_limits_and_errors():
    import surfel_native as n
    assert n.call(None, "surfel_scene_resample_table", 4800, 100, None, None, 0) == 193       # 48 x: the stated cap
    with pytest.raises(n.LimitError, match="ksize"):
        n.call(None, "surfel_scene_resample_table", 4900, 100, None, None, 0)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        n.call(None, "surfel_scene_resample_table", 0, 100, None, None, 0)
    b, c = (C.c_int * 8)(), (C.c_int * 8)()
    with pytest.raises(RuntimeError, match="fewer than"):
        n.call(None, "surfel_scene_resample_table", 8, 4, b, c, 8)


# ------------------------------------------------------------------------------------------------ 3. resolution rule
def test_resolution_rule(ref):
    import surfel_scene
    widths = ref["rule/widths"].tolist()
    for r in (-1, 1, 2, 4, 8, 20, 777):
        for w, (w2, h2) in zip(widths, ref["rule/r%d" % r].tolist()):
            assert surfel_scene.target_resolution(w, 701, r) == (w2, h2), (r, w)
    assert surfel_scene.target_resolution(53, 55, 2) == (26, 28)          # round half to even
    narrow = []
    for w in range(1601, 4001):
        got = surfel_scene.target_resolution(w, 1200, -1)
        assert got == SO.target_resolution(w, 1200, -1), w
        if got[0] != 1600:
            narrow.append(w)
    assert narrow[:5] == [1601, 1610, 1617, 1619, 1626] and all(surfel_scene.target_resolution(w, 1200, -1)[0] == 1599 for w in narrow)


# ------------------------------------------------------------------------------------------------ 4. readers
TOL = dict(atol=1e-12, rtol=1e-12)


def _check_infos(infos, ref, tag):
    assert [c.image_name for c in infos] == ref[tag + "/names"].tolist()
    assert [c.uid for c in infos] == ref[tag + "/uid"].tolist()
    assert [[c.width, c.height] for c in infos] == ref[tag + "/wh"].tolist()
    assert np.array_equal(np.stack([c.T for c in infos]), ref[tag + "/T"])
    np.testing.assert_allclose(np.stack([c.R for c in infos]), ref[tag + "/R"], **TOL)
    np.testing.assert_allclose(np.array([[c.FovX, c.FovY] for c in infos]), ref[tag + "/fov"], **TOL)


def _check_split(info, ref, tag):
    import surfel_scene
    np.testing.assert_allclose(info.nerf_normalization["translate"], ref[tag + "/translate"], **TOL)
    np.testing.assert_allclose(float(info.nerf_normalization["radius"]), float(ref[tag + "/radius"]), **TOL)
    got = [surfel_scene.camera_to_json(i, c) for i, c in enumerate(list(info.test_cameras) + list(info.train_cameras))]
    want = json.loads(str(ref[tag + "/cameras_json"]))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        assert (g["id"], g["img_name"], g["width"], g["height"]) == (w["id"], w["img_name"], w["width"], w["height"])
        for key in ("position", "rotation", "fx", "fy"):
            np.testing.assert_allclose(np.asarray(g[key]), np.asarray(w[key]), **TOL)
    json.dumps(got)      # serialisable as it stands


@pytest.mark.parametrize("fmt", ["bin", "txt"])
def test_colmap_reader_matches_the_reference(tmp_path, ref, fmt):
    import surfel_io
    import surfel_scene
    root = str(tmp_path / "capture")
    SS.write_colmap(root, fmt)
    for ev in (False, True):
        info = surfel_scene.read_scene_info(root, "images", eval=ev)
        tag = "colmap/eval%d" % ev
        assert [c.image_name for c in info.train_cameras] == ref[tag + "/train"].tolist()
        assert [c.image_name for c in info.test_cameras] == ref[tag + "/test"].tolist()
        if ev:
            assert [c.image_name for c in info.test_cameras] == ["view_00", "view_09"] and len(info.train_cameras) == 7
        else:
            _check_infos(info.train_cameras, ref, "colmap/cams")
            assert not any(c.composite for c in info.train_cameras)
        _check_split(info, ref, tag)
    # the points3D conversion, exact
    assert info.ply_path.endswith("sparse/0/points3D.ply") and os.path.exists(info.ply_path)
    assert info.point_cloud.points.dtype == np.float32 and np.array_equal(info.point_cloud.points, ref["colmap/points"])
    assert np.array_equal(info.point_cloud.colors, ref["colmap/colors_u8"] / 255.0) and not np.any(info.point_cloud.normals)
    raw = surfel_io.read_ply(info.ply_path)
    assert list(raw) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and raw["red"].dtype == np.uint8 and raw["x"].dtype == np.float32


def test_colmap_bin_and_txt_are_identical(tmp_path):
    import surfel_scene
    infos = []
    for fmt in ("bin", "txt"):
        root = str(tmp_path / fmt)
        SS.write_colmap(root, fmt)
        infos.append(surfel_scene.read_scene_info(root, "images", eval=True))
    a, b = infos
    for ca, cb in zip(a.train_cameras + a.test_cameras, b.train_cameras + b.test_cameras):
        assert ca.image_name == cb.image_name and ca.uid == cb.uid and (ca.width, ca.height, ca.FovX, ca.FovY) == (cb.width, cb.height, cb.FovX, cb.FovY)
        assert np.array_equal(ca.R, cb.R) and np.array_equal(ca.T, cb.T)
    assert np.array_equal(a.point_cloud.points, b.point_cloud.points) and np.array_equal(a.point_cloud.colors, b.point_cloud.colors)
    assert np.array_equal(a.nerf_normalization["translate"], b.nerf_normalization["translate"])


def test_colmap_reader_refuses_distorted_models(tmp_path):
    import surfel_scene
    root = str(tmp_path / "capture")
    SS.write_colmap(root, "txt")
    path = os.path.join(root, "sparse", "0", "cameras.txt")
    text = open(path).read().replace("SIMPLE_PINHOLE", "SIMPLE_RADIAL")
    open(path, "w").write(text)
    with pytest.raises(ValueError, match="SIMPLE_RADIAL.*undistort"):
        surfel_scene.read_scene_info(root, "images")
    with pytest.raises(ValueError, match="could not recognize"):
        surfel_scene.read_scene_info(str(tmp_path))


def test_blender_reader_matches_the_reference(tmp_path, ref):
    import surfel_scene
    root = SS.write_blender(str(tmp_path / "lego"))
    for ev in (False, True):
        info = surfel_scene.read_scene_info(root, white_background=False, eval=ev, seed=0)
        tag = "blender/eval%d" % ev
        assert len(info.train_cameras) == int(ref[tag + "/n_train"]) == (4 if ev else 6) and len(info.test_cameras) == (2 if ev else 0)
        _check_infos(list(info.train_cameras) + list(info.test_cameras), ref, "blender/cams")
        assert all(c.composite for c in info.train_cameras)
        _check_split(info, ref, tag)
    pts = info.point_cloud.points
    assert pts.shape[0] == int(ref["blender/points_n"]) == 100_000 and np.array_equal(pts[:64], ref["blender/points_head"])
    assert np.array_equal(pts.astype(np.float64).sum(0), ref["blender/points_sum"])
    assert np.array_equal(np.round(info.point_cloud.colors[:64] * 255.0).astype(np.uint8), ref["blender/colors_head"])
    assert np.abs(pts).max() <= 1.3


def test_decode_refuses_what_pillow_resamples_differently():
    Image = pytest.importorskip("PIL.Image")
    import surfel_scene
    for mode in ("P", "1", "I;16", "LA", "F"):
        with pytest.raises(ValueError, match="not supported"):
            surfel_scene.decode(Image.new(mode, (4, 3)))
    assert surfel_scene.decode(Image.new("L", (4, 3))).shape == (3, 4, 1) and surfel_scene.decode(Image.new("RGBA", (4, 3))).shape == (3, 4, 4)


def test_oracle_composite_truncates():
    """the 256 x 256 (colour, alpha) table: truncation, not rounding (they differ in about half of the pairs)"""
    v = np.arange(256, dtype=np.uint8)
    rgba = np.zeros((256, 256, 4), np.uint8)
    rgba[:, :, :3] = v[:, None, None]
    rgba[:, :, 3] = v[None, :]
    for white in (False, True):
        out = SO.composite(rgba, white)
        n = rgba.astype(np.float64) / 255.0
        exact = (n[:, :, :3] * n[:, :, 3:4] + float(white) * (1 - n[:, :, 3:4])) * 255.0
        assert np.array_equal(out, np.floor(exact).astype(np.uint8))
        assert 20000 < int((out[:, :, 0] != np.round(exact[:, :, 0]).astype(np.uint8)).sum()) < 40000
        assert np.array_equal(out[:, 255], rgba[:, 255, :3]) and np.all(out[:, 0] == (255 if white else 0))


# ------------------------------------------------------------------------------------------------ 5. C ABI
def test_scene_header_signatures_and_exports():
    """include/surfel_scene.h <-> SIGNATURES["surfel_scene.h"] <-> the library's exports (as test_abi_cpu does for the other headers)"""
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_scene.h")
    assert len(protos) == mentions == 5
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_scene.h"]) == sorted(n.SCENE_EXPORTS)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert C.cast(fn, C.c_void_p).value and fn.restype is C.c_int and ret == "int"
        assert len(fn.argtypes) == len(params), name
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            elif ctype == "int*" and name == "surfel_scene_resample_table":
                assert at is C.POINTER(C.c_int), where          # host tables
            else:
                assert ctype.endswith("*") and at is (n.Stream if pname == "stream" else n.DevPtr), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
    hdr = open(os.path.join(REPO, "include", "surfel_scene.h")).read()
    assert int(re.search(r"#define SURFEL_SCENE_MAX_KSIZE (\d+)", hdr).group(1)) >= 67
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "scene_image.hip" in mod.SOURCES and any(h.endswith("surfel_scene.h") for h in mod.HEADERS)


# ------------------------------------------------------------------------------------------------ 6. training CLI
def test_cli_arguments_and_cfg_args_roundtrip(tmp_path):
    import surfel_trainer as TR
    args = TR.parse_args(["-s", "data/scan24", "-m", str(tmp_path / "out")])
    assert args.source_path == os.path.abspath("data/scan24") and args.images == "images" and args.resolution == -1
    assert args.white_background is False and args.eval is False and args.sh_degree == 3 and args.data_device == "cuda"
    assert args.iterations == 30_000 and args.test_iterations == [7_000, 30_000] and args.save_iterations == [7_000, 30_000, 30_000]
    assert args.checkpoint_iterations == [] and args.start_checkpoint is None and args.quiet is False and args.seed == 0
    assert args.depth_ratio == 0.0 and args.lambda_dist == 0.0 and args.lambda_normal == 0.05 and args.densify_grad_threshold == 0.0002
    assert not hasattr(args, "ip") and not hasattr(args, "port")
    defaults = vars(TR.optimization_params())
    opt = TR.optimization_from_args(args)
    assert vars(opt) == defaults
    args = TR.parse_args(["-s", "x", "-m", str(tmp_path / "m"), "-i", "images_4", "-r", "2", "-w", "--eval", "--sh_degree", "2", "--iterations", "300",
                          "--save_iterations", "100", "200", "--test_iterations", "50", "--checkpoint_iterations", "300", "--quiet", "--seed", "7",
                          "--depth_ratio", "1.0", "--lambda_dist", "100", "--position_lr_init", "0.0002", "--densify_until_iter", "200"])
    assert (args.images, args.resolution, args.white_background, args.eval, args.sh_degree, args.seed) == ("images_4", 2, True, True, 2, 7)
    assert args.save_iterations == [100, 200, 300] and args.test_iterations == [50] and args.checkpoint_iterations == [300] and args.quiet
    opt = TR.optimization_from_args(args)
    assert (opt.iterations, opt.lambda_dist, opt.position_lr_init, opt.densify_until_iter) == (300, 100.0, 0.0002, 200)
    assert opt.dist_from_iter == defaults["dist_from_iter"]
    # cfg_args: str(Namespace(...)) that evaluates back (what the reference's get_combined_args does with it)
    path = TR.write_cfg_args(args)
    assert path == os.path.join(args.model_path, "cfg_args")
    back = eval(open(path).read(), {"Namespace": argparse.Namespace})
    assert isinstance(back, argparse.Namespace)
    assert vars(back) == dict(sh_degree=2, source_path=os.path.abspath("x"), model_path=args.model_path, images="images_4", resolution=2,
                              white_background=True, data_device="cuda", eval=True)
    with pytest.raises(SystemExit):
        TR.parse_args(["-s", "x", "--port", "6009"])
