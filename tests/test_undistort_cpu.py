"""Host checks of the undistortion (UNDISTORT.md): the camera rule of the product (surfel_undistort.py) against the numpy oracle
(tests/undistort_oracle.py) and against the sizes written down with the rule, a geometry anchor that shares no formulation with the
forward map, the invalid-pixel rule, the reader's flag and folder layout, the C ABI and the CLIs' flags.  No GPU is needed."""
import argparse
import ctypes as C
import math
import os
import re
import shutil

import numpy as np
import pytest

import scene_scenes as SS
import undistort_oracle as UO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the captures of scene_scenes.write_colmap with their camera lines rewritten: camera 1 is 53 x 37 (RGB files), camera 2 48 x 36 (RGBA)
CAPTURE_CAMERAS = {
    "SIMPLE_RADIAL": {1: ("SIMPLE_RADIAL", (61.25, 26.5, 18.5, 0.1))},
    "RADIAL": {1: ("RADIAL", (61.25, 26.3, 18.7, -0.12, 0.03))},
    "OPENCV": {1: ("OPENCV", (61.25, 60.5, 26.2, 18.9, -0.15, 0.05, 0.002, -0.003))},
    "FULL_OPENCV": {1: ("FULL_OPENCV", (61.25, 60.5, 26.2, 18.9, 0.1, 0.02, 0.001, -0.002, 0.003, 0.2, 0.03, 0.001))},
    "both": {1: ("SIMPLE_RADIAL", (61.25, 26.5, 18.5, 0.1)), 2: ("OPENCV", (52.5, 51.75, 24.3, 17.8, -0.1, 0.03, 0.001, -0.002))},
}


def rewrite_cameras(root, cameras, sparse="sparse/0"):
    """root/<sparse>/cameras.txt of a write_colmap(root, "txt") capture with the lines of `cameras` = {id: (model, params)} replaced"""
    path = os.path.join(root, sparse, "cameras.txt")
    lines = []
    for line in open(path).read().splitlines():
        e = line.split()
        if e and e[0].isdigit() and int(e[0]) in cameras:
            model, params = cameras[int(e[0])]
            line = "%s %s %s %s %s" % (e[0], model, e[2], e[3], " ".join(repr(float(v)) for v in params))
        lines.append(line)
    open(path, "w").write("\n".join(lines) + "\n")


def to_convert_layout(root):
    """images/ -> input/, sparse/0 -> distorted/sparse/0: what convert.py has before its undistortion step"""
    os.rename(os.path.join(root, "images"), os.path.join(root, "input"))
    os.makedirs(os.path.join(root, "distorted"))
    os.rename(os.path.join(root, "sparse"), os.path.join(root, "distorted", "sparse"))


def _size(cid):
    return SS.COLMAP_CAMERAS[cid][1], SS.COLMAP_CAMERAS[cid][2]


# ------------------------------------------------------------------------------------------------ 1. the camera rule
def test_parameter_vector_of_every_model():
    import surfel_undistort as SU
    assert SU.distortion_params("SIMPLE_RADIAL", (60, 33.5, 24.2, 0.12)).tolist() == [60, 60, 33.5, 24.2, 0.12, 0, 0, 0, 0, 0, 0, 0]
    assert SU.distortion_params("RADIAL", (300, 161, 119, -0.15, 0.04)).tolist() == [300, 300, 161, 119, -0.15, 0.04, 0, 0, 0, 0, 0, 0]
    assert SU.distortion_params("OPENCV", (1, 2, 3, 4, 5, 6, 7, 8)).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 0, 0, 0, 0]
    assert SU.distortion_params("FULL_OPENCV", range(1, 13)).tolist() == list(range(1, 13))
    for model, params in (("OPENCV_FISHEYE", range(8)), ("FOV", range(5)), ("THIN_PRISM_FISHEYE", range(12)), ("PINHOLE", range(4)), ("RADIAL", range(4)),
                          ("SIMPLE_RADIAL", (-60, 1, 1, 0)), ("SIMPLE_RADIAL", (60, 1, float("nan"), 0))):
        with pytest.raises(ValueError):
            SU.distortion_params(model, params)
    for model, params, _, _, _ in UO.CAMERAS:
        assert np.array_equal(SU.distortion_params(model, params), UO.distortion_params(model, params))


def _all_fixtures():
    out = [(m, p, w, h, want) for m, p, w, h, want in UO.CAMERAS]
    for cams in CAPTURE_CAMERAS.values():
        out += [(m, p) + _size(cid) + (None,) for cid, (m, p) in cams.items()]
    return out


def test_camera_rule_matches_the_oracle_and_the_written_sizes():
    import surfel_undistort as SU
    for model, params, W, H, want in _all_fixtures():
        q = SU.distortion_params(model, params)
        got, ref = SU.undistorted_camera(q, W, H), UO.undistorted_camera(UO.distortion_params(model, params), W, H)
        assert got[:2] == ref[:2] and (want is None or got[:2] == want), (model, params, got, ref, want)
        assert got[2:4] == (q[0], q[1]) and got[4] == q[2] * got[0] / W and got[5] == q[3] * got[1] / H
        assert np.allclose(got[2:], ref[2:], rtol=1e-12, atol=0)
        # the Newton tolerance (1e-12 in ray coordinates) cannot flip a size: the scaled sizes stay clear of every integer
        sx, sy = UO.camera_scales(q, W, H)
        for v in (sx * W, sy * H):
            assert abs(v - round(v)) >= 1e-6, (model, params, v)
        assert SU.undistorted_camera(q, W, H, blank=0.0) == got


def test_inverse_inverts_and_refuses_what_is_no_lens():
    import surfel_undistort as SU
    for model, params, W, H, _ in UO.CAMERAS:
        q = UO.distortion_params(model, params)
        x, y = np.meshgrid(np.linspace(0.5, W - 0.5, 9), np.linspace(0.5, H - 0.5, 7))
        ud, vd = (x - q[2]) / q[0], (y - q[3]) / q[1]
        u, v = SU.undistort_points(q, ud, vd)
        bu, bv = UO.distort(q, u, v)
        assert np.abs(bu - ud).max() < 1e-11 and np.abs(bv - vd).max() < 1e-11
        ou, ov = UO.undistort_points(q, ud, vd)
        assert np.abs(ou - u).max() < 1e-10 and np.abs(ov - v).max() < 1e-10
    # u * (1 - 5 r^2) never reaches 0.55: there is nothing to converge to
    with pytest.raises(ValueError, match="did not converge"):
        SU.undistorted_camera(SU.distortion_params("SIMPLE_RADIAL", (60, 33.5, 24.2, -5.0)), 67, 49)


# ------------------------------------------------------------------------------------------------ 2. geometry anchor
def test_pattern_painted_through_the_inverse_comes_back_undistorted():
    """A smooth pattern of the undistorted ray direction is painted into the distorted image through the Newton inverse at every
    distorted pixel centre; undistorting it must give the pattern as the undistorted pinhole sees it.  Measured on the five cameras:
    at most 0.99 levels (two roundings to 8 bits and the bilinear error), mean 0.29; the bound is 2 levels, and at blank = 0 no
    output pixel may look outside the source."""
    for model, params, W, H, _ in UO.CAMERAS:
        q = UO.distortion_params(model, params)
        W2, H2, fx, fy, cx2, cy2 = UO.undistorted_camera(q, W, H)
        out, valid = UO.undistort(UO.paint_distorted(q, W, H), q, (fx, fy, cx2, cy2), (W2, H2), return_valid=True)
        x, y = np.meshgrid(np.arange(W2) + 0.5, np.arange(H2) + 0.5)
        want = UO.pattern((x - cx2) / fx, (y - cy2) / fy)
        err = np.abs(out.astype(np.float64) - want)
        print("%s: max %.3f mean %.3f levels, %d invalid" % (model, err.max(), err.mean(), int((~valid).sum())))
        assert valid.all() and err.max() <= 2.0, (model, err.max())


# ------------------------------------------------------------------------------------------------ 3. invalid pixels
FORCED = dict(model="SIMPLE_RADIAL", params=(60, 33.5, 24.2, -0.08), W=67, H=49, size=(90, 70), pinhole=(60.0, 60.0, 45.0, 35.0), invalid=2958)


# finite parameters whose formula overflows at every output pixel (the pinhole puts every ray at r2 >= 1e8, so r6 * 1e300 is infinite)
OVERFLOW = {
    "inf_denominator": ((60, 60, 33.5, 24.2, 0.1, 0, 0, 0, 0, 0, 0, 1e300), (1e-3, 1e-3, -10.0, -10.0)),
    "inf_over_inf": ((60, 60, 33.5, 24.2, 0.1, 0, 0, 0, 1e300, 0, 0, 1e300), (1e-3, 1e-3, -10.0, -10.0)),
    "inf_numerator": ((60, 60, 33.5, 24.2, 0.1, 0, 0, 0, 1e300, 0, 0, 0), (1e-3, 1e-3, -10.0, -10.0)),
}


def test_pixels_that_look_outside_the_source_are_zero():
    q = UO.distortion_params(FORCED["model"], FORCED["params"])
    W, H = FORCED["W"], FORCED["H"]
    src = SS.noise_image(5, H, W, 4)
    src[src == 0] = 1                       # so that a zero in the result can only be an invalid pixel
    out, valid = UO.undistort(src, q, FORCED["pinhole"], FORCED["size"], return_valid=True)
    assert out.shape == (70, 90, 4) and int((~valid).sum()) == FORCED["invalid"]
    assert not out[~valid].any() and out[valid].all()      # every channel, the alpha too
    assert not valid[0].any() and not valid[-1].any() and not valid[:, 0].any() and not valid[:, -1].any()      # all four sides
    xs, ys = UO.source_coordinates(q, FORCED["pinhole"], FORCED["size"])
    x0, y0 = np.floor(xs[valid]), np.floor(ys[valid])
    assert x0.min() >= 0 and (x0 + 1).max() == W - 1 and y0.min() >= 0 and (y0 + 1).max() <= H - 1      # the x0 + 1 == W - 1 edge is met
    # overflow: a denominator that is infinite under a finite numerator gives rad = 0, every pixel samples the principal point; with
    # the numerator infinite too the coordinates are NaN, with the numerator alone infinite: all of those pixels are invalid
    for name, (q_over, ph_over) in OVERFLOW.items():
        out = UO.undistort(src, UO.distortion_params("FULL_OPENCV", q_over), ph_over, FORCED["size"])
        if name == "inf_denominator":
            assert (out == out[0, 0]).all() and out.all()
        else:
            assert not out.any(), name


# ------------------------------------------------------------------------------------------------ 4. the reader
def _capture(tmp_path, key, name="capture"):
    root = str(tmp_path / name)
    SS.write_colmap(root, "txt")
    rewrite_cameras(root, CAPTURE_CAMERAS[key])
    return root


@pytest.mark.parametrize("key", ["SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV", "both"])
def test_reader_undistorts_with_the_flag_only(tmp_path, key):
    import surfel_scene
    root = _capture(tmp_path, key)
    with pytest.raises(ValueError, match="%s.*undistort" % CAPTURE_CAMERAS[key][1][0]):
        surfel_scene.read_scene_info(root, "images")
    with pytest.raises(ValueError, match="undistort"):
        surfel_scene.read_colmap_scene(root, undistort=False)
    info = surfel_scene.read_scene_info(root, "images", eval=True, undistort=True)
    plain = str(tmp_path / "plain")
    SS.write_colmap(plain, "txt")
    base = surfel_scene.read_scene_info(plain, "images", eval=True)
    assert [c.image_name for c in info.train_cameras] == [c.image_name for c in base.train_cameras]
    assert [c.image_name for c in info.test_cameras] == [c.image_name for c in base.test_cameras]
    seen = set()
    for c, b in zip(list(info.train_cameras) + list(info.test_cameras), list(base.train_cameras) + list(base.test_cameras)):
        assert np.array_equal(c.R, b.R) and np.array_equal(c.T, b.T) and c.uid == b.uid and c.image_path == os.path.join(root, "images", os.path.basename(b.image_path)) and not c.composite
        if c.uid not in CAPTURE_CAMERAS[key]:      # a pinhole camera never passes through any of this
            assert c.distortion is None and c.pinhole is None and c.source_size is None and (c.width, c.height, c.FovX, c.FovY) == (b.width, b.height, b.FovX, b.FovY)
            continue
        seen.add(c.uid)
        model, params = CAPTURE_CAMERAS[key][c.uid]
        q = UO.distortion_params(model, params)
        W2, H2, fx, fy, cx2, cy2 = UO.undistorted_camera(q, *_size(c.uid))
        assert (c.width, c.height) == (W2, H2) and c.source_size == _size(c.uid)
        assert c.FovX == 2 * math.atan(W2 / (2 * fx)) and c.FovY == 2 * math.atan(H2 / (2 * fy))
        assert np.array_equal(c.distortion, q) and np.allclose(c.pinhole, (fx, fy, cx2, cy2), rtol=1e-12, atol=0)
    assert seen == set(CAPTURE_CAMERAS[key])


def test_camera_info_keeps_its_constructions():
    import surfel_scene
    c = surfel_scene.CameraInfo(0, np.eye(3), np.zeros(3), 1.0, 1.0, "a.png", "a", 4, 3)
    assert (c.composite, c.distortion, c.pinhole, c.source_size) == (False, None, None, None)
    assert surfel_scene.CameraInfo._fields[9:] == ("composite", "distortion", "pinhole", "source_size")


def test_reader_finds_the_convert_layout_and_still_refuses_fisheye(tmp_path):
    import surfel_scene
    root = _capture(tmp_path, "SIMPLE_RADIAL")
    want = surfel_scene.read_scene_info(root, "images", undistort=True)
    to_convert_layout(root)
    with pytest.raises(ValueError, match="could not recognize"):
        surfel_scene.read_scene_info(root, "images")                       # without the flag distorted/sparse is no capture
    got = surfel_scene.read_scene_info(root, "images", undistort=True)     # -i names no folder: input/
    assert os.path.exists(os.path.join(root, "distorted/sparse/0/points3D.ply")) and not os.path.exists(os.path.join(root, "sparse"))
    for a, b in zip(want.train_cameras, got.train_cameras):
        assert a.image_name == b.image_name and (a.width, a.height, a.FovX, a.FovY) == (b.width, b.height, b.FovX, b.FovY)
        assert b.image_path == os.path.join(root, "input", os.path.basename(a.image_path)) and os.path.exists(b.image_path)
    assert np.array_equal(want.point_cloud.points, got.point_cloud.points)
    # an -i folder that exists wins over input/
    shutil.copytree(os.path.join(root, "input"), os.path.join(root, "images_2"))
    assert all(c.image_path.startswith(os.path.join(root, "images_2")) for c in surfel_scene.read_scene_info(root, "images_2", undistort=True).train_cameras)
    # the models that need atan stay refused, with the flag too
    for model, params in (("OPENCV_FISHEYE", (61.25, 60.5, 26.2, 18.9, 0.01, 0.0, 0.0, 0.0)), ("FOV", (61.25, 60.5, 26.2, 18.9, 0.5)),
                          ("THIN_PRISM_FISHEYE", (61.25, 60.5, 26.2, 18.9) + (0.0,) * 8), ("SIMPLE_RADIAL_FISHEYE", (61.25, 26.2, 18.9, 0.01))):
        rewrite_cameras(root, {1: (model, params)}, "distorted/sparse/0")
        with pytest.raises(ValueError, match="%s is not supported" % model):
            surfel_scene.read_scene_info(root, "images", undistort=True)


# ------------------------------------------------------------------------------------------------ 5. C ABI and build
def test_undistort_header_signature_and_export():
    """include/surfel_undistort.h <-> SIGNATURES["surfel_undistort.h"] <-> UNDISTORT_EXPORTS <-> the library's export"""
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_undistort.h")
    assert len(protos) == mentions == 1
    assert [p[0] for p in protos] == list(n.SIGNATURES["surfel_undistort.h"]) == n.UNDISTORT_EXPORTS == ["surfel_scene_undistort"]
    name, ret, params = protos[0]
    fn = getattr(lib, name)
    assert C.cast(fn, C.c_void_p).value and fn.restype is C.c_int and ret == "int" and len(fn.argtypes) == len(params) == 10
    for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
        where = (k, ctype, pname, at)
        if ctype == "int":
            assert at is C.c_int, where
        elif ctype == "double*":
            assert pname in ("q", "pinhole") and at is C.POINTER(C.c_double), where      # host arrays, passed on by value
        else:
            assert ctype in ("uint8_t*", "void*") and at is (n.Stream if pname == "stream" else n.DevPtr), where
    assert params[-1][1] == "stream"
    others = [name for h, group in n.SIGNATURES.items() if h != "surfel_undistort.h" for name in group]
    assert "surfel_scene_undistort" not in others
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "scene_undistort.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["scene_undistort.hip"]
    assert any(h.endswith("surfel_undistort.h") for h in mod.HEADERS)


def test_entry_refuses_bad_arguments_before_any_launch():
    """the argument checks run on the host, before the launch: no device is touched by a refused call"""
    import surfel_native as n
    lib = n.load()
    q = (C.c_double * 12)(60, 60, 33.5, 24.2, 0.1, 0, 0, 0, 0, 0, 0, 0)
    ph = (C.c_double * 4)(60, 60, 30, 20)
    fake = C.c_void_p(4096)      # never dereferenced: every call below is refused

    def rc(H=49, W=67, Cn=3, H2=40, W2=60, q=q, ph=ph, src=fake, dst=fake):
        return lib.surfel_scene_undistort(H, W, Cn, H2, W2, q, ph, src, dst, None)
    E_INVALID = rc(Cn=2)
    assert E_INVALID < 0 and E_INVALID != n.E_LIMIT and "scene_undistort" in n.last_error()
    for kw in (dict(Cn=0), dict(Cn=5), dict(H=0), dict(W2=0), dict(H2=-1), dict(src=None), dict(dst=None), dict(q=None), dict(ph=None)):
        assert rc(**kw) == E_INVALID, kw
    for kw in (dict(H=32769), dict(W=32769), dict(H2=32769), dict(W2=40000)):
        assert rc(**kw) == n.E_LIMIT, kw
    for k, bad in ((4, float("nan")), (11, float("inf")), (0, 0.0), (1, -1.0), (2, float("-inf"))):
        qq = (C.c_double * 12)(*q)
        qq[k] = bad
        assert rc(q=qq) == E_INVALID, (k, bad)
    for k, bad in ((0, 0.0), (1, float("nan")), (3, float("inf"))):
        pp = (C.c_double * 4)(*ph)
        pp[k] = bad
        assert rc(ph=pp) == E_INVALID, (k, bad)


# ------------------------------------------------------------------------------------------------ 6. the CLIs
def test_cli_flags_and_cfg_args(tmp_path):
    import surfel_convert
    import surfel_mesh
    import surfel_trainer as TR
    args = TR.parse_args(["-s", "x", "-m", str(tmp_path / "plain")])
    assert args.undistort is False
    back = eval(open(TR.write_cfg_args(args)).read(), {"Namespace": argparse.Namespace})
    assert "undistort" not in vars(back)      # a run without the flag writes what it always wrote
    args = TR.parse_args(["-s", "x", "-m", str(tmp_path / "und"), "--undistort"])
    assert args.undistort is True
    back = eval(open(TR.write_cfg_args(args)).read(), {"Namespace": argparse.Namespace})
    assert back.undistort is True and back.images == "images"
    ap = surfel_mesh.build_parser()
    assert ap.parse_args(["-m", "m"]).undistort is False and ap.parse_args(["-m", "m", "-s", "x", "--undistort"]).undistort is True
    with pytest.raises(SystemExit):
        surfel_convert.main([])
    with pytest.raises(SystemExit):
        surfel_convert.main(["-s", "x", "--resize"])      # out of scope


def test_documents_name_the_rule():
    doc = open(os.path.join(REPO, "UNDISTORT.md")).read()
    assert "[UPSTREAM-RECALL]" in doc and "blank_pixels" in doc and "principal point" in doc
    assert re.search(r"surfel_convert\.py", open(os.path.join(REPO, "README.md")).read())
