"""CPU tests of the trajectory renderer (RENDER.md): the path generator against what the reference's utils/render_utils.py returned on
the same cameras (tests/golden/ref_path.npz, minted by tests/golden/make_golden_path.py), the numpy oracle of the frame kernels against
the real thing (the reference's save_img_u8 expression, matplotlib's turbo colormap, np.percentile), the generated colour table, the
FrameWriter on host tensors, the C ABI and the CLI's flags.  Nothing here touches a device."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import path_oracle as PO
import path_scenes as PS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(REPO, "tests", "golden", "ref_path.npz"))


def _cameras(name):
    import torch
    wvt, H, W = PS.camera_set(name)
    proj = torch.from_numpy(PS.projection(H, W))
    return [types.SimpleNamespace(world_view_transform=torch.from_numpy(w), projection_matrix=proj, image_height=H, image_width=W, uid=k)
            for k, w in enumerate(wvt)], H, W


# ------------------------------------------------------------------------------------------------ 1. the path
@pytest.mark.parametrize("name", PS.SETS)
def test_path_parts_match_the_reference(ref, name):
    import surfel_path as SP
    wvt, H, W = PS.camera_set(name)
    assert np.array_equal(wvt, ref[name + "/wvt"]) and (H % 2, W % 2) == (1, 1)      # the fixture's inputs are these cameras
    pose = ref[name + "/pose"]
    c2ws = np.array([np.linalg.inv(w.T) for w in wvt])
    np.testing.assert_allclose(c2ws[:, :3, :] @ np.diag([1, -1, -1, 1]), pose, rtol=1e-9, atol=0)
    # distinct PCA eigenvalues: the order of the principal axes is well defined
    t = pose[:, :3, 3] - pose[:, :3, 3].mean(0)
    ev = np.sort(np.linalg.eigvalsh(t.T @ t))
    assert np.all(np.diff(ev) > 1e-3 * ev[-1])
    rec, tr = SP.transform_poses_pca(pose)
    np.testing.assert_allclose(rec, ref[name + "/recentered"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(tr, ref[name + "/transform"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(SP.focus_point_fn(rec), ref[name + "/focus"], rtol=1e-9, atol=0)
    assert np.linalg.det(tr[:3, :3]) == pytest.approx(1.0, abs=1e-12)
    for n in (8, 240):
        ell = SP.generate_ellipse_path(rec, n_frames=n)
        assert ell.shape == (n, 3, 4) and np.all(ell[:, 2, 3] == 0.0)      # the path lies in the z = 0 plane of the PCA frame
        np.testing.assert_allclose(ell, ref["%s/ellipse%d" % (name, n)], rtol=1e-9, atol=0)
    p = SP.pad_poses(rec)
    assert p.shape == (len(wvt), 4, 4) and np.array_equal(p[:, 3], np.tile([0, 0, 0, 1.0], (len(wvt), 1))) and np.array_equal(p[:, :3], rec)
    vm = SP.viewmatrix(np.array([0.0, 0.0, 2.0]), np.array([0.0, 1.0, 0.0]), np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(vm, np.array([[1.0, 0, 0, 1], [0, 1.0, 0, 2], [0, 0, 1.0, 3]]))


@pytest.mark.parametrize("name", PS.SETS)
@pytest.mark.parametrize("n", [8, 240])
def test_generate_path_matches_the_reference(ref, name, n):
    import torch
    import surfel_path as SP
    cams, H, W = _cameras(name)
    traj = SP.generate_path(cams, n_frames=n)
    want = ref["%s/path%d" % (name, n)]
    assert len(traj) == n and want.shape == (n, 4, 4)
    for cam, w in zip(traj, want):
        assert cam.world_view_transform.dtype == torch.float32
        np.testing.assert_allclose(cam.world_view_transform.numpy(), w, rtol=1e-5, atol=1e-6)
        assert (cam.image_height, cam.image_width) == (H - 1, W - 1)      # odd sizes rounded down to even
        wvt = cam.world_view_transform
        assert torch.equal(cam.full_proj_transform, wvt @ cams[0].projection_matrix)
        assert torch.equal(cam.camera_center, torch.linalg.inv(wvt)[3, :3])
        # a rigid transform, and the centre it implies is the camera centre
        R = wvt[:3, :3].double().numpy()
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-5)
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-5)
    assert traj[0].uid == cams[0].uid and (cams[0].image_height, cams[0].image_width) == (H, W)      # a copy of cameras[0]; the original is untouched
    assert traj[0] is not traj[1] and not torch.equal(traj[0].world_view_transform, traj[1].world_view_transform)


def test_generate_path_drops_a_camera_s_cached_constants():
    """surfel_render.Camera caches the constants its render_post kernel reads; a path camera must not inherit cameras[0]'s"""
    import torch
    import surfel_path as SP
    from surfel_render import Camera
    wvt, H, W = PS.camera_set("ring")
    fx, fy = PS.fov(H, W)
    cams = []
    for w in wvt:
        w2c = w.T.astype(np.float64)
        cams.append(Camera(colmap_id=0, R=w2c[:3, :3].T, T=w2c[:3, 3], FoVx=fx, FoVy=fy, image=torch.zeros(3, H, W), data_device="cpu"))
    first = cams[0].post_consts()
    traj = SP.generate_path(cams, n_frames=8)
    assert traj[3]._post is None and traj[3].original_image is cams[0].original_image
    assert not torch.equal(traj[3].post_consts(), first) and torch.equal(cams[0].post_consts(), first)
    assert even(traj[3].image_height) and even(traj[3].image_width)


def even(v):
    return v % 2 == 0


# ------------------------------------------------------------------------------------------------ 2. the oracle is the real thing
def _save_img_u8_expression(img):
    """utils/render_utils.py:274 on an [H, W, C] float32 image"""
    with np.errstate(invalid="ignore"):
        return (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)


@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 3, 129), (3, 33, 65)])
def test_quantize_oracle_is_save_img_u8(shape):
    a = PS.frame(3, *shape)
    assert np.isnan(a).any() and np.isinf(a).any() and (a < 0).any() and (a > 1).any()
    assert np.array_equal(PO.quantize(a), _save_img_u8_expression(a.transpose(1, 2, 0)))
    # every k / 255 and its two neighbours, in one row
    sp = PS.special_values()[None, None, :]
    got = PO.quantize(sp)
    assert np.array_equal(got, _save_img_u8_expression(sp.transpose(1, 2, 0)))
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    up = PO.quantize(np.nextafter(k, np.float32(2))[None, None])[0, :, 0]
    assert np.all(up[:255] >= PO.quantize(k[None, None])[0, :255, 0])
    # the normal-map form: numpy evaluates img * 0.5 + 0.5 on float32 in float32, one rounding per operation
    nrm = PS.frame(4, *shape, normal=True)
    with np.errstate(invalid="ignore"):
        want = _save_img_u8_expression(nrm.transpose(1, 2, 0) * 0.5 + 0.5)
    assert np.array_equal(PO.quantize(nrm, 0.5, 0.5), want)


def _create_videos_depth_frame(depth, lo, hi):
    """utils/render_utils.py:262-266 on a float32 depth frame, with matplotlib.colormaps in place of the removed cm.get_cmap"""
    import matplotlib
    with np.errstate(divide="ignore", invalid="ignore"):
        img = np.log(depth)
        img = np.clip((img - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1)
        img = matplotlib.colormaps["turbo"](img)[..., :3]
        return (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)


def _limits(depth0, p=3):
    """utils/render_utils.py:219-220"""
    with np.errstate(divide="ignore"):
        lo, hi = [np.log(x) for x in np.percentile(depth0.flatten(), [p, 100 - p])]
    return lo, hi


@pytest.mark.parametrize("zero_frac, black", [(0.0, False), (0.009, False), (0.08, True)])
def test_turbo_oracle_is_matplotlib(zero_frac, black):
    pytest.importorskip("matplotlib")
    d0 = PS.depth_frame(5, 61, 83, zero_frac)
    lo, hi = _limits(d0)
    assert isinstance(lo, np.float64) and (lo == -np.inf) == black
    for d in (d0, PS.depth_frame(6, 61, 83, 0.02, lo=0.5, hi=9.0)):
        want = _create_videos_depth_frame(d, lo, hi)
        got = PO.depth_turbo(d, lo, hi)
        assert np.array_equal(got, want)
        assert (not want.any()) == black
        if not black and zero_frac:
            assert np.all(got[d == 0] == PO.turbo_table()[0]) and (d == 0).any()


def test_turbo_oracle_on_a_constant_frame_and_nan():
    """hi == lo: a pixel whose fp32 log equals the fp64 limit is 0 / 0 = NaN = black, which is the whole frame when the constant's log
    is exact in both precisions (1.0).  For any other constant the fp32 log, widened, misses the fp64 log by a rounding error, and
    (x - lo) / 0 = +-inf clips to the last or first table entry: what the reference's expression does, and the oracle with it."""
    pytest.importorskip("matplotlib")
    d = np.full((9, 11), 1.0, np.float32)
    lo, hi = _limits(d)
    assert lo == hi == 0.0
    assert not PO.depth_turbo(d, lo, hi).any() and not _create_videos_depth_frame(d, lo, hi).any()
    d = np.full((9, 11), 2.5, np.float32)
    lo, hi = _limits(d)
    assert lo == hi and float(np.log(np.float32(2.5))) > lo
    got = PO.depth_turbo(d, lo, hi)
    assert np.array_equal(got, _create_videos_depth_frame(d, lo, hi)) and np.all(got == PO.turbo_table()[255])
    d2 = PS.depth_frame(8, 9, 11)
    d2[2, 3] = np.nan
    lo, hi = _limits(PS.depth_frame(8, 9, 11))
    got = PO.depth_turbo(d2, lo, hi)
    assert np.array_equal(got, _create_videos_depth_frame(d2, lo, hi)) and not got[2, 3].any() and got.any()


@pytest.mark.parametrize("kind", PS.ORDER_KINDS)
def test_percentile_oracle_is_np_percentile(kind):
    import surfel_path as SP
    for n in PS.ORDER_SIZES:
        x = PS.order_data(kind, n)
        for q in ([3, 97], [0, 50, 100], [12.5], [99.999]):
            with np.errstate(invalid="ignore"):
                want = np.percentile(x, q)
                got = PO.percentile(x, q)
                # the product's host half (ranks, then numpy's lerp) on the sorted data's order statistics
                ranks, prev, nxt, gamma = SP.percentile_ranks(n, q)
                host = SP.lerp_percentiles(np.sort(x)[ranks], ranks, prev, nxt, gamma)
            assert ranks == sorted(set(ranks)) and len(ranks) <= 8 and ranks[-1] == n - 1
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(host, want, rtol=1e-12, atol=0, equal_nan=True)
    x = PS.order_data("uniform", 100)
    x[17] = np.nan
    assert np.isnan(PO.percentile(x, [3, 97])).all() and np.isnan(np.percentile(x, [3, 97])).all()
    assert np.array_equal(PO.order_stats(x, [0, 99])[:1], [np.nanmin(x)]) and np.isnan(PO.order_stats(x, [99])[0])


def test_turbo_table_header_is_current():
    pytest.importorskip("matplotlib")
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "gen_turbo_table.py"), "--check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    tab = PO.turbo_table()
    assert tab.shape == (256, 3) and tab.dtype == np.uint8 and tuple(tab[0]) == (48, 18, 59) and tuple(tab[255]) == (122, 4, 2)


# ------------------------------------------------------------------------------------------------ 3. FrameWriter on host tensors
def test_frame_writer_on_host_tensors(tmp_path):
    import torch
    from PIL import Image
    import surfel_path as SP
    rng = np.random.default_rng(0)
    frames = []
    with SP.FrameWriter(workers=3, ring=4) as fw:
        assert (fw.workers, fw.ring) == (3, 4)
        for k in range(20):
            if k % 3 == 2:
                a = rng.normal(size=(13 + k, 17)).astype(np.float32)
                a[0, 0], a[1, 1] = np.nan, 1e-42
                path = str(tmp_path / ("f%02d.tiff" % k))
            else:
                a = rng.integers(0, 256, size=(11 + k, 9, 1 if k % 3 else 3), dtype=np.uint8)
                path = str(tmp_path / ("f%02d.png" % k))
            frames.append((path, a))
            t = torch.from_numpy(a.copy())
            fw.submit(path, t)
            t.zero_()      # the writer holds its own copy from submit() on
    assert fw.frames == 20 and len(fw._idle) == 4
    for path, a in frames:
        got = np.asarray(Image.open(path))
        if a.dtype == np.uint8:
            assert got.dtype == np.uint8 and np.array_equal(got, a[:, :, 0] if a.shape[2] == 1 else a), path
        else:
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.nan_to_num(a).view(np.uint32)), path
            assert got[0, 0] == 0.0
    assert SP.FrameWriter(workers=64).workers == 8      # the scene loader's ceiling, whatever the machine has


def test_frame_writer_surfaces_a_worker_exception(tmp_path):
    import torch
    import surfel_path as SP
    fw = SP.FrameWriter(workers=2, ring=2)
    ok = str(tmp_path / "ok.png")
    fw.submit(ok, torch.zeros((4, 4, 3), dtype=torch.uint8))
    fw.submit(str(tmp_path / "no_such_folder" / "x.png"), torch.zeros((4, 4, 3), dtype=torch.uint8))
    fw.submit(str(tmp_path / "ok2.png"), torch.zeros((4, 4, 3), dtype=torch.uint8))      # (the ring is not lost to the failed frame)
    with pytest.raises(FileNotFoundError, match="no_such_folder"):
        fw.close()
    assert os.path.exists(ok) and os.path.exists(str(tmp_path / "ok2.png"))
    with pytest.raises(RuntimeError, match="after close"):
        fw.submit(ok, torch.zeros((4, 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected"):
        SP.FrameWriter().submit(ok, torch.zeros((4, 4), dtype=torch.float64))


def test_device_entries_refuse_host_tensors():
    import torch
    import surfel_path as SP
    with pytest.raises(RuntimeError, match="HIP device"):
        SP.quantize_u8(torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        SP.colorize_depth(torch.ones(4, 4), 0.0, 1.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        SP.percentiles(torch.ones(16), [3, 97])


# ------------------------------------------------------------------------------------------------ 4. C ABI and CLI
def test_vis_header_signatures_and_exports():
    """include/surfel_vis.h <-> SIGNATURES["surfel_vis.h"] <-> the library's exports, both ways (as test_abi_cpu does for its headers)"""
    import re
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_vis.h")
    assert len(protos) == mentions == 3
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_vis.h"]) == sorted(n.VIS_EXPORTS)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert C.cast(fn, C.c_void_p).value and fn.restype is C.c_int and ret == "int"
        assert len(fn.argtypes) == len(params), name
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            elif pname == "ranks":
                assert ctype == "int64_t*" and at is C.POINTER(C.c_int64), where      # a host array
            else:
                assert ctype.endswith("*") and at is (n.Stream if pname == "stream" else n.DevPtr), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
    # the reverse: every surfel_vis_* the library's dynamic symbol table exports is declared
    out = subprocess.run(["nm", "-D", "--defined-only", n.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r"\b(surfel_vis_\w+)\b", out)))
    assert exported == sorted(p[0] for p in protos)
    hdr = open(os.path.join(REPO, "include", "surfel_vis.h")).read()
    import surfel_path
    assert int(re.search(r"#define SURFEL_VIS_ORDER_SCRATCH_BYTES (\d+)", hdr).group(1)) == surfel_path._ORDER_SCRATCH
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_path_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "frame_vis.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["frame_vis.hip"]
    assert any(h.endswith("surfel_vis.h") for h in mod.HEADERS) and "vis_turbo_table.h" in mod.HEADERS


def test_vis_entries_check_their_arguments_without_a_device():
    import surfel_native as n
    p = C.c_void_p(256)
    ranks = (C.c_int64 * 2)(0, 5)
    for args in ((2, 4, 4, p, 1.0, 0.0, p), (3, 0, 4, p, 1.0, 0.0, p), (3, 4, 4, None, 1.0, 0.0, p), (3, 4, 4, C.c_void_p(258), 1.0, 0.0, p)):
        with pytest.raises(RuntimeError, match=r"\(-1\): vis_quantize"):
            n.call(None, "surfel_vis_quantize", *args)
    with pytest.raises(n.LimitError, match="65536"):
        n.call(None, "surfel_vis_depth_turbo", 70000, 4, p, 0.0, 1.0, p)
    with pytest.raises(RuntimeError, match="ascending"):
        n.call(None, "surfel_vis_order_stats", 5, p, 2, ranks, p, p, 8448)
    with pytest.raises(RuntimeError, match="ascending"):
        n.call(None, "surfel_vis_order_stats", 9, p, 2, (C.c_int64 * 2)(5, 0), p, p, 8448)
    with pytest.raises(RuntimeError, match="scratch"):
        n.call(None, "surfel_vis_order_stats", 9, p, 2, ranks, p, p, 8447)
    with pytest.raises(RuntimeError, match="bad arguments"):
        n.call(None, "surfel_vis_order_stats", 9, p, 9, ranks, p, p, 8448)


def test_mesh_cli_lists_the_new_flags(capsys):
    import surfel_mesh
    with pytest.raises(SystemExit) as e:
        surfel_mesh.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--render_path", "--n_frames", "--skip_train", "--skip_test", "--skip_mesh", "--vis_normals"):
        assert flag in text, flag
    args = surfel_mesh.build_parser().parse_args(["-m", "x"])
    assert (args.render_path, args.n_frames, args.skip_train, args.skip_test, args.skip_mesh, args.vis_normals) == (False, 240, False, False, False, False)
