"""GPU checks of the undistortion (UNDISTORT.md): the kernel byte for byte against the numpy oracle (tests/undistort_oracle.py), guard
pages, Scene(undistort=True) against oracle undistort -> resize -> to_float, and the training / convert CLIs end to end on a capture
warped into a SIMPLE_RADIAL camera.  Exact equality everywhere: the arithmetic is fp64 without contraction."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import scene_oracle as SO
import scene_scenes as SS
import undistort_oracle as UO
from test_undistort_cpu import CAPTURE_CAMERAS, FORCED, OVERFLOW, rewrite_cameras, to_convert_layout

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def SU():
    import surfel_undistort
    return surfel_undistort


@pytest.fixture(scope="module")
def SC():
    import surfel_scene
    return surfel_scene


def _run(torch, SU, src, q, pinhole, size):
    return SU.undistort(torch.from_numpy(np.ascontiguousarray(src)).cuda(), q, pinhole, size).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the kernel
# the five cameras of UNDISTORT.md at blank = 0: all four models; 67 x 49 (odd width, the result narrower, and for k < 0 as wide as the
# source); 320 x 240 into 333 x 244 and the like (many workgroups, a ragged last tile in x and in y)
@pytest.mark.parametrize("cam", UO.CAMERAS, ids=lambda c: "%s-%dx%d-k%g" % (c[0], c[2], c[3], c[1][-1] if c[0] == "SIMPLE_RADIAL" else c[1][4]))
def test_undistort_is_byte_equal_to_the_oracle(torch, SU, cam):
    model, params, W, H, size = cam
    q = SU.distortion_params(model, params)
    W2, H2, fx, fy, cx2, cy2 = SU.undistorted_camera(q, W, H)
    assert (W2, H2) == size
    for Cn in (1, 3, 4):
        src = SS.noise_image(20 + Cn, H, W, Cn)
        got = _run(torch, SU, src, q, (fx, fy, cx2, cy2), (W2, H2))
        want, valid = UO.undistort(src, q, (fx, fy, cx2, cy2), (W2, H2), return_valid=True)
        assert got.shape == (H2, W2, Cn) and got.dtype == np.uint8 and valid.all()
        assert np.array_equal(got, want), (model, Cn, int((got != want).sum()))


def test_forced_wide_output_has_zero_pixels_on_all_four_sides(torch, SU):
    q = UO.distortion_params(FORCED["model"], FORCED["params"])
    for Cn in (1, 3, 4):
        src = SS.noise_image(5, FORCED["H"], FORCED["W"], Cn)
        src[src == 0] = 1
        got = _run(torch, SU, src, q, FORCED["pinhole"], FORCED["size"])
        want, valid = UO.undistort(src, q, FORCED["pinhole"], FORCED["size"], return_valid=True)
        assert int((~valid).sum()) == FORCED["invalid"] and np.array_equal(got, want)
        assert not got[~valid].any() and got[valid].all()      # zero in every channel (the alpha too) exactly where the pixel is invalid


def test_one_pixel_output_and_sources_without_a_pair_of_taps(torch, SU):
    q = UO.distortion_params("SIMPLE_RADIAL", (60, 33.5, 24.2, 0.12))
    src = SS.noise_image(9, 49, 67, 3)
    got = _run(torch, SU, src, q, (60.0, 60.0, 0.5, 0.5), (1, 1))      # the one ray is the optical axis: the principal point's four taps
    assert got.shape == (1, 1, 3) and np.array_equal(got, UO.undistort(src, q, (60.0, 60.0, 0.5, 0.5), (1, 1))) and got.any()
    for H, W in ((1, 9), (9, 1), (1, 1)):      # x0 + 1 <= W - 1 (or the same in y) holds nowhere
        one = np.full((H, W, 3), 200, np.uint8)
        assert not _run(torch, SU, one, UO.distortion_params("SIMPLE_RADIAL", (60, W / 2, H / 2, 0.01)), (60.0, 60.0, 4.0, 4.0), (8, 8)).any()


@pytest.mark.parametrize("name", list(OVERFLOW))
def test_overflowing_coordinates_are_invalid(torch, SU, name):
    """finite parameters, infinite intermediate values: the NaN and the infinite coordinates compare false and come out zero; an
    infinite denominator alone is rad = 0, the principal point everywhere, like the oracle"""
    params, pinhole = OVERFLOW[name]
    q = UO.distortion_params("FULL_OPENCV", params)
    src = SS.noise_image(5, 49, 67, 4)
    src[src == 0] = 1
    got = _run(torch, SU, src, q, pinhole, (90, 70))
    assert np.array_equal(got, UO.undistort(src, q, pinhole, (90, 70)))
    assert got.all() if name == "inf_denominator" else not got.any()


def test_host_tensors_and_bad_arguments_are_refused(torch, SU):
    import surfel_native as n
    q = UO.distortion_params("SIMPLE_RADIAL", (60, 33.5, 24.2, 0.12))
    src = torch.from_numpy(SS.noise_image(1, 49, 67, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        SU.undistort(src, q, (60.0, 60.0, 31.0, 22.0), (62, 45))
    with pytest.raises(ValueError):
        SU.undistort(src.cuda().float(), q, (60.0, 60.0, 31.0, 22.0), (62, 45))
    with pytest.raises(RuntimeError, match="scene_undistort"):
        SU.undistort(src.cuda()[:, :, :2], q, (60.0, 60.0, 31.0, 22.0), (62, 45))
    with pytest.raises(RuntimeError, match="not positive"):
        SU.undistort(src.cuda(), q, (0.0, 60.0, 31.0, 22.0), (62, 45))
    with pytest.raises(n.LimitError):
        SU.undistort(src.cuda(), q, (60.0, 60.0, 31.0, 22.0), (32769, 1))


# ------------------------------------------------------------------------------------------------ 2. guard pages
def test_guard_pages_around_source_and_result():
    p = subprocess.run([sys.executable, os.path.join(HERE, "undistort_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "undistort_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 13, p.stdout
    assert sorted(int(line.split()[-3]) for line in p.stdout.splitlines() if line.startswith("ok blank 0")) == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ 3. Scene
def _u8(t):
    return t.detach().cpu().numpy().transpose(1, 2, 0)


def _expected(pixels, cam_id, r):
    """oracle undistort -> scene_oracle.resize -> to_float of one decoded image of COLMAP camera cam_id"""
    model, params = CAPTURE_CAMERAS["both"][cam_id]
    q = UO.distortion_params(model, params)
    W2, H2, fx, fy, cx2, cy2 = UO.undistorted_camera(q, SS.COLMAP_CAMERAS[cam_id][1], SS.COLMAP_CAMERAS[cam_id][2])
    und = UO.undistort(pixels, q, (fx, fy, cx2, cy2), (W2, H2))
    return SO.to_float(SO.resize(und, *SO.target_resolution(W2, H2, r))[0])


def _check_scene(scene, pixels_of, cam_of, r):
    cams = scene.getTrainCameras() + scene.getTestCameras()
    assert len(cams) == 9
    for cam in cams:
        planes, mask = _expected(pixels_of[cam.image_name], cam_of[cam.image_name], r)
        assert np.array_equal(_u8(cam.original_image), planes.transpose(1, 2, 0)), (cam.image_name, r)
        assert (cam.image_height, cam.image_width) == planes.shape[1:]
        assert (mask is None and cam.gt_alpha_mask is None) or np.array_equal(_u8(cam.gt_alpha_mask), mask.transpose(1, 2, 0)), (cam.image_name, r)


def _same(torch, a, b):
    for ca, cb in zip(a.getTrainCameras() + a.getTestCameras(), b.getTrainCameras() + b.getTestCameras()):
        assert ca.image_name == cb.image_name and torch.equal(ca.original_image, cb.original_image)
        assert torch.equal(ca.world_view_transform, cb.world_view_transform) and torch.equal(ca.full_proj_transform, cb.full_proj_transform)
        assert (ca.gt_alpha_mask is None) == (cb.gt_alpha_mask is None) and (ca.gt_alpha_mask is None or torch.equal(ca.gt_alpha_mask, cb.gt_alpha_mask))


def test_scene_undistorts_every_camera_like_the_oracle(torch, SC, tmp_path):
    from PIL import Image
    root = str(tmp_path / "capture")
    images, _ = SS.write_colmap(root, "txt")
    rewrite_cameras(root, CAPTURE_CAMERAS["both"])
    cam_of = {im[4].split(".")[0]: im[3] for im in images}
    pixels_of = {name: SC.decode(Image.open(os.path.join(root, "images", name + ".png"))) for name in cam_of}
    assert {p.shape[2] for p in pixels_of.values()} == {3, 4}
    with pytest.raises(ValueError, match="undistort"):
        SC.Scene(root, str(tmp_path / "refused"), shuffle=False)
    scenes = {}
    for r in (1, 2):
        model = str(tmp_path / ("model_r%d" % r))
        scenes[r] = SC.Scene(root, model, resolution=r, eval=True, shuffle=False, workers=1, undistort=True)
        _check_scene(scenes[r], pixels_of, cam_of, r)
        # cameras.json carries the undistorted sizes and focal lengths
        for entry in json.load(open(os.path.join(model, "cameras.json"))):
            m, params = CAPTURE_CAMERAS["both"][cam_of[entry["img_name"]]]
            q = UO.distortion_params(m, params)
            W2, H2, fx, fy, _, _ = UO.undistorted_camera(q, *SS.COLMAP_CAMERAS[cam_of[entry["img_name"]]][1:3])
            assert (entry["width"], entry["height"]) == (W2, H2) and entry["fx"] == pytest.approx(fx, rel=1e-12) and entry["fy"] == pytest.approx(fy, rel=1e-12)
    _same(torch, scenes[2], SC.Scene(root, str(tmp_path / "w3"), resolution=2, eval=True, shuffle=False, workers=3, undistort=True))
    # a file that is not the size of its COLMAP camera is an error that names it
    Image.fromarray(SS.noise_image(1, 37, 52, 3)).save(os.path.join(root, "images", "view_00.png"))
    with pytest.raises(ValueError, match="view_00.png is 52 x 37"):
        SC.Scene(root, str(tmp_path / "bad"), shuffle=False, undistort=True)


def test_scene_undistorts_a_jpeg_capture_the_same_on_host_and_device(torch, SC, tmp_path):
    """the JPEG copy of the capture in convert.py's layout (input/ + distorted/sparse/0): decode="device" and decode="host" give the
    same cameras, and both are the oracle's on Pillow's decode of the same files"""
    from PIL import Image
    root = str(tmp_path / "capture")
    images, _ = SS.write_colmap(root, "txt")
    rewrite_cameras(root, CAPTURE_CAMERAS["both"])
    cam_of, pixels_of = {}, {}
    for im in images:
        name = im[4].split(".")[0]
        png = os.path.join(root, "images", im[4])
        Image.open(png).convert("RGB").save(os.path.join(root, "images", name + ".jpg"), "JPEG", quality=92)
        os.remove(png)
        cam_of[name] = im[3]
        pixels_of[name] = SC.decode(Image.open(os.path.join(root, "images", name + ".jpg")))
    path = os.path.join(root, "sparse", "0", "images.txt")
    text = open(path).read().replace(".png", ".jpg")
    open(path, "w").write(text)
    to_convert_layout(root)
    host = SC.Scene(root, str(tmp_path / "host"), resolution=1, eval=True, shuffle=False, workers=1, undistort=True)
    dev = SC.Scene(root, str(tmp_path / "dev"), resolution=1, eval=True, shuffle=False, workers=3, undistort=True, decode="device")
    _check_scene(host, pixels_of, cam_of, 1)
    _same(torch, host, dev)


# ------------------------------------------------------------------------------------------------ 4. end to end
K_E2E = 0.1


def _write_distorted_capture(torch, root):
    """8 views at 64 x 48 of synthetic_object, rendered with the project's renderer and warped on the host into a SIMPLE_RADIAL camera
    (k = 0.1) of the same focal length: input/ + distorted/sparse/0"""
    from PIL import Image
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    gt = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    cams = TR.capture_views(gt, TR.orbit_cameras(8, 64, 48, device=dev), torch.zeros(3, device=dev))
    fx, fy = 64 / (2 * np.tan(cams[0].FoVx / 2)), 48 / (2 * np.tan(cams[0].FoVy / 2))
    assert abs(fx - fy) < 1e-9 * fx
    q = UO.distortion_params("SIMPLE_RADIAL", (fx, 32.0, 24.0, K_E2E))
    sparse = os.path.join(root, "distorted", "sparse", "0")
    os.makedirs(sparse)
    os.makedirs(os.path.join(root, "input"))
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for k, cam in enumerate(cams):
            name = "%03d.png" % k
            u8 = (cam.original_image.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8)
            Image.fromarray(UO.warp_to_distorted(u8, q, (fx, fy, 32.0, 24.0))).save(os.path.join(root, "input", name), "PNG")
            Rw2c = np.asarray(cam.R, np.float64).T
            f.write(struct.pack("<i7di", k + 1, *SS.rotmat_to_qvec(Rw2c), *np.asarray(cam.T, np.float64), 1) + name.encode() + b"\x00")
            f.write(struct.pack("<Q", 2) + struct.pack("<ddq", 1.5, 2.5, -1) + struct.pack("<ddq", 3.0, 4.0, 7))      # observations: dropped by the converter
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, 2, 64, 48) + struct.pack("<4d", fx, 32.0, 24.0, K_E2E))      # model 2: SIMPLE_RADIAL
    xyz = gt.get_xyz.detach().cpu().numpy().astype(np.float64)
    rgb = np.clip((gt._features_dc.detach().cpu().numpy()[:, 0] * 0.28209479177387814 + 0.5) * 255.0, 0, 255).astype(np.uint8)
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", xyz.shape[0]))
        for p in range(xyz.shape[0]):
            f.write(struct.pack("<Q3d3Bd", p + 1, *xyz[p], *[int(v) for v in rgb[p]], 0.5) + struct.pack("<Q", 0))
    return q


def test_train_and_convert_clis_end_to_end(torch, SC, tmp_path):
    import surfel_convert
    import surfel_mesh
    import surfel_trainer as TR
    from PIL import Image
    root, model = str(tmp_path / "capture"), str(tmp_path / "model")
    q = _write_distorted_capture(torch, root)
    W2, H2, fx, fy, _, _ = UO.undistorted_camera(q, 64, 48)
    assert (W2, H2) != (64, 48)
    bg = torch.zeros(3, device="cuda:0")

    def held_out_psnr(scene):
        (cam,) = scene.getTestCameras()
        assert cam.image_name == "000" and (cam.image_width, cam.image_height) == (W2, H2)
        with torch.no_grad():
            img = TR.render(cam, scene.gaussians, TR.pipeline_params(), bg)["render"].clamp(0.0, 1.0)
        return float(TR.psnr(img, cam.original_image).mean())

    with pytest.raises(ValueError, match="could not recognize"):
        SC.Scene(root, str(tmp_path / "refused"), eval=True, shuffle=False)
    before = held_out_psnr(SC.Scene(root, str(tmp_path / "fresh"), eval=True, shuffle=False, undistort=True))
    assert TR.main(["-s", root, "-m", model, "--undistort", "--eval", "--iterations", "300", "--save_iterations", "300", "--quiet"]) == 0
    assert "undistort=True" in open(os.path.join(model, "cfg_args")).read()
    trained = SC.Scene(root, model, eval=True, shuffle=False, load_iteration=-1, undistort=True)
    after = held_out_psnr(trained)
    print("held-out PSNR on the undistorted view: %.3f dB before, %.3f dB after 300 iterations" % (before, after))
    assert after > before
    # the mesh CLI finds the flag in cfg_args: the ground truth it exports is the undistorted image
    assert surfel_mesh.main(["-m", model, "-s", root, "--skip_mesh", "--skip_train"]) == 0
    gt0 = np.asarray(Image.open(os.path.join(model, "test", "ours_300", "gt", "00000.png")))
    (held,) = trained.getTestCameras()
    assert gt0.shape == (H2, W2, 3) and np.array_equal(gt0.astype(np.float32) / np.float32(255), _u8(held.original_image))
    # the converter on the same folder, then the unchanged default reader: the same cameras, the same images
    assert surfel_convert.main(["-s", root, "--quiet"]) == 0
    for name in ("cameras.bin", "images.bin", "points3D.bin"):
        assert os.path.exists(os.path.join(root, "sparse", "0", name)), name
    assert open(os.path.join(root, "sparse/0/points3D.bin"), "rb").read() == open(os.path.join(root, "distorted/sparse/0/points3D.bin"), "rb").read()
    (pin,) = SC.read_cameras_bin(os.path.join(root, "sparse/0/cameras.bin")).values()
    assert (pin.model, pin.width, pin.height) == ("PINHOLE", W2, H2) and pin.params.tolist() == [fx, fy, 32.0 * W2 / 64, 24.0 * H2 / 48]
    assert os.path.getsize(os.path.join(root, "sparse/0/images.bin")) == 8 + 8 * (4 + 56 + 4 + 8 + 8)      # no 2-D observations
    plain = SC.Scene(root, str(tmp_path / "plain"), eval=True, shuffle=False)      # sparse/0 + images/, no flag
    und = trained.getTestCameras() + trained.getTrainCameras()
    cams = plain.getTestCameras() + plain.getTrainCameras()
    assert len(cams) == len(und) == 8
    for a, b in zip(cams, und):
        assert a.image_name == b.image_name and (a.image_width, a.image_height, a.FoVx, a.FoVy) == (b.image_width, b.image_height, b.FoVx, b.FoVy)
        assert torch.equal(a.world_view_transform, b.world_view_transform) and torch.equal(a.full_proj_transform, b.full_proj_transform)
        assert torch.equal(a.original_image, b.original_image), a.image_name
