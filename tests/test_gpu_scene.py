"""GPU checks of the capture loader (SCENE.md): the resampling passes, the float conversion and the composite bit for bit against the
numpy oracle (tests/scene_oracle.py, itself bit-equal to Pillow: tests/test_scene_cpu.py), guard pages, Scene on the COLMAP and Blender
captures against what the reference loaded from them (tests/golden/ref_scene.npz), and the training / mesh CLIs end to end.  Exact
equality everywhere: the arithmetic is integer, one correctly rounded fp32 division, and fp64 without contraction."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_oracle as SO
import scene_scenes as SS
from test_scene_cpu import SHAPES

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def SC():
    import surfel_scene
    return surfel_scene


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(REPO, "tests", "golden", "ref_scene.npz"))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the passes
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resample_is_bit_equal_to_the_oracle(torch, SC, shape):
    H, W, H2, W2 = shape
    for Cn in (1, 3, 4):
        src = SS.noise_image(1000 + Cn, H, W, Cn)
        want, mid = SO.resize(src, W2, H2)
        d = _dev(torch, src)
        if W2 != W:
            assert np.array_equal(SC.resample_h(d, W2).cpu().numpy(), mid), (shape, Cn, "intermediate")
        image, mask = SC.load_image(d, (W2, H2))
        planes, m = SO.to_float(want)
        assert image.dtype == torch.float32 and tuple(image.shape) == (min(Cn, 3), H2, W2)
        assert np.array_equal(image.cpu().numpy(), planes), (shape, Cn)
        assert np.array_equal(image.cpu().numpy(), (want.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[:3])
        if Cn == 4:
            assert tuple(mask.shape) == (1, H2, W2) and np.array_equal(mask.cpu().numpy(), m), (shape, Cn, "mask")
        else:
            assert mask is None


def test_resample_dtu_size_on_sampled_rows_and_columns(torch, SC):
    """1200 x 1600 -> 600 x 800 (-r 2 of a DTU frame): many strips and rows; the oracle is evaluated on 64 seeded rows and columns"""
    rng = np.random.default_rng(5)
    src = SS.noise_image(77, 1200, 1600, 3)
    cols, rows = np.sort(rng.choice(800, 64, replace=False)), np.sort(rng.choice(600, 64, replace=False))
    cols[0], cols[-1], rows[0], rows[-1] = 0, 799, 0, 599
    d = _dev(torch, src)
    mid = SC.resample_h(d, 800).cpu().numpy()
    assert mid.shape == (1200, 800, 3) and np.array_equal(mid[:, cols], SO.resample_h(src, 800, cols))
    image, mask = SC.load_image(d, (800, 600))
    want = SO.resample_v(np.ascontiguousarray(mid[:, cols]), 600, rows)              # [64 rows, 64 cols, 3]
    got = image.cpu().numpy()[:, rows][:, :, cols]
    assert mask is None and np.array_equal(got, SO.to_float(want)[0])


# ------------------------------------------------------------------------------------------------ 3. / 4. conversion and composite
def test_to_float_alone_on_all_256_values(torch, SC):
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for Cn in (1, 3, 4):
        src = np.stack([np.roll(v, c, axis=1) for c in range(Cn)], axis=2)
        image, mask = SC.load_image(_dev(torch, src), (16, 16))
        planes, m = SO.to_float(src)
        assert np.array_equal(image.cpu().numpy(), planes)
        assert (mask is None) if Cn < 4 else np.array_equal(mask.cpu().numpy(), m)
    assert np.array_equal(np.sort(image.cpu().numpy()[0].ravel()), np.arange(256, dtype=np.float32) / np.float32(255))


def test_composite_all_colour_alpha_pairs(torch, SC):
    v = np.arange(256, dtype=np.uint8)
    rgba = np.zeros((256, 256, 4), np.uint8)
    rgba[:, :, 0], rgba[:, :, 1], rgba[:, :, 2] = v[:, None], v[::-1, None], (v[:, None] * 7 + 3).astype(np.uint8)
    rgba[:, :, 3] = v[None, :]
    d = _dev(torch, rgba)
    for white in (False, True):
        out = SC.composite(d, white)
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), SO.composite(rgba, white))


# ------------------------------------------------------------------------------------------------ 5. guard pages
def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "scene_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "scene_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 9, p.stdout


# ------------------------------------------------------------------------------------------------ 6. Scene against the reference
def _u8(t):
    return t.detach().cpu().numpy().transpose(1, 2, 0)


def _check_cam(cam, ref, tag, key):
    want = ref["%s/%s/image" % (tag, key)]
    assert np.array_equal(_u8(cam.original_image), want.astype(np.float32) / np.float32(255)), (tag, key)
    assert (cam.image_height, cam.image_width) == want.shape[:2]
    mk = "%s/%s/mask" % (tag, key)
    if mk in ref.files:
        assert np.array_equal(_u8(cam.gt_alpha_mask), ref[mk].astype(np.float32) / np.float32(255)), (tag, key, "mask")
    else:
        assert cam.gt_alpha_mask is None


def test_scene_colmap_matches_the_reference(torch, SC, ref, tmp_path):
    root = str(tmp_path / "capture")
    SS.write_colmap(root, "bin")
    for r in (-1, 1, 2, 20):
        for ev in (False, True):
            if ev and r != 2:
                continue
            model = str(tmp_path / ("model_r%d_%d" % (r, ev)))
            sc = SC.Scene(root, model, resolution=r, eval=ev, shuffle=False, workers=1)
            tag = "colmap/eval%d" % ev
            assert [c.image_name for c in sc.getTrainCameras()] == ref[tag + "/train"].tolist()
            assert [c.image_name for c in sc.getTestCameras()] == ref[tag + "/test"].tolist()
            assert [c.uid for c in sc.getTrainCameras()] == list(range(len(sc.getTrainCameras())))
            for cam in sc.getTrainCameras() + sc.getTestCameras():
                _check_cam(cam, ref, "colmap/r%d" % max(r, 1), cam.image_name)
            assert sc.cameras_extent == pytest.approx(float(ref[tag + "/radius"]), rel=1e-12) and sc.gaussians.P == 200
            got, want = json.load(open(os.path.join(model, "cameras.json"))), json.loads(str(ref[tag + "/cameras_json"]))
            assert [(g["id"], g["img_name"]) for g in got] == [(w["id"], w["img_name"]) for w in want]
            assert os.path.getsize(os.path.join(model, "input.ply")) == os.path.getsize(os.path.join(root, "sparse/0/points3D.ply"))
    # any number of decoding threads, shuffled or not: the same tensors
    a = SC.Scene(root, str(tmp_path / "wa"), resolution=2, eval=True, shuffle=True, seed=3, workers=1)
    b = SC.Scene(root, str(tmp_path / "wb"), resolution=2, eval=True, shuffle=True, seed=3, workers=3)
    assert [c.image_name for c in a.getTrainCameras()] == [c.image_name for c in b.getTrainCameras()] != ref["colmap/eval1/train"].tolist()
    for ca, cb in zip(a.getTrainCameras() + a.getTestCameras(), b.getTrainCameras() + b.getTestCameras()):
        assert torch.equal(ca.original_image, cb.original_image) and torch.equal(ca.world_view_transform, cb.world_view_transform)
        assert (ca.gt_alpha_mask is None) == (cb.gt_alpha_mask is None) and (ca.gt_alpha_mask is None or torch.equal(ca.gt_alpha_mask, cb.gt_alpha_mask))


def test_scene_blender_matches_the_reference(torch, SC, ref, tmp_path):
    root = SS.write_blender(str(tmp_path / "lego"))
    for white in (False, True):
        for r in (-1, 2, 20):
            sc = SC.Scene(root, str(tmp_path / ("m%d_%d" % (white, r))), resolution=r, white_background=white, eval=True, shuffle=False, workers=3)
            assert len(sc.getTrainCameras()) == 4 and len(sc.getTestCameras()) == 2 and sc.gaussians.P == 100_000
            for k, cam in enumerate(sc.getTrainCameras() + sc.getTestCameras()):
                _check_cam(cam, ref, "blender/white%d/r%d" % (white, max(r, 1)), "%d" % k)
            assert sc.cameras_extent == pytest.approx(float(ref["blender/eval1/radius"]), rel=1e-12)


# ------------------------------------------------------------------------------------------------ 7. no host path
def test_host_tensors_and_cpu_device_are_refused(torch, SC):
    src = SS.noise_image(1, 12, 10, 3)
    for size in ((5, 6), (10, 6), (5, 12), (10, 12)):
        with pytest.raises(RuntimeError, match="HIP device"):
            SC.load_image(torch.from_numpy(src), size)
        with pytest.raises(RuntimeError, match="HIP device"):
            SC.load_image(src, size, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        SC.composite(torch.zeros((4, 4, 4), dtype=torch.uint8), True)


# ------------------------------------------------------------------------------------------------ 8. end to end
def _write_capture(torch, root):
    """8 views at 64 x 48 of synthetic_object, rendered with the project's renderer, as a COLMAP capture"""
    import struct
    from PIL import Image
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    gt = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    cams = TR.capture_views(gt, TR.orbit_cameras(8, 64, 48, device=dev), torch.zeros(3, device=dev))
    sparse = os.path.join(root, "sparse", "0")
    os.makedirs(sparse)
    os.makedirs(os.path.join(root, "images"))
    pixels = {}
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for k, cam in enumerate(cams):
            name = "%03d.png" % k
            u8 = (cam.original_image.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8)
            Image.fromarray(u8).save(os.path.join(root, "images", name), "PNG")
            pixels[name] = u8
            Rw2c = np.asarray(cam.R, np.float64).T
            f.write(struct.pack("<i7di", k + 1, *SS.rotmat_to_qvec(Rw2c), *np.asarray(cam.T, np.float64), 1) + name.encode() + b"\x00" + struct.pack("<Q", 0))
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        fx, fy = 64 / (2 * np.tan(cams[0].FoVx / 2)), 48 / (2 * np.tan(cams[0].FoVy / 2))
        f.write(struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, 1, 64, 48) + struct.pack("<4d", fx, fy, 32.0, 24.0))
    xyz = gt.get_xyz.detach().cpu().numpy().astype(np.float64)
    rgb = np.clip((gt._features_dc.detach().cpu().numpy()[:, 0] * 0.28209479177387814 + 0.5) * 255.0, 0, 255).astype(np.uint8)
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", xyz.shape[0]))
        for p in range(xyz.shape[0]):
            f.write(struct.pack("<Q3d3Bd", p + 1, *xyz[p], *[int(v) for v in rgb[p]], 0.5) + struct.pack("<Q", 0))
    return pixels


def test_train_and_mesh_clis_end_to_end(torch, SC, tmp_path):
    import surfel_io
    import surfel_mesh
    import surfel_trainer as TR
    from PIL import Image
    root, model = str(tmp_path / "capture"), str(tmp_path / "model")
    pixels = _write_capture(torch, root)
    bg = torch.zeros(3, device="cuda:0")

    def held_out_psnr(scene):
        (cam,) = scene.getTestCameras()
        assert cam.image_name == "000"
        with torch.no_grad():
            img = TR.render(cam, scene.gaussians, TR.pipeline_params(), bg)["render"].clamp(0.0, 1.0)
        return float(TR.psnr(img, cam.original_image).mean())

    before = held_out_psnr(SC.Scene(root, str(tmp_path / "fresh"), eval=True, shuffle=False))
    assert TR.main(["-s", root, "-m", model, "--eval", "--iterations", "300", "--save_iterations", "300", "--quiet"]) == 0
    for name in ("cfg_args", "cameras.json", "input.ply", "point_cloud/iteration_300/point_cloud.ply"):
        assert os.path.exists(os.path.join(model, name)), name
    trained = SC.Scene(root, model, eval=True, shuffle=False, load_iteration=-1)
    assert trained.loaded_iter == 300
    after = held_out_psnr(trained)
    print("held-out PSNR: %.3f dB before, %.3f dB after 300 iterations" % (before, after))
    assert after > before
    # the mesh CLI on that folder, with the capture's ground truth
    assert surfel_mesh.main(["-m", model, "-s", root, "--mesh_res", "64"]) == 0
    gt0 = np.asarray(Image.open(os.path.join(model, "train", "ours_300", "gt", "00000.png")))
    assert np.array_equal(gt0, pixels["001.png"])              # the first training view (000 is held out)
    assert len(os.listdir(os.path.join(model, "train", "ours_300", "renders"))) == 7
    assert sorted(os.listdir(os.path.join(model, "test", "ours_300", "gt"))) == ["00000.png"] and os.path.exists(os.path.join(model, "train", "ours_300", "fuse.ply"))
    assert np.array_equal(np.asarray(Image.open(os.path.join(model, "test", "ours_300", "gt", "00000.png"))), pixels["000.png"])
    # cameras.json reproduces the Scene's cameras (test first, then train)
    from_json = surfel_io.read_cameras_json(os.path.join(model, "cameras.json"), device="cuda:0")
    scene_cams = trained.getTestCameras() + trained.getTrainCameras()
    assert len(from_json) == len(scene_cams) == 8
    for a, b in zip(from_json, scene_cams):
        assert a.image_name == b.image_name and (a.image_width, a.image_height) == (b.image_width, b.image_height)
        for m in ("world_view_transform", "full_proj_transform", "camera_center"):
            assert torch.allclose(getattr(a, m), getattr(b, m), atol=1e-6, rtol=0), (a.image_name, m)
