"""GPU checks of the JPEG decoder (JPEGDEC.md): the HIP decoder byte for byte against Pillow and the numpy restatement
(tests/jpegdec_oracle.py, itself checked against Pillow in tests/test_jpegdec_cpu.py), its counters against the restatement's, the
"not converged" and "damaged" statuses, guard pages, load_cameras(decode="device") against decode="host", and the CLI in a child
process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegdec_oracle as JO
import jpegdec_scenes as JS
import scene_scenes as SS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
BITS = (128, 1024)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def JD():
    import surfel_jpegdec
    return surfel_jpegdec


@functools.lru_cache(maxsize=None)
def oracle_info(name, bits):
    import surfel_jpegdec
    pixels, info = JO.decode(JS.jpeg(name), bits, surfel_jpegdec.MAX_ROUNDS_DEFAULT)
    assert np.array_equal(pixels, JS.pixels(name))
    return info


# ------------------------------------------------------------------------------------------------ 1. the decoder
@pytest.mark.parametrize("name", JS.NAMES)
def test_pixels_equal_pillow_and_counters_equal_the_oracle(torch, JD, name):
    data, want = JS.jpeg(name), JS.pixels(name)
    for bits in BITS:
        got = JD.decode_jpeg(data, subseq_bits=bits)
        info = JD.decode_info()
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        first = got.cpu().numpy()
        assert np.array_equal(first, want), (name, bits, np.argwhere(first != want)[:4])
        assert info == oracle_info(name, bits), (name, bits, info)
        assert np.array_equal(JD.decode_jpeg(data, subseq_bits=bits).cpu().numpy(), first), (name, bits, "second run")


def test_a_file_of_the_projects_own_encoder(torch, JD):
    """surfel_video.jpeg_bytes: 4:2:0, standard tables, one restart interval per MCU row"""
    import surfel_video
    img = JS.ramp_noise(2, 40, 56, 3, 0.5)
    data = surfel_video.jpeg_bytes(torch.from_numpy(img).cuda(), quality=90)
    desc = JD.parse(data)
    assert desc is not None and desc.restart_interval == desc.mcux and desc.nintervals == desc.mcuy == 3
    want = JS.pillow(data)
    for bits in BITS:
        got = JD.decode_jpeg(data, subseq_bits=bits).cpu().numpy()
        assert np.array_equal(got, want), bits
        assert JD.decode_info() == JO.decode(data, bits, JD.MAX_ROUNDS_DEFAULT)[1], bits


def test_the_synchronisation_is_exercised(torch, JD):
    data = JS.jpeg(JS.SYNC)
    assert JD.parse(data).restart_interval == 0
    JD.decode_jpeg(data, subseq_bits=128)
    info = JD.decode_info()
    assert info["rounds"] >= 2 and info["subsequences"] >= 50 and info["rounds"] == oracle_info(JS.SYNC, 128)["rounds"], info
    # one round cannot verify a blind start: a status, and an exception
    with pytest.raises(JD.JpegNotDecoded, match="not converged") as e:
        JD.decode_jpeg(data, subseq_bits=128, max_rounds=1)
    assert e.value.reason == "not converged"
    assert JD.decode_info() == JO.decode(data, 128, 1)[1] and JD.decode_info()["status"] == "not converged"
    # at the fixed point's own round count the cap is just enough: the round behind the last change verifies it
    rounds = info["rounds"]
    assert np.array_equal(JD.decode_jpeg(data, subseq_bits=128, max_rounds=rounds + 1).cpu().numpy(), JS.pixels(JS.SYNC))
    with pytest.raises(JD.JpegNotDecoded, match="not converged"):
        JD.decode_jpeg(data, subseq_bits=128, max_rounds=rounds)


def test_damaged_and_unsupported_files_are_statuses(torch, JD):
    cut = JS.truncated()
    with pytest.raises(JD.JpegNotDecoded, match="damaged"):
        JD.decode_jpeg(cut, subseq_bits=128)
    assert JD.decode_info() == JO.decode(cut, 128, JD.MAX_ROUNDS_DEFAULT)[1] and JD.decode_info()["status"] == "damaged"
    with pytest.raises(JD.JpegNotDecoded, match="damaged"):
        JD.decode_jpeg(cut)
    # a stream that ends inside its last block, or behind it without EOI: never "ok" with wrong pixels
    for name in JS.CUT_NAMES:
        for k, keep_eoi in ((0, False), (1, False), (2, False), (3, False), (1, True), (2, True), (3, True)):
            short = JS.cut_before_eoi(name, k, keep_eoi)
            for bits in BITS:
                with pytest.raises(JD.JpegNotDecoded, match="damaged"):
                    JD.decode_jpeg(short, subseq_bits=bits)
                assert JD.decode_info() == JO.decode(short, bits, JD.MAX_ROUNDS_DEFAULT)[1], (name, k, keep_eoi, bits)
    lost = JS.jpeg("rgb-48x48-420-rows").replace(b"\xff\xd1", b"\x00\x00", 1)      # one restart marker gone
    with pytest.raises(JD.JpegNotDecoded, match="damaged"):
        JD.decode_jpeg(lost, subseq_bits=128)
    assert JD.decode_info() == {"status": "damaged", "rounds": 0, "subsequences": 0, "blocks": 0}
    with pytest.raises(JD.JpegNotDecoded, match="not supported"):
        JD.decode_jpeg(JS.progressive())
    # the decoder is whole afterwards
    assert np.array_equal(JD.decode_jpeg(JS.jpeg(JS.SYNC)).cpu().numpy(), JS.pixels(JS.SYNC))


def test_decode_checks_its_buffers(torch, JD):
    data = JS.jpeg("rgb-33x17-420")
    desc = JD.parse(data)
    file = JD.upload(data)
    need = JD.scratch_bytes(desc, 128)
    out = torch.full((17, 33, 3), 0xCD, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"\(-1\): jpegdec_decode: scratch"):
        JD.launch(desc, file, 128, out=out, scratch=torch.empty(need - 16, dtype=torch.uint8, device="cuda"), status=status)
    with pytest.raises(RuntimeError, match=r"\(-1\): jpegdec_decode: the entropy-coded segment"):
        JD.launch(desc, file[:-1], 128, out=out, status=status)
    with pytest.raises(RuntimeError, match=r"\(-1\): jpegdec_decode: bad arguments"):
        JD.launch(desc, file, 128, max_rounds=65, out=out, status=status)
    with pytest.raises(RuntimeError, match="HIP device"):
        JD.launch(desc, file, 128, out=out.cpu(), status=status)
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all()) and status.tolist() == [-7] * 4
    # stage by stage in one scratch gives the same pixels as one call
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    for k in range(len(JD.STAGE_NAMES)):
        JD.launch(desc, file, 128, stages=1 << k, out=out, scratch=scratch, status=status)
    assert status.tolist()[0] == 0 and np.array_equal(out.cpu().numpy(), JS.pixels("rgb-33x17-420"))


def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "jpegdec_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "jpegdec_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 16, p.stdout


# ------------------------------------------------------------------------------------------------ 2. capture loading
def write_capture(root, files, points=40):
    """a COLMAP text model whose images are `files` {name: (bytes, width, height)}: one PINHOLE camera per image"""
    sparse = os.path.join(root, "sparse", "0")
    os.makedirs(sparse)
    os.makedirs(os.path.join(root, "images"))
    rng = np.random.default_rng(5)
    with open(os.path.join(sparse, "cameras.txt"), "w") as fc, open(os.path.join(sparse, "images.txt"), "w") as fi:
        for k, (name, (data, w, h)) in enumerate(files.items()):
            with open(os.path.join(root, "images", name), "wb") as f:
                f.write(data)
            ang = 2 * np.pi * k / len(files) + 0.1
            R, t = SS.look_at_w2c((3.0 * float(np.cos(ang)), 0.3 * float(np.sin(2 * ang)), 3.0 * float(np.sin(ang))))
            fc.write("%d PINHOLE %d %d %r %r %r %r\n" % (k + 1, w, h, 1.2 * w, 1.2 * w, w / 2.0, h / 2.0))
            fi.write("%d %s %d %s\n\n" % (k + 1, " ".join(repr(float(v)) for v in list(SS.rotmat_to_qvec(R)) + list(t)), k + 1, name))
    with open(os.path.join(sparse, "points3D.txt"), "w") as f:
        for p in range(points):
            xyz, rgb = rng.normal(size=3) * 0.5, rng.integers(0, 256, size=3)
            f.write("%d %r %r %r %d %d %d 0.5 1 0\n" % (p + 1, float(xyz[0]), float(xyz[1]), float(xyz[2]), rgb[0], rgb[1], rgb[2]))
    return root


def _png(a):
    import io
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, "PNG")
    return f.getvalue()


def _same_cameras(a, b):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert x.image_name == y.image_name and x.original_image.shape == y.original_image.shape
        assert bool((x.original_image == y.original_image).all()), x.image_name
        assert (x.gt_alpha_mask is None) == (y.gt_alpha_mask is None)


@pytest.fixture(scope="module")
def mixed_capture(tmp_path_factory):
    """4:2:0, 4:2:2, gray, progressive (outside the decoder's scope), PNG; an upper-case extension; sizes that -r 2 halves unevenly"""
    files = {
        "a_420.jpg": (JS._save(JS.ramp_noise(20, 37, 53, 3, 8), quality=90, subsampling=2), 53, 37),
        "b_gray.jpeg": (JS._save(JS.ramp_noise(21, 37, 53, 1, 8), quality=85), 53, 37),
        "c_progressive.jpg": (JS._save(JS.ramp_noise(22, 37, 53, 3, 8), quality=90, progressive=True), 53, 37),
        "d_plain.png": (_png(JS.ramp_noise(23, 36, 48, 3, 8)), 48, 36),
        "e_422.JPG": (JS._save(JS.ramp_noise(24, 36, 48, 3, 8), quality=95, subsampling=1, optimize=True), 48, 36),
        "f_sync.jpg": (JS.jpeg(JS.SYNC), 40, 56),
    }
    return write_capture(str(tmp_path_factory.mktemp("jpegdec") / "capture"), files)


def test_load_cameras_device_equals_host(torch, mixed_capture, capsys):
    import surfel_scene as SC
    infos = SC.read_scene_info(mixed_capture).train_cameras
    assert [os.path.basename(c.image_path) for c in infos] == ["a_420.jpg", "b_gray.jpeg", "c_progressive.jpg", "d_plain.png", "e_422.JPG", "f_sync.jpg"]
    host = SC.load_cameras(infos, resolution=2, workers=1)
    capsys.readouterr()
    for workers in (1, 4):
        dev = SC.load_cameras(infos, resolution=2, workers=workers, decode="device")
        _same_cameras(host, dev)
        assert capsys.readouterr().out.count("decoded by Pillow") == 1      # the progressive file, reported once
    _same_cameras(SC.load_cameras(infos, resolution=1, workers=2), SC.load_cameras(infos, resolution=1, workers=3, decode="device"))
    assert tuple(host[0].original_image.shape) == (3, 18, 26) and tuple(host[1].original_image.shape) == (1, 18, 26)
    with pytest.raises(ValueError, match="decode"):
        SC.load_cameras(infos, decode="gpu")


def test_load_cameras_falls_back_for_a_stream_that_does_not_converge(torch, mixed_capture, capsys):
    import surfel_scene as SC
    infos = SC.read_scene_info(mixed_capture).train_cameras
    host = SC.load_cameras(infos, resolution=1)
    capsys.readouterr()
    dev = SC.load_cameras(infos, resolution=1, decode="device", decode_options={"subseq_bits": 128, "max_rounds": 1})
    _same_cameras(host, dev)
    out = capsys.readouterr().out
    assert out.count("decoded by Pillow") == 1 and "[ INFO ] 5 of 6 images" in out      # every JPEG file: none converges in one round
    # the default is the host path, and says nothing
    SC.load_cameras(infos, resolution=1)
    assert "Pillow" not in capsys.readouterr().out


def test_a_truncated_file_fails_as_it_does_on_the_host(torch, tmp_path):
    """cut in the middle of the entropy-coded segment, right in front of EOI, and two bytes earlier (inside the last block)"""
    import surfel_scene as SC
    files = {"a_mid.jpg": JS.truncated(), "b_no_eoi.jpg": JS.cut_before_eoi(JS.SYNC, 0), "c_last_block.jpg": JS.cut_before_eoi(JS.SYNC, 2)}
    for name, data in files.items():
        root = write_capture(str(tmp_path / name.split(".")[0]), {name: (data, 40, 56)})
        infos = SC.read_scene_info(root).train_cameras
        errors = []
        for mode in ("host", "device"):
            with pytest.raises(OSError) as e:
                SC.load_cameras(infos, resolution=1, decode=mode)
            errors.append(str(e.value))
        assert errors[0] == errors[1] and "truncated" in errors[0], (name, errors)
    # with the marker kept Pillow decodes what is there: the device hands the file over and the cameras are the host's
    root = write_capture(str(tmp_path / "early_eoi"), {"d.jpg": (JS.cut_before_eoi(JS.SYNC, 2, keep_eoi=True), 40, 56)})
    infos = SC.read_scene_info(root).train_cameras
    _same_cameras(SC.load_cameras(infos, resolution=1), SC.load_cameras(infos, resolution=1, decode="device"))


def test_trainer_cli_with_device_decode(torch, mixed_capture, tmp_path):
    """surfel_trainer.py --decode device in a child process, then surfel_mesh.py --decode device on its model: the ground-truth
    images both export are the files' pixels"""
    import surfel_mesh
    from PIL import Image
    files = {name: (JS._save(JS.ramp_noise(30 + k, 48, 64, 3, 4, 1.0), quality=92, subsampling=2), 64, 48) for k, name in
             enumerate(("v0.jpg", "v1.jpg", "v2.jpg"))}
    root, model = write_capture(str(tmp_path / "capture"), files), str(tmp_path / "model")
    p = subprocess.run([sys.executable, os.path.join(REPO, "2d-gaussian-splatting_amd", "surfel_trainer.py"), "-s", root, "-m", model, "--iterations", "2",
                        "--save_iterations", "2", "--quiet", "--decode", "device"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "surfel_trainer.py: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert os.path.exists(os.path.join(model, "point_cloud", "iteration_2", "point_cloud.ply"))
    import surfel_trainer as TR
    with pytest.raises(SystemExit):
        TR.parse_args(["-s", root, "--decode", "gpu"])
    assert surfel_mesh.main(["-m", model, "-s", root, "--skip_mesh", "--decode", "device"]) == 0
    for k, name in enumerate(files):
        gt = np.asarray(Image.open(os.path.join(model, "train", "ours_2", "gt", "%05d.png" % k)))
        assert np.array_equal(gt, JS.pillow(files[name][0])), name
