"""GPU checks of the PNG encoder (PNG.md): the HIP encoder byte for byte against the numpy restatement (tests/png_oracle.py, itself
checked against Pillow and zlib in tests/test_png_cpu.py), input and output alignment and untouched surroundings, buffer checks, guard
pages, FrameWriter(png="device"), render_path and export_image with png="device", and the CLI in a child process."""
import functools
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import png_oracle as PO
import png_scenes as PS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def SG():
    import surfel_png
    return surfel_png


@functools.lru_cache(maxsize=None)
def oracle(name):
    return PO.encode(PS.scene(name))


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the scenes are read-only)


def _decode(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data) if isinstance(data, bytes) else data))
    return a[:, :, None] if a.ndim == 2 else a


def _pillow_file(a):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a).save(f, "PNG")
    return f.getvalue()


# ------------------------------------------------------------------------------------------------ 1. the encoder
@pytest.mark.parametrize("name", PS.NAMES)
def test_png_is_byte_equal_to_the_oracle(torch, SG, name):
    img = PS.scene(name)
    d = _dev(torch, img)
    want = oracle(name)
    buf, size = SG.encode_png(d)
    assert buf.dtype == torch.uint8 and buf.numel() == SG.capacity(*img.shape) and size.dtype == torch.int64
    got = buf[:int(size.item())].cpu().numpy().tobytes()
    assert int(size.item()) == len(want), (name, int(size.item()), len(want))
    assert got == want, (name, next(k for k in range(len(want)) if got[k] != want[k]))
    assert np.array_equal(_decode(got), img)
    assert SG.png_bytes(d) == want, (name, "second run")


@pytest.mark.parametrize("name", ["noise-17x33", "ragged-7x13", "disc-40x40"])
def test_every_alignment_of_input_and_output_leaves_the_surroundings(torch, SG, name):
    img = PS.scene(name)
    cap, nbytes = SG.capacity(*img.shape), img.size
    want = oracle(name)
    flat = torch.from_numpy(np.array(img).reshape(-1))
    for off in range(4):
        src = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
        src[off:off + nbytes] = flat.cuda()
        buf = torch.full((cap + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0 and src.data_ptr() % 4 == 0
        pix = src[off:off + nbytes].view(*img.shape)
        out, size = SG.encode_png(pix, out=buf[(3 - off):(3 - off) + cap])
        assert pix.data_ptr() % 4 == off and out.data_ptr() % 4 == 3 - off and int(size.item()) == len(want)
        host = buf.cpu().numpy()
        lo = 3 - off
        assert host[lo:lo + len(want)].tobytes() == want, (name, off)
        assert np.all(host[:lo] == 0xAB) and np.all(host[lo + len(want):] == 0xAB), (name, off)      # nothing at or beyond `size`


def test_encode_png_checks_its_buffers(torch, SG):
    import surfel_native as n
    img = PS.scene("noise-17x33")
    d = _dev(torch, img)
    cap, scr = SG.capacity(17, 33, 3), SG.scratch_bytes(17, 33, 3)
    with pytest.raises(ValueError, match="at least"):
        SG.encode_png(d, out=torch.empty(cap - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="at least"):
        SG.encode_png(d, scratch=torch.empty(scr - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="uint8"):
        SG.encode_png(d.float())
    with pytest.raises(ValueError, match="1 or 3"):
        SG.encode_png(torch.zeros((4, 4, 2), dtype=torch.uint8, device="cuda"))
    # the library itself: one byte short is SURFEL_E_INVALID before any launch — the sentinel-filled buffers stay as they were
    out = torch.full((cap,), 0xCD, dtype=torch.uint8, device="cuda")
    scratch = torch.full((scr,), 0xCD, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for kw in (dict(capacity=cap - 1), dict(scratch_bytes=scr - 1)):
        a = dict(capacity=cap, scratch_bytes=scr)
        a.update(kw)
        with pytest.raises(RuntimeError, match=r"\(-1\): png_encode: (capacity|scratch)"):
            n.call(d.device, "surfel_png_encode", 17, 33, 3, d, out, a["capacity"], size, scratch, a["scratch_bytes"])
    for shape in ((17, 33, 2), (0, 33, 3)):
        with pytest.raises(RuntimeError, match=r"\(-1\): png_encode: bad arguments"):
            n.call(d.device, "surfel_png_encode", shape[0], shape[1], shape[2], d, out, cap, size, scratch, scr)
    with pytest.raises(n.LimitError, match="limits"):
        n.call(d.device, "surfel_png_encode", 17, 1 << 20, 3, d, out, cap, size, scratch, scr)
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all()) and bool((scratch == 0xCD).all()) and int(size.item()) == -7
    # an explicit scratch and size word are used as given
    buf, got = SG.encode_png(d, out=out, scratch=scratch, size=size)
    assert got is size and buf is out and out[:int(size.item())].cpu().numpy().tobytes() == oracle("noise-17x33")


def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "png_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "png_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 4, p.stdout


# ------------------------------------------------------------------------------------------------ 2. the writer
def _frames(count, H, W):
    rng = np.random.default_rng(11)
    out = []
    for k in range(count):
        y, x = np.mgrid[0:H + (k % 3), 0:W]
        a = np.stack([(x * 4 + k * 9) % 256, (y * 6) % 256, np.where(x > W // 2, 255, (x + y + k) % 256)], axis=2).astype(np.uint8)
        a[: H // 3] = rng.integers(0, 256, size=a[: H // 3].shape, dtype=np.uint8)
        out.append(a[:, :, :1].copy() if k % 4 == 3 else a)      # gray frames among the RGB ones, three heights
    return out


def test_frame_writer_encodes_device_frames_on_the_device(torch, SG, tmp_path):
    import surfel_path as SP
    frames = _frames(10, 37, 51)
    depth = np.linspace(0, 5, 37 * 51, dtype=np.float32).reshape(37, 51)
    for mode in ("pillow", "device"):
        os.makedirs(str(tmp_path / mode))
        with SP.FrameWriter(workers=2, ring=3, png=mode) as fw:      # (10 frames through 3 slots: the ring wraps)
            for k, a in enumerate(frames):
                t = _dev(torch, a)
                fw.submit(str(tmp_path / mode / ("%02d.png" % k)), t)
                t.zero_()      # stream-ordered behind the encoder / the copy
                del t
            fw.submit(str(tmp_path / mode / "host.png"), torch.from_numpy(np.array(frames[0])))      # a host tensor: Pillow in both modes
            fw.submit(str(tmp_path / mode / "depth.tiff"), _dev(torch, depth))
        assert fw.frames == 12
    for k, a in enumerate(frames):
        dev_file = open(str(tmp_path / "device" / ("%02d.png" % k)), "rb").read()
        assert dev_file == PO.encode(a), k                                    # the device's file, byte for byte
        assert np.array_equal(_decode(dev_file), a)
        assert np.array_equal(_decode(str(tmp_path / "pillow" / ("%02d.png" % k))), a)
        assert open(str(tmp_path / "pillow" / ("%02d.png" % k)), "rb").read() == _pillow_file(a)      # the default: Pillow's own bytes
    for f in ("host.png", "depth.tiff"):
        assert open(str(tmp_path / "pillow" / f), "rb").read() == open(str(tmp_path / "device" / f), "rb").read(), f


def test_frame_writer_surfaces_a_workers_error(torch, tmp_path):
    import surfel_path as SP
    frames = _frames(6, 37, 51)
    fw = SP.FrameWriter(workers=1, ring=2, png="device")
    store = fw._store

    def failing(path, data):
        if path.endswith("02.png"):
            raise OSError("disk on fire")
        store(path, data)
    fw._store = failing
    for k, a in enumerate(frames):
        fw.submit(str(tmp_path / ("%02d.png" % k)), _dev(torch, a))      # (the ring keeps turning behind the error)
    with pytest.raises(OSError, match="disk on fire"):
        fw.close()
    assert sorted(os.listdir(str(tmp_path))) == ["%02d.png" % k for k in (0, 1, 3, 4, 5)]
    assert open(str(tmp_path / "05.png"), "rb").read() == PO.encode(frames[5])


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.fixture(scope="module")
def small_state(torch):
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    model = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    bg = torch.zeros(3, device=dev)
    cams = TR.capture_views(model, TR.orbit_cameras(8, 65, 49, device=dev), bg)
    return model, cams, bg, TR.pipeline_params()


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def _same_frames(plain, device):
    """the same names; TIFFs byte-identical; PNGs: the default run's are Pillow's own bytes, the device run's decode to the same pixels
    and are the restatement's bytes"""
    assert _tree(plain) == _tree(device) and _tree(plain)
    for f in _tree(plain):
        a, b = open(os.path.join(plain, f), "rb").read(), open(os.path.join(device, f), "rb").read()
        if f.endswith(".tiff"):
            assert a == b, f
            continue
        pa, pb = _decode(a), _decode(b)
        assert np.array_equal(pa, pb), f
        assert a == _pillow_file(pa), f
        assert b == PO.encode(pb) and b[:8] == a[:8] and b != a, f


def test_render_path_with_device_png(torch, small_state, tmp_path):
    import surfel_path as SP
    from surfel_render import render
    model, cams, bg, pipe = small_state
    plain, device = str(tmp_path / "plain"), str(tmp_path / "device")
    SP.render_path(model, cams, render, pipe, bg, plain, n_frames=5, vis_normals=True)
    info = {}
    SP.render_path(model, cams, render, pipe, bg, device, n_frames=5, vis_normals=True, png="device", timings=info)
    assert info["files"] == 20 and len(_tree(device)) == 20
    _same_frames(plain, device)
    with pytest.raises(ValueError, match="pillow"):
        SP.render_path(model, cams, render, pipe, bg, str(tmp_path / "bad"), n_frames=2, png="zlib")


def test_export_image_with_device_png(torch, small_state, tmp_path):
    import surfel_mesh
    from surfel_render import render
    model, cams, bg, pipe = small_state
    ext = surfel_mesh.GaussianExtractor(model, render, pipe)
    ext.reconstruction(cams[:3])
    plain, device, vis = str(tmp_path / "plain"), str(tmp_path / "device"), str(tmp_path / "vis")
    ext.export_image(plain)
    ext.export_image(device, png="device")
    assert sorted(os.listdir(device)) == ["gt", "renders"] and len(_tree(device)) == 6
    _same_frames(plain, device)
    ext.export_image(vis, vis=True, png="device")
    assert sorted(os.listdir(vis)) == ["gt", "renders", "vis"]
    for f in _tree(device):
        assert open(os.path.join(device, f), "rb").read() == open(os.path.join(vis, f), "rb").read(), f


def test_mesh_cli_render_path_with_device_png(torch, small_state, tmp_path):
    model, cams, bg, pipe = small_state
    roots = {}
    for mode in ("pillow", "device"):
        root = roots[mode] = str(tmp_path / mode)
        os.makedirs(os.path.join(root, "point_cloud", "iteration_7"))
        model.save_ply(os.path.join(root, "point_cloud", "iteration_7", "point_cloud.ply"))
        entries = []
        for k, cam in enumerate(cams):
            Rt = np.eye(4)
            Rt[:3, :3], Rt[:3, 3] = np.asarray(cam.R, np.float64).T, np.asarray(cam.T, np.float64)
            c2w = np.linalg.inv(Rt)
            entries.append({"id": k, "img_name": cam.image_name, "width": 65, "height": 49, "position": c2w[:3, 3].tolist(),
                            "rotation": [r.tolist() for r in c2w[:3, :3]], "fx": 65 / (2 * math.tan(cam.FoVx / 2)), "fy": 49 / (2 * math.tan(cam.FoVy / 2))})
        with open(os.path.join(root, "cameras.json"), "w") as f:
            json.dump(entries, f)
    procs = {mode: subprocess.Popen([sys.executable, os.path.join(REPO, "2d-gaussian-splatting_amd", "surfel_mesh.py"), "-m", roots[mode], "--render_path",
                                     "--skip_mesh", "--n_frames", "3"] + (["--png", "device"] if mode == "device" else []),
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for mode in roots}
    for mode, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, "surfel_mesh.py (%s): rc %d\n%s\n%s" % (mode, p.returncode, out[-2000:], err[-2000:])
    plain, device = (os.path.join(roots[mode], "traj", "ours_7") for mode in ("pillow", "device"))
    assert sorted(os.listdir(device)) == ["renders", "video", "vis"] and len(_tree(device)) == 9
    _same_frames(plain, device)
