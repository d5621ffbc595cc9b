"""GPU checks of the trajectory videos (VIDEO.md): the HIP JPEG encoder byte for byte against the numpy restatement
(tests/video_oracle.py, itself checked against libjpeg in tests/test_video_cpu.py), output alignment and untouched surroundings, guard
pages, the VideoWriter on device frames, render_path with videos end to end, and the CLI in a child process."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import video_oracle as VO
import video_scenes as VS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def SV():
    import surfel_video
    return surfel_video


@functools.lru_cache(maxsize=None)
def oracle(name, quality):
    return VO.encode(VS.scene(name), quality)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the encoder
@pytest.mark.parametrize("name", VS.NAMES)
def test_jpeg_is_byte_equal_to_the_oracle(torch, SV, name):
    img = VS.scene(name)
    d = _dev(torch, img)
    for q in VS.QUALITIES:
        want = oracle(name, q)
        buf, size = SV.encode_jpeg(d, q)
        assert buf.dtype == torch.uint8 and buf.numel() == SV.capacity(*img.shape[:2]) and size.dtype == torch.int64
        assert int(size.item()) == len(want), (name, q)
        assert buf[:len(want)].cpu().numpy().tobytes() == want, (name, q)
        assert SV.jpeg_bytes(d, q) == want, (name, q, "second run")


@pytest.mark.parametrize("name", ["edges-17x33", "noise-150x218"])
def test_output_at_every_alignment_leaves_its_surroundings(torch, SV, name):
    img = VS.scene(name)
    d = _dev(torch, img)
    cap = SV.capacity(*img.shape[:2])
    want = oracle(name, 95)
    for off in range(4):
        buf = torch.full((cap + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        out, size = SV.encode_jpeg(d, 95, out=buf[off:off + cap])
        assert out.data_ptr() % 4 == off and int(size.item()) == len(want)
        host = buf.cpu().numpy()
        assert host[off:off + len(want)].tobytes() == want, (name, off)
        assert np.all(host[:off] == 0xAB) and np.all(host[off + len(want):] == 0xAB), (name, off)      # nothing at or beyond `size`


def test_encode_jpeg_checks_its_buffers(torch, SV):
    d = _dev(torch, VS.scene("edges-17x33"))
    with pytest.raises(ValueError, match="at least"):
        SV.encode_jpeg(d, out=torch.empty(SV.capacity(17, 33) - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="uint8"):
        SV.encode_jpeg(d.float())
    with pytest.raises(RuntimeError, match="quality"):
        SV.encode_jpeg(d, quality=0)


def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "video_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "video_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 4, p.stdout


# ------------------------------------------------------------------------------------------------ 2. the writer
def test_video_writer_on_device_frames(torch, SV, tmp_path):
    frames = VS.frames(12, 37, 51)
    path = str(tmp_path / "v.avi")
    with SV.VideoWriter(path, 37, 51, fps=24, quality=95, ring=2) as vw:
        for f in frames:
            t = _dev(torch, f)
            vw.add_frame(t)
            t.zero_()      # stream-ordered behind the encoder
            del t
    assert vw.frames == vw.submitted == 12
    avi = VO.read_avi(path)
    assert len(avi["frames"]) == 12 and avi["avih"]["total_frames"] == 12 and avi["strh"]["rate"] == 24
    for k, (got, f) in enumerate(zip(avi["frames"], frames)):
        assert got == VO.encode(f, 95), k
    with pytest.raises(ValueError, match="expected"):
        SV.VideoWriter(str(tmp_path / "w.avi"), 37, 51).add_frame(_dev(torch, frames[0][:, :50]))


def test_video_writer_surfaces_the_threads_error(torch, SV, tmp_path):
    frames = VS.frames(5, 37, 51)
    vw = SV.VideoWriter(str(tmp_path / "e.avi"), 37, 51, ring=2)
    append = vw._append

    def failing(data):
        if len(vw._index) == 2:
            raise OSError("disk on fire")
        append(data)
    vw._append = failing
    for f in frames:
        vw.add_frame(_dev(torch, f))      # (the ring keeps turning behind the error)
    with pytest.raises(OSError, match="disk on fire"):
        vw.close()
    assert VO.read_avi(str(tmp_path / "e.avi"))["frames"] == [VO.encode(f, 95) for f in frames[:2]]


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.fixture(scope="module")
def small_state(torch):
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    model = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    bg = torch.zeros(3, device=dev)
    cams = TR.capture_views(model, TR.orbit_cameras(8, 65, 49, device=dev), bg)
    return model, cams, bg, TR.pipeline_params()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def test_render_path_with_videos(torch, SV, small_state, tmp_path):
    import surfel_path as SP
    from surfel_render import render
    model, cams, bg, pipe = small_state
    plain, both, only = str(tmp_path / "plain"), str(tmp_path / "both"), str(tmp_path / "only")
    SP.render_path(model, cams, render, pipe, bg, plain, n_frames=6, vis_normals=True)
    info = {}
    SP.render_path(model, cams, render, pipe, bg, both, n_frames=6, vis_normals=True, video=True, timings=info)
    videos = ["render_traj_%s.avi" % s for s in ("color", "depth", "normal")]
    per_frame = sorted(["renders/%05d.png" % k for k in range(6)] + ["video/depth/%05d.png" % k for k in range(6)] +
                       ["vis/depth_%05d.tiff" % k for k in range(6)] + ["vis/normal_%05d.png" % k for k in range(6)])
    # defaults: the listing tests/test_gpu_path.py expects, nothing else
    assert sorted(os.listdir(plain)) == ["renders", "video", "vis"] and _tree(plain) == per_frame
    assert _tree(both) == sorted(per_frame + videos) and info["files"] == 24 and info["videos"] == ["color", "depth", "normal"]
    for f in per_frame:      # the folders are unchanged by the videos
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(both, f), "rb").read(), f
    for video, pattern in (("color", "renders/%05d.png"), ("depth", "video/depth/%05d.png"), ("normal", "vis/normal_%05d.png")):
        avi = VO.read_avi(os.path.join(both, "render_traj_%s.avi" % video))
        assert len(avi["frames"]) == 6 and (avi["avih"]["width"], avi["avih"]["height"], avi["strh"]["rate"]) == (64, 48, 60)
        for k, data in enumerate(avi["frames"]):
            frame = _png(os.path.join(both, pattern % k))
            assert frame.shape == (48, 64, 3) and data == VO.encode(frame, 95), (video, k)
    SP.render_path(model, cams, render, pipe, bg, only, n_frames=6, vis_normals=True, video_only=True, video_quality=75, fps=30)
    assert _tree(only) == videos
    avi = VO.read_avi(os.path.join(only, "render_traj_color.avi"))
    assert avi["strh"]["rate"] == 30 and avi["frames"] == [VO.encode(_png(os.path.join(both, "renders/%05d.png" % k)), 75) for k in range(6)]
    SP.render_path(model, cams, render, pipe, bg, str(tmp_path / "two"), n_frames=2, video=True)      # without vis_normals: two videos
    assert [f for f in _tree(str(tmp_path / "two")) if f.endswith(".avi")] == videos[:2]


def test_mesh_cli_render_path_with_video(torch, small_state, tmp_path):
    model, cams, bg, pipe = small_state
    root = str(tmp_path / "model")
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
    p = subprocess.run([sys.executable, os.path.join(REPO, "2d-gaussian-splatting_amd", "surfel_mesh.py"), "-m", root, "--render_path", "--skip_mesh",
                        "--video", "--n_frames", "4"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "surfel_mesh.py: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    traj = os.path.join(root, "traj", "ours_7")
    assert sorted(os.listdir(traj)) == ["render_traj_color.avi", "render_traj_depth.avi", "renders", "video", "vis"]
    for video, pattern in (("color", "renders/%05d.png"), ("depth", "video/depth/%05d.png")):
        avi = VO.read_avi(os.path.join(traj, "render_traj_%s.avi" % video))
        assert avi["avih"]["total_frames"] == 4 and avi["frames"] == [VO.encode(_png(os.path.join(traj, pattern % k)), 95) for k in range(4)]
