"""GPU checks of the trajectory renderer (RENDER.md): the quantiser bit for bit and the selection value for value against the numpy
oracle (tests/path_oracle.py, itself equal to the reference's expressions: tests/test_path_cpu.py), the depth colouring within the
one-step allowance a device logf needs, guard pages, render_path / export_image(vis=True) end to end, and the CLI in a child process."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import path_oracle as PO
import path_scenes as PS

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def SP():
    import surfel_path
    return surfel_path


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. quantise
@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 5, 7), (1, 3, 129), (3, 33, 65), (3, 16, 260)], ids=lambda s: "%dx%dx%d" % s)
def test_quantize_is_bit_equal_to_the_oracle(torch, SP, shape):
    Cn, H, W = shape
    n = H * W * Cn
    for seed, (scale, bias) in enumerate(((1.0, 0.0), (0.5, 0.5))):
        a = PS.frame(40 + seed, Cn, H, W, normal=bias != 0.0)
        want = PO.quantize(a, scale, bias)
        d = _dev(torch, a)
        got = SP.quantize_u8(d, scale, bias)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, Cn)
        assert np.array_equal(got.cpu().numpy(), want), (shape, scale, bias)
        for off in range(4):      # the output at every byte offset mod 4; the bytes around it stay as they were
            buf = torch.full((n + 8,), 0xAB, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 4 == 0
            out = SP.quantize_u8(d, scale, bias, out=buf[off:off + n])
            assert out.data_ptr() % 4 == off
            host = buf.cpu().numpy()
            assert np.array_equal(host[off:off + n].reshape(H, W, Cn), want), (shape, scale, bias, off)
            assert np.all(host[:off] == 0xAB) and np.all(host[off + n:] == 0xAB), (shape, off)
    if Cn == 3:      # a [H, W] plane is C = 1
        assert np.array_equal(SP.quantize_u8(d[0]).cpu().numpy(), PO.quantize(a[:1], 1.0, 0.0))


# ------------------------------------------------------------------------------------------------ 2. order statistics
@pytest.mark.parametrize("kind", PS.ORDER_KINDS)
def test_order_stats_equal_the_sorted_array(torch, SP, kind):
    for n in PS.ORDER_SIZES:
        x = PS.order_data(kind, n)
        ranks = PS.order_ranks(n)
        want = PO.order_stats(x, ranks)
        d = _dev(torch, x)
        got = SP.order_stats(d, ranks).cpu().numpy()
        assert got.dtype == np.float32 and np.all(got == want), (kind, n, ranks, got, want)      # (== : -0 and +0 tie)
        again = SP.order_stats(d, ranks).cpu().numpy()
        assert got.tobytes() == again.tobytes(), (kind, n)
        for q in ([3, 97], [0, 50, 100]):
            np.testing.assert_allclose(SP.percentiles(d, q), np.percentile(x, q), rtol=1e-12, atol=0, err_msg="%s %d %s" % (kind, n, q))
        if n > 4:      # an input that starts at every 4-byte offset of a 16-byte line (the vector loads' head)
            for off in (1, 2, 3):
                assert np.all(SP.order_stats(d[off:], [0, n - off - 1]).cpu().numpy() == PO.order_stats(x[off:], [0, n - off - 1])), (kind, n, off)


def test_order_stats_put_nan_last_and_take_eight_ranks(torch, SP):
    x = PS.order_data("mixed", 4097)
    x[[5, 77, 4000]] = np.nan
    x[100] = np.float32(np.uint32(0xFFC00001).view(np.float32))      # a negative NaN sorts last too
    ranks = [0, 1, 2000, 4092, 4093, 4094, 4095, 4096]
    got = SP.order_stats(_dev(torch, x), ranks).cpu().numpy()
    want = PO.order_stats(x, ranks)
    assert np.isnan(want[4:]).all() and not np.isnan(want[:4]).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(got[:4] == want[:4])
    assert np.isnan(SP.percentiles(_dev(torch, x), [3, 97])).all()       # as np.percentile answers when the data holds a NaN
    d = _dev(torch, x[:9])
    for bad in ([3, 2], [0, 9], [-1, 0], list(range(9))):
        with pytest.raises((RuntimeError, ValueError)):
            SP.order_stats(d, bad)


# ------------------------------------------------------------------------------------------------ 3. depth colouring
def _bins(rgb):
    """table index of every pixel (-1 = black); the table's 256 colours are distinct"""
    tab = PO.turbo_table().astype(np.int64)
    code = tab[:, 0] | tab[:, 1] << 8 | tab[:, 2] << 16
    assert len(set(code.tolist())) == 256 and 0 not in code
    lut = {int(c): k for k, c in enumerate(code)}
    lut[0] = -1
    px = rgb.astype(np.int64)
    return np.vectorize(lambda c: lut[c])(px[..., 0] | px[..., 1] << 8 | px[..., 2] << 16)


@pytest.mark.parametrize("H, W", [(37, 53), (48, 80)])
def test_depth_turbo_within_one_step_of_the_oracle(torch, SP, H, W):
    d = PS.depth_frame(H, H, W, zero_frac=0.009)
    d.reshape(-1)[7] = np.nan
    dd = _dev(torch, d)
    lo, hi = SP.depth_limits(dd)
    assert math.isnan(lo) and math.isnan(hi)                 # np.percentile answers NaN for data that holds one, and so do we
    d0 = np.where(np.isnan(d), np.float32(1.0), d)           # the limits of the frame without its NaN
    lo, hi = SP.depth_limits(_dev(torch, d0))
    assert (lo, hi) == pytest.approx(tuple(np.log(np.percentile(d0, [3, 97]))), rel=1e-12, abs=0) and np.isfinite(lo) and lo < hi
    got = SP.colorize_depth(dd, lo, hi)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
    got = got.cpu().numpy()
    idx, black = PO.turbo_index(d, lo, hi)
    gb = _bins(got)
    assert np.array_equal(gb < 0, black) and black.sum() == 1 and black.reshape(-1)[7]      # the NaN pixel is black, nothing else
    step = np.abs(gb - idx)[~black]
    differ = int((step != 0).sum())
    print("depth_turbo %dx%d: %d of %d pixels one table step from the fp64 oracle" % (H, W, differ, H * W))
    assert step.max() <= 1
    assert differ <= max(2, int(0.001 * H * W))
    assert (d == 0).sum() >= 1 and np.all(got[d == 0] == PO.turbo_table()[0])      # 0.9 % holes: log(0) = -inf clips to the first entry
    # at every byte offset of the output
    n = H * W * 3
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 0xCD, dtype=torch.uint8, device="cuda")
        SP.colorize_depth(dd, lo, hi, out=buf[off:off + n])
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + n].reshape(H, W, 3), got) and np.all(host[:off] == 0xCD) and np.all(host[off + n:] == 0xCD)


def test_depth_turbo_black_frames(torch, SP):
    H, W = 37, 53
    holes = PS.depth_frame(3, H, W, zero_frac=0.08)
    lo, hi = SP.depth_limits(_dev(torch, holes))
    assert lo == -math.inf and math.isfinite(hi)             # more than 3 % of the frame is empty
    assert not SP.colorize_depth(_dev(torch, holes), lo, hi).any()
    assert not SP.colorize_depth(_dev(torch, PS.depth_frame(4, H, W)), lo, hi).any()      # ... and every later frame of that video
    nan = np.full((H, W), np.nan, np.float32)
    assert not SP.colorize_depth(_dev(torch, nan), 0.0, 1.0).any()
    neg = np.full((H, W), -2.0, np.float32)                  # log of a negative depth is NaN
    assert not SP.colorize_depth(_dev(torch, neg), 0.0, 1.0).any()
    const = np.full((H, W), 1.0, np.float32)                 # hi == lo and every pixel on it: 0 / 0
    lo, hi = SP.depth_limits(_dev(torch, const))
    assert lo == hi == 0.0
    assert not SP.colorize_depth(_dev(torch, const), lo, hi).any()
    assert np.array_equal(SP.colorize_depth(_dev(torch, const), lo, hi).cpu().numpy(), PO.depth_turbo(const, lo, hi))


# ------------------------------------------------------------------------------------------------ 4. guard pages
def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "path_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "path_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 11, p.stdout


# ------------------------------------------------------------------------------------------------ 5. end to end
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


def test_render_path_end_to_end(torch, SP, small_state, tmp_path):
    from surfel_render import render
    model, cams, bg, pipe = small_state
    out = str(tmp_path / "traj")
    info = {}
    traj = SP.render_path(model, cams, render, pipe, bg, out, n_frames=6, vis_normals=True, timings=info)
    assert len(traj) == 6 and info["files"] == 24
    names = ["%05d.png" % k for k in range(6)]
    assert sorted(os.listdir(os.path.join(out, "renders"))) == names and sorted(os.listdir(os.path.join(out, "video", "depth"))) == names
    assert sorted(os.listdir(os.path.join(out, "vis"))) == sorted(["depth_%05d.tiff" % k for k in range(6)] + ["normal_%05d.png" % k for k in range(6)])
    assert not os.path.exists(os.path.join(out, "gt"))
    lo = hi = None
    for k, cam in enumerate(traj):
        assert (cam.image_height, cam.image_width) == (48, 64)
        with torch.no_grad():
            pkg = render(cam, model, pipe, bg)      # a separate render of the same path camera
        depth = pkg["surf_depth"][0].cpu().numpy()
        rgb = _png(os.path.join(out, "renders", names[k]))
        assert rgb.shape == (48, 64, 3) and np.array_equal(rgb, PO.quantize(pkg["render"].cpu().numpy()))
        assert rgb.any()                              # the path looks at the object
        tif = _png(os.path.join(out, "vis", "depth_%05d.tiff" % k))
        assert tif.dtype == np.float32 and tif.shape == (48, 64) and tif.tobytes() == depth.tobytes()
        nrm = _png(os.path.join(out, "vis", "normal_%05d.png" % k))
        assert np.array_equal(nrm, PO.quantize(pkg["rend_normal"].cpu().numpy(), 0.5, 0.5))
        if k == 0:
            with np.errstate(divide="ignore"):
                lo, hi = np.log(np.percentile(depth, [3, 97]))
        col = _png(os.path.join(out, "video", "depth", names[k]))
        idx, black = PO.turbo_index(depth, lo, hi)
        if black.all():
            assert not col.any()
        else:
            gb = _bins(col)
            assert np.array_equal(gb < 0, black) and np.abs(gb - idx)[~black].max() <= 1
            assert int((gb != idx)[~black].sum()) <= max(2, int(0.001 * 48 * 64))


def test_export_image_with_and_without_vis(torch, small_state, tmp_path):
    import surfel_mesh
    from surfel_render import render
    model, cams, bg, pipe = small_state
    ext = surfel_mesh.GaussianExtractor(model, render, pipe)
    ext.reconstruction(cams[:3])
    plain, vis = str(tmp_path / "plain"), str(tmp_path / "vis")
    ext.export_image(plain)
    assert sorted(os.listdir(plain)) == ["gt", "renders"]
    ext.export_image(vis, vis=True)
    assert sorted(os.listdir(vis)) == ["gt", "renders", "vis"]
    for k in range(3):
        for folder in ("gt", "renders"):
            a, b = _png(os.path.join(plain, folder, "%05d.png" % k)), _png(os.path.join(vis, folder, "%05d.png" % k))
            assert a.shape == (49, 65, 3) and np.array_equal(a, b), (folder, k)
        tif = _png(os.path.join(vis, "vis", "depth_%05d.tiff" % k))
        assert tif.dtype == np.float32 and tif.tobytes() == ext.depthmaps[k][0].cpu().numpy().tobytes()
    assert sorted(os.listdir(os.path.join(vis, "vis"))) == ["depth_%05d.tiff" % k for k in range(3)]


def test_frame_writer_takes_device_tensors(torch, SP, tmp_path):
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, size=(21 + k, 30, 3), dtype=np.uint8) for k in range(10)]
    with SP.FrameWriter(workers=2, ring=3) as fw:
        for k, a in enumerate(frames):
            t = _dev(torch, a)
            fw.submit(str(tmp_path / ("%02d.png" % k)), t)
            t.zero_()      # stream-ordered behind the copy
            del t
    for k, a in enumerate(frames):
        assert np.array_equal(_png(str(tmp_path / ("%02d.png" % k))), a)
    assert all(b is None or b.is_pinned() for b in fw._buffers)


# ------------------------------------------------------------------------------------------------ 6. the CLI, in a fresh process
def test_mesh_cli_render_path(torch, small_state, tmp_path):
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
                        "--n_frames", "4"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "surfel_mesh.py: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    traj = os.path.join(root, "traj", "ours_7")
    names = ["%05d.png" % k for k in range(4)]
    assert sorted(os.listdir(traj)) == ["renders", "video", "vis"]
    assert sorted(os.listdir(os.path.join(traj, "renders"))) == names == sorted(os.listdir(os.path.join(traj, "video", "depth")))
    assert sorted(os.listdir(os.path.join(traj, "vis"))) == ["depth_%05d.tiff" % k for k in range(4)]
    assert _png(os.path.join(traj, "renders", names[0])).shape == (48, 64, 3)
    assert not any(f.endswith(".ply") for _, _, files in os.walk(os.path.join(root, "train")) for f in files) and not os.path.exists(os.path.join(root, "test"))
