"""GPU checks of the live viewer (VIEWER.md): net_image of every mode against the numpy restatement (tests/view_oracle.py, itself equal
to the reference's bytes: tests/test_view_cpu.py), the stated rules for maps without a range, run-to-run identity, guard pages, and the
serve loop end to end over socket.socketpair() — frames equal to a direct render, and a training that a viewer watches ending in the
same parameters as one that nobody watches."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import path_oracle as PO
import view_oracle as VO
import view_scenes as VS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_INDETERMINATE = 0.01      # of a frame's pixels (tests/test_view_cpu.py)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def SV():
    import surfel_view
    return surfel_view


def _dev(torch, pkg):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pkg.items()}


def _compare(got, pkg, mode, what):
    want, loose = VO.net_image(pkg, mode)
    differ = (got != want).any(axis=2)
    print("%s %s: %d indeterminate, %d differing pixels of %d" % (what, VS.RENDER_ITEMS[mode], int(loose.sum()), int(differ.sum()), differ.size))
    assert loose.mean() <= MAX_INDETERMINATE, (what, mode, int(loose.sum()))
    assert not (differ & ~loose).any(), (what, mode, np.argwhere(differ & ~loose)[:5])
    if VS.RENDER_ITEMS[mode] in ("RGB", "Normal"):
        assert not differ.any(), (what, mode)


# ------------------------------------------------------------------------------------------------ 1. every mode against the oracle
@pytest.mark.parametrize("shape", VS.GPU_SHAPES, ids=lambda s: "%dx%d" % s)
def test_net_image_matches_the_oracle(torch, SV, shape):
    H, W = shape
    pkg = VS.package(H, W)
    d = _dev(torch, pkg)
    for mode, name in enumerate(VS.RENDER_ITEMS):
        got = SV.net_image(d, mode)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3) and got.is_cuda
        _compare(got.cpu().numpy(), pkg, mode, "%dx%d" % shape)
        assert torch.equal(SV.net_image(d, name.lower()), got)      # by name
    if shape == (23, 37):      # the output at every byte offset mod 4; the bytes around it stay as they were
        n = H * W * 3
        for mode in (3, 5):
            want = SV.net_image(d, mode).cpu().numpy()
            for off in range(4):
                buf = torch.full((n + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                assert buf.data_ptr() % 4 == 0
                out = SV.net_image(d, mode, out=buf[off:off + n])
                assert out.data_ptr() % 4 == off
                host = buf.cpu().numpy()
                assert np.array_equal(host[off:off + n].reshape(H, W, 3), want), (mode, off)
                assert np.all(host[:off] == 0xAB) and np.all(host[off + n:] == 0xAB), (mode, off)
        with pytest.raises(ValueError, match="contiguous uint8"):
            SV.net_image(d, 1, out=torch.empty(n + 1, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------ 2. maps without a range
def test_special_frames_follow_the_stated_rules(torch, SV):
    H, W = 33, 130
    tab = PO.turbo_table()
    base = VS.package(H, W)
    rng = np.random.default_rng(4)
    entry0 = np.broadcast_to(tab[0], (H, W, 3))

    def run(pkg, mode):
        return SV.net_image(_dev(torch, pkg), mode).cpu().numpy()
    # a constant map: hi == lo, every t is NaN, every pixel takes entry 0; a constant image has no edges away from its border
    const = dict(base, surf_depth=np.full((1, H, W), 2.5, np.float32), rend_alpha=np.zeros((1, H, W), np.float32),
                 render=np.zeros((3, H, W), np.float32))
    assert np.array_equal(run(const, 3), entry0) and np.array_equal(run(const, 1), entry0) and np.array_equal(run(const, 4), entry0)
    flat = dict(base, render=np.full((3, H, W), 0.5, np.float32))      # the zero padding makes the border an edge
    got = run(flat, 4)
    assert np.array_equal(got[1:-1, 1:-1], entry0[1:-1, 1:-1]) and np.array_equal(got[0, 0], tab[255]) and (got[0] != tab[0]).any()
    _compare(got, flat, 4, "flat")
    # NaNs: ignored by min and max, the pixels themselves take entry 0; the others are coloured as if the NaNs were not there
    holes = rng.random((H, W)) < 0.1
    nan = dict(base, surf_depth=np.where(holes, np.nan, base["surf_depth"][0]).astype(np.float32)[None],
               render=np.where(holes[None] & (np.arange(3) == 1)[:, None, None], np.nan, base["render"]).astype(np.float32))
    for mode in (3, 4):      # (Edge: the Sobel stencil skips its centre, so it is a hole's eight neighbours that take entry 0)
        got = run(nan, mode)
        _compare(got, nan, mode, "nan")
        dead = holes if mode == 3 else np.isnan(VO.gradient(nan["render"]))
        assert holes.sum() > 100 and (~dead).sum() > 100 and np.array_equal(got[dead], np.broadcast_to(tab[0], (int(dead.sum()), 3)))
    idx, _ = VO.colour_index(nan["surf_depth"][0])
    assert idx[~holes].min() == 0 and idx[~holes].max() == 255
    assert np.array_equal(run(dict(base, surf_depth=np.full((1, H, W), np.nan, np.float32)), 3), entry0)
    # +-inf: the range is not finite, every t is 0 or NaN, every pixel takes entry 0
    for special in (np.inf, -np.inf):
        d = base["surf_depth"].copy()
        d[0, 7, 9] = special
        got = run(dict(base, surf_depth=d), 3)
        assert np.array_equal(got, entry0), special
        r = base["render"].copy()
        r[2, 20, 100] = special      # its neighbours' gradients are inf or NaN
        broken = dict(base, render=r)
        got = run(broken, 4)
        assert np.array_equal(got, entry0), special
        _compare(got, broken, 4, "inf")


def test_two_runs_give_identical_bytes(torch, SV):
    d = _dev(torch, VS.package(180, 320))
    for mode in range(6):
        first = SV.net_image(d, mode).clone()
        torch.empty(1 << 20, dtype=torch.uint8, device="cuda").fill_(0x5A)      # (a different history of the scratch's memory)
        for _ in range(3):
            assert torch.equal(SV.net_image(d, mode), first), mode


# ------------------------------------------------------------------------------------------------ 3. guard pages
def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "view_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "view_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 10, p.stdout


# ------------------------------------------------------------------------------------------------ 4. end to end
def _pair():
    a, b = socket.socketpair()
    a.settimeout(10.0); b.settimeout(10.0)
    return a, b


def _recv_exactly(sock, n):
    got = bytearray()
    while len(got) < n:
        piece = sock.recv(n - len(got))
        assert piece, "the viewer side closed after %d of %d bytes" % (len(got), n)
        got += piece
    return bytes(got)


def _recv_json(sock):
    return json.loads(_recv_exactly(sock, int.from_bytes(_recv_exactly(sock, 4), "little")).decode())


def _recv_frame(sock, W, H):
    image = np.frombuffer(_recv_exactly(sock, W * H * 3), np.uint8).reshape(H, W, 3)
    verify = _recv_exactly(sock, int.from_bytes(_recv_exactly(sock, 4), "little")).decode("ascii")
    return image, verify, _recv_json(sock)


def _minicam(torch, SV, msg):
    wvt = np.array(msg["view_matrix"], np.float32).reshape(4, 4) * np.array([1, -1, -1, 1], np.float32)
    full = np.array(msg["view_projection_matrix"], np.float32).reshape(4, 4) * np.array([1, -1, 1, 1], np.float32)
    return SV.MiniCam(msg["resolution_x"], msg["resolution_y"], msg["fov_y"], msg["fov_x"], msg["z_near"], msg["z_far"],
                      torch.from_numpy(wvt).cuda(), torch.from_numpy(full).cuda())


def test_serve_sends_the_frames_a_direct_render_gives(torch, SV):
    import surfel_trainer as TR
    from surfel_render import render
    dev = torch.device("cuda:0")
    model = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    bg, pipe = torch.zeros(3, device=dev), TR.pipeline_params()
    W, H = 65, 49
    a, b = _pair()
    viewer = SV.Viewer.attached(a)
    assert viewer.listener is None and _recv_json(b) == SV.RENDER_ITEMS
    frames = {}
    for mode in range(6):
        for sm in (1.0, 0.5):
            msg = VS.message(W, H, mode, seed=3, train=1, keep_alive=1, scaling_modifier=sm)
            b.sendall(VS.frame_message(msg))
            viewer.serve(model, pipe, bg, "/capture/path", lambda: {"#": model.P, "loss": 0.25}, 1, 10)      # one frame: train = 1 lets go
            assert viewer.conn is not None
            image, verify, metrics = _recv_frame(b, W, H)
            assert verify == "/capture/path" and metrics == {"#": 800, "loss": 0.25}
            with torch.no_grad():
                want = SV.net_image(render(_minicam(torch, SV, msg), model, pipe, bg, sm), mode)
            assert np.array_equal(image, want.cpu().numpy()), (mode, sm)
            frames[mode, sm] = image
        assert (frames[mode, 1.0] != frames[mode, 0.5]).any(), mode
    assert viewer.frames == 12 and frames[0, 1.0].any() and len(np.unique(frames[3, 1.0].reshape(-1, 3), axis=0)) > 20
    pinned = viewer._pinned
    assert pinned.is_pinned() and pinned.numel() == W * H * 3      # one buffer for all twelve frames
    # an empty request gets verify and metrics only; a mode off the list drops the viewer
    b.sendall(VS.frame_message(VS.message(0, 0, 0, train=1, keep_alive=0)) + VS.frame_message(VS.message(W, H, 0, seed=3, train=1)))
    viewer.serve(model, pipe, bg, "", None, 1, 10)
    assert int.from_bytes(_recv_exactly(b, 4), "little") == 0 and _recv_json(b) == {}
    assert _recv_frame(b, W, H)[0].shape == (H, W, 3)
    b.sendall(VS.frame_message(VS.message(W, H, 6, seed=3, train=1)))
    viewer.serve(model, pipe, bg, "", None, 1, 10)
    assert viewer.conn is None
    b.close()


def test_a_watched_training_ends_in_the_same_parameters(torch, SV):
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    W, H, steps = 40, 30, 4

    def run(viewer):
        model = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
        cams = TR.capture_views(model, TR.orbit_cameras(3, 64, 48, device=dev), torch.zeros(3, device=dev))
        model.spatial_lr_scale = 1.0
        opt = TR.optimization_params(dist_from_iter=0, normal_from_iter=0, lambda_dist=10.0)
        tr = TR.training(model, cams, opt, TR.pipeline_params(depth_ratio=1.0), iterations=steps, viewer=viewer)
        torch.cuda.synchronize()
        assert tr.iteration == steps
        return [t.clone() for t in model.capture()[1:7]]
    alone = run(None)
    a, b = _pair()
    viewer = SV.Viewer.attached(a)
    assert _recv_json(b) == SV.RENDER_ITEMS
    for k in range(steps):      # the viewer's requests wait in the socket: one per step, train = 1 (the last without keep_alive)
        b.sendall(VS.frame_message(VS.message(W, H, (1, 4, 0, 5)[k], seed=k, train=1, keep_alive=int(k < steps - 1), scaling_modifier=(1.0, 0.5)[k % 2])))
    watched = run(viewer)
    assert viewer.frames == steps and viewer.conn is not None
    for k in range(steps):
        image, _, metrics = _recv_frame(b, W, H)
        assert metrics["#"] == 800 and np.isfinite(metrics["loss"]) and image.any()
    for x, y in zip(alone, watched):
        assert x.dtype == y.dtype and torch.equal(x, y)
    viewer.close(); b.close()
