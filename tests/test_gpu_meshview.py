"""GPU checks of the mesh viewer (include/surfel_meshview.h, MESHVIEW.md): the depth half of the visibility buffer against mesh_depth
bit for bit, the triangle ids against the float64 oracle on every decided pixel, run-to-run and class-to-class identity of the whole key,
the inputs a rasteriser must skip, the shaded frames byte for byte against the float32 restatement applied to the device's own keys
(tests/meshview_oracle.py), a plane with affine colours in closed form, canaries around every output buffer, and the three ways to look
at a mesh end to end: frame files, videos, the remote viewer."""
import json
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cull_oracle as O  # noqa: E402
import cull_scenes as S  # noqa: E402
import meshview_oracle as M  # noqa: E402
import view_scenes as VS  # noqa: E402
from device_mesh import dev as _dev, mesh as _mesh, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZN, ZF = S.SCENE["znear"], S.SCENE["zfar"]
SHADE_VIEWS = (0, 11, 23, 24)      # an ordinary view at either end of the arc's first half, the filler's view, the view that sees nothing


def _keys(ref, ssaa=1, views=None, **kw):
    import surfel_meshview as P
    w2c = ref["w2c"] if views is None else ref["w2c"][list(views)]
    k = M.scaled_intrinsics(ref["intr"], ssaa)[0]
    return P.visibility(_mesh(ref["verts"], ref["tris"]), w2c, k, ref["H"] * ssaa, ref["W"] * ssaa, ZN, ZF, **kw)


# ------------------------------------------------------------------------------------------------ 1: the depth half
@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_depth_half_is_mesh_depth_bit_for_bit(size):
    import surfel_cull as C
    import surfel_meshview as P
    ref = O.scene_reference(size)
    want = C.mesh_depth(_mesh(ref["verts"], ref["tris"]), ref["w2c"], ref["intr"], ref["H"], ref["W"], ZN, ZF)
    for small in (-1, 0, 1 << 30):
        key = _keys(ref, small_pixels=small)
        assert key.dtype == torch.int64 and tuple(key.shape) == tuple(want.shape)
        depth, tri = P.unpack(key)
        assert torch.equal(depth.view(torch.int32), want.view(torch.int32)), small
        assert torch.equal(tri >= 0, want > 0) and int(tri.max()) < len(ref["tris"])
        assert bool((key[tri < 0] == P.EMPTY_KEY).all())
        d, t = M.unpack(key.cpu().numpy())
        assert np.array_equal(d, depth.cpu().numpy()) and np.array_equal(t, tri.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 2: the triangle ids
@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_triangle_ids_are_the_oracles_nearest(size):
    import surfel_meshview as P
    r = M.scene_reference(size)
    _, tri = P.unpack(_keys(r))
    got = tri.cpu().numpy()
    ok = ~r["und"]
    share = r["und"].mean((1, 2))
    print("%s: undecided pixels per image: %s %%" % (size, " ".join("%.3f" % (100 * s) for s in share)))
    print("%s: ids differ on %d decided and %d undecided pixels" % (size, ((got != r["tri64"]) & ok).sum(), ((got != r["tri64"]) & ~ok).sum()))
    assert share.max() <= M.CAP
    assert np.array_equal((got >= 0)[ok], (r["tri64"] >= 0)[ok])
    assert np.array_equal(got[ok], r["tri64"][ok]), np.argwhere((got != r["tri64"]) & ok)[:5]


# ------------------------------------------------------------------------------------------------ 3: the same bits
def test_same_key_bits_on_two_runs_and_through_either_class():
    ref = O.scene_reference(S.FIXTURE_SIZE)
    stats = {}
    first = _keys(ref, timings=stats)
    assert stats["large_pairs"] > 100
    torch.empty(1 << 22, dtype=torch.uint8, device=_dev()).fill_(0x5A)      # (a different history of the allocator's memory)
    assert torch.equal(_keys(ref), first)
    all_large, all_small = {}, {}
    assert torch.equal(_keys(ref, small_pixels=0, timings=all_large), first)
    assert torch.equal(_keys(ref, small_pixels=1 << 30, timings=all_small), first)
    assert all_small["large_pairs"] == 0 and all_large["large_pairs"] >= stats["large_pairs"] + 1000
    # among triangles that reach the same depth bits the lowest index wins: the same triangle three times
    import surfel_meshview as P
    v, t, _, _ = S.quad_anchor()
    k = S.intrinsics("small")
    H, W = S.SIZES["small"][:2]
    eye = np.eye(4, dtype=np.float32)[None]
    one = P.unpack(P.visibility(_mesh(v, t[:1]), eye, k, H, W, ZN, ZF))
    for small in (-1, 0, 1 << 30):
        two = P.unpack(P.visibility(_mesh(v, np.concatenate([t[:1], t[:1], t[:1]])), eye, k, H, W, ZN, ZF, small_pixels=small))
        assert torch.equal(two[0], one[0]) and torch.equal(two[1], one[1]) and int(one[1].max()) == 0 and int((one[1] == 0).sum()) > 100


# ------------------------------------------------------------------------------------------------ 4: skipped inputs
def test_skipped_inputs_change_nothing():
    """degenerate triangles, indices outside the vertices and a NaN vertex: depth and shaded frames are those of the scene without them
    (the special triangles come last, so the others keep their numbers; none of them is visible anywhere)"""
    import surfel_meshview as P
    a, b = O.scene_reference(S.FIXTURE_SIZE), O.scene_reference(S.FIXTURE_SIZE, special=False)
    ka, kb = _keys(a), _keys(b)
    assert torch.equal(ka, kb)
    assert int(P.unpack(ka)[1].max()) < len(b["tris"])      # no special triangle is visible
    ma, mb = _mesh(a["verts"], a["tris"], a["colors"]), _mesh(b["verts"], b["tris"], b["colors"])
    cams = (a["w2c"][[0, 23]], a["intr"], a["H"], a["W"])
    for smooth in (True, False):
        fa, fb = P.render_mesh(ma, cams, smooth=smooth), P.render_mesh(mb, cams, smooth=smooth)
        assert torch.equal(fa, fb) and fa.dtype == torch.uint8 and tuple(fa.shape) == (2, a["H"], a["W"], 3)
    assert torch.equal(P.render_mesh(ma, cams, mode="depth"), P.render_mesh(mb, cams, mode="depth"))
    # an empty mesh, and a mesh of skipped triangles only: nothing but background
    none = P.render_mesh(_mesh(a["verts"], np.zeros((0, 3), np.int32), a["colors"]), cams, background=(0.25, 0.5, 1.0))
    bad = P.render_mesh(_mesh(a["verts"], a["tris"][-5:], a["colors"]), cams, background=(0.25, 0.5, 1.0))
    want = torch.tensor([63, 127, 255], dtype=torch.uint8, device=_dev())
    assert bool((none == want).all()) and bool((bad == want).all())


# ------------------------------------------------------------------------------------------------ 5: shading, byte for byte
def test_vertex_normal_sums_equal_numpy():
    import surfel_meshview as P
    v, t, _ = S.mesh()
    normals, acc = P.vertex_normals(_mesh(v, t), return_sums=True)
    want = M.normal_sums(v, t)
    assert acc.dtype == torch.int64 and np.array_equal(acc.cpu().numpy(), want)
    assert np.array_equal(normals.cpu().numpy().view(np.uint32), M.normals_from_sums(want).view(np.uint32))
    again, acc2 = P.vertex_normals(_mesh(v, t), return_sums=True)
    assert torch.equal(acc2, acc) and torch.equal(again.view(torch.int32), normals.view(torch.int32))
    # valence 5 000: a component of the hub's sum passes 2^32
    import test_meshview_cpu as TC
    fv, ft = TC._fan()
    normals, acc = P.vertex_normals(_mesh(fv, ft), return_sums=True)
    want = M.normal_sums(fv, ft)
    assert np.array_equal(acc.cpu().numpy(), want) and int(acc[0, 2]) > 1 << 32
    assert np.array_equal(normals.cpu().numpy().view(np.uint32), M.normals_from_sums(want).view(np.uint32))


@pytest.mark.parametrize("size,ssaa", [(s, a) for s in sorted(S.SIZES) for a in (1, 2)])
def test_shading_is_the_restatement_byte_for_byte(size, ssaa):
    """every mode, flat and smooth, on the device's own key buffer: the restatement's bytes, all of them"""
    import surfel_meshview as P
    ref = O.scene_reference(size)
    H, W = ref["H"], ref["W"]
    mesh = _mesh(ref["verts"], ref["tris"], ref["colors"])
    w2c = ref["w2c"][list(SHADE_VIEWS)]
    ks = M.scaled_intrinsics(ref["intr"], ssaa)
    key = _keys(ref, ssaa, SHADE_VIEWS)
    host_keys = key.cpu().numpy().view(np.uint64)
    normals = P.vertex_normals(mesh)
    n_host = normals.cpu().numpy()
    assert (host_keys[-1] == M.EMPTY).all() and (host_keys[-2] != M.EMPTY).all() and 0.2 < (host_keys[0] != M.EMPTY).mean() < 0.8
    for mode in ("shaded", "normal", "color"):
        for smooth in (True, False):
            for albedo in (("color", "grey") if mode == "shaded" else ("color",)):
                bg = (1.0, 1.0, 1.0) if smooth else (0.1, 0.6, 0.35)
                got = P.shade(mesh, key, w2c, ks, H, W, ssaa, mode, normals if smooth else None, albedo, bg).cpu().numpy()
                want = M.shade_views(host_keys, ref["verts"], ref["tris"], ref["colors"] if albedo == "color" else None, n_host if smooth else None,
                                     w2c, ks, H, W, ssaa, mode, bg)
                diff = np.argwhere(got != want)
                assert not len(diff), (mode, smooth, albedo, len(diff), diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])
                if mode == "shaded" and smooth and albedo == "color":      # render_mesh is visibility + vertex normals + shade
                    full = P.render_mesh(mesh, (w2c, ref["intr"], H, W), ssaa=ssaa, budget_bytes=1, znear=ZN, zfar=ZF)      # (one view per batch)
                    assert np.array_equal(full.cpu().numpy(), want)
                    assert torch.equal(P.render_mesh(mesh, (w2c, ref["intr"], H, W), ssaa=ssaa, znear=ZN, zfar=ZF), full)


# ------------------------------------------------------------------------------------------------ 6: the anchor in closed form
def test_a_plane_with_affine_colours_in_closed_form():
    """A quad in the plane n . p = d under an identity camera, vertex colours an affine function of position: the colour frame is that
    function at p = (d / (n . ray)) ray, the normal frame the plane's normal turned to the camera — no barycentrics on this side."""
    import surfel_meshview as P
    v, t, n, d = S.quad_anchor()
    A = np.array([[0.07, 0.01, 0.02], [-0.02, 0.08, -0.03], [0.03, -0.04, 0.05]])
    b = np.array([0.44, 0.59, 0.35])
    colors = M.anchor_colors(v, A, b)      # (far outside [0, 1] at the quad's distant corners: the kernel clips nothing before it quantises)
    H, W = S.SIZES["large"][:2]
    k = S.intrinsics("large")
    eye = np.eye(4, dtype=np.float32)[None]
    color, normal = M.anchor_frames(n, d, A, b, k, H, W)
    assert color.min() > 0.05 and color.max() < 0.95      # inside the frame the function stays clear of the quantiser's clip
    # the vertex colours are float32 and the corners sit on the plane only up to their float32 rounding: both move a colour by less than
    # 1e-5, far below a level; a level more for the float32 interpolation and the truncating quantiser
    want_c, want_n = np.clip(color, 0, 1) * 255, np.clip(normal, 0, 1) * 255
    for smooth in (True, False):
        for ssaa in (1, 2):
            got_c = P.render_mesh(_mesh(v, t, colors), (eye, k, H, W), mode="color", smooth=smooth, ssaa=ssaa).cpu().numpy()[0].astype(np.float64)
            got_n = P.render_mesh(_mesh(v, t, colors), (eye, k, H, W), mode="normal", smooth=smooth, ssaa=ssaa).cpu().numpy()[0].astype(np.float64)
            # (ssaa 2: the four samples lie symmetrically about the pixel's ray and the colour moves by less than a level per pixel, so
            # their mean is the centre's value to second order)
            print("anchor (smooth %d, ssaa %d): colour off by at most %.3f levels, normal by %.3f" %
                  (smooth, ssaa, np.abs(got_c - np.floor(want_c)).max(), np.abs(got_n - np.floor(want_n)).max()))
            assert np.abs(got_c - np.floor(want_c)).max() <= 1 and np.abs(got_n - np.floor(want_n)).max() <= 1
    assert want_c.max() - want_c.min() > 60      # the colour varies over the frame


# ------------------------------------------------------------------------------------------------ 7: buffers respected
def test_canaries_around_every_output_buffer():
    """key, frames, normals and accumulators carved out of one allocation filled with a pattern, at the odd size (out-of-range indices,
    the NaN vertex and border boxes all run): the pattern on both sides of each is intact after the calls"""
    import surfel_native as N
    ref = O.scene_reference(S.FIXTURE_SIZE)
    v, t, H, W = ref["verts"], ref["tris"], ref["H"], ref["W"]
    dev = _dev()
    views, ssaa = [0, 23, 24], 2
    nv = len(views)
    w2c = _t(np.ascontiguousarray(ref["w2c"][views][:, :3, :].reshape(nv, 12), np.float32))
    ks = _t(M.scaled_intrinsics(ref["intr"], ssaa))
    pv, pt, pc = _t(v), _t(t), _t(ref["colors"])
    sizes = {"key": 8 * nv * H * W * ssaa * ssaa, "out": 3 * nv * H * W, "normals": 12 * len(v), "acc": 24 * len(v)}
    pad = 4096
    total = pad + sum(s + pad + 8 for s in sizes.values())
    big = torch.empty(total, dtype=torch.uint8, device=dev)
    pattern = (torch.arange(total, device=dev) * 37 + 11).to(torch.uint8)
    big.copy_(pattern)
    off, at = {}, pad
    for name, s in sizes.items():
        at = (at + 7) // 8 * 8
        off[name] = at
        at += s + pad
    view = lambda name, dtype: big[off[name]:off[name] + sizes[name]].view(dtype)
    key, out, normals, acc = view("key", torch.int64), view("out", torch.uint8), view("normals", torch.float32), view("acc", torch.int64)
    alloc = N.TorchAllocator(dev)
    N.call(dev, "surfel_meshview_visibility", alloc.cb, None, len(v), len(t), pv, pt, nv, w2c, ks, 1, H * ssaa, W * ssaa, ZN, ZF, -1, key, None)
    N.call(dev, "surfel_meshview_vertex_normals", len(v), len(t), pv, pt, acc, normals)
    N.call(dev, "surfel_meshview_shade", len(v), len(t), pv, pt, pc, normals, nv, w2c, ks, 1, H, W, ssaa, key, 0, 1.0, 1.0, 1.0, out)
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool, device=dev)
    for name, s in sizes.items():
        inside[off[name]:off[name] + s] = True
    assert torch.equal(big[~inside], pattern[~inside])
    assert int((~inside).sum()) >= 5 * pad
    # and what lies inside is the result
    got = out.view(nv, H, W, 3).cpu().numpy()
    want = M.shade_views(key.view(nv, H * ssaa, W * ssaa).cpu().numpy().view(np.uint64), v, t, ref["colors"], normals.view(-1, 3).cpu().numpy(),
                         ref["w2c"][views], ks.cpu().numpy(), H, W, ssaa, "shaded")
    assert np.array_equal(got, want) and np.array_equal(acc.view(-1, 3).cpu().numpy(), M.normal_sums(v, t))


# ------------------------------------------------------------------------------------------------ 8: end to end
def _scene_mesh():
    ref = O.scene_reference(S.FIXTURE_SIZE)
    return _mesh(ref["verts"], ref["tris"], ref["colors"])


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_render_mesh_path_writes_frames_and_videos(tmp_path):
    import surfel_meshview as P
    import surfel_trainer as TR
    mesh = _scene_mesh()
    cams = TR.orbit_cameras(8, 65, 49, radius=2.5, device=_dev())
    out = str(tmp_path / "traj")
    modes = ("shaded", "normal", "color", "depth")
    info = {}
    traj = P.render_mesh_path(mesh, cams, out, n_frames=6, modes=modes, video=True, timings=info)
    assert len(traj) == 6 and info["files"] == 24 and info["videos"] == sorted(modes)
    assert sorted(os.listdir(os.path.join(out, "mesh"))) == sorted("%s_%05d.png" % (m, k) for m in modes for k in range(6))
    assert sorted(f for f in os.listdir(out) if f.endswith(".avi")) == sorted("render_traj_mesh_%s.avi" % m for m in modes)
    for m in modes:
        want = P.render_mesh(mesh, traj, mode=m, depth_range=info["depth_limits"]).cpu().numpy()
        assert want.shape == (6, 48, 64, 3)
        for k in range(6):
            assert np.array_equal(_png(os.path.join(out, "mesh", "%s_%05d.png" % (m, k))), want[k]), (m, k)
        assert len(np.unique(want[0].reshape(-1, 3), axis=0)) > 20      # the path looks at the object
        with open(os.path.join(out, "render_traj_mesh_%s.avi" % m), "rb") as f:
            head = f.read(16)
        assert head[:4] == b"RIFF" and head[8:12] == b"AVI "
    only = str(tmp_path / "only")
    P.render_mesh_path(mesh, cams, only, n_frames=6, video_only=True, png="device")
    assert sorted(os.listdir(only)) == ["render_traj_mesh_normal.avi", "render_traj_mesh_shaded.avi"]
    # one frame per camera instead of the path; the device's PNG encoder gives the same pixels
    train = str(tmp_path / "train")
    P.render_mesh_path(mesh, cams[:3], train, modes=("shaded",), path=False, png="device")
    want = P.render_mesh(mesh, cams[:3])
    for k in range(3):
        assert np.array_equal(_png(os.path.join(train, "mesh", "shaded_%05d.png" % k)), want[k].cpu().numpy())


def test_cameras_of_two_sizes_are_grouped():
    """render_mesh_cameras: views of one size share their batches, and the frames come back in the cameras' order"""
    import surfel_meshview as P
    a, b = O.scene_reference("small"), O.scene_reference("large")
    mesh = _scene_mesh()
    cams = [P.PoseCamera(a["w2c"][0], a["intr"], a["H"], a["W"]), P.PoseCamera(a["w2c"][5], a["intr"], a["H"], a["W"]),
            P.PoseCamera(b["w2c"][3], b["intr"], b["H"], b["W"]), P.PoseCamera(a["w2c"][7], a["intr"], a["H"], a["W"])]
    frames = P.render_mesh_cameras(mesh, cams, znear=ZN, zfar=ZF)
    want_a = P.render_mesh(mesh, (a["w2c"][[0, 5, 7]], a["intr"], a["H"], a["W"]), znear=ZN, zfar=ZF)
    want_b = P.render_mesh(mesh, (b["w2c"][[3]], b["intr"], b["H"], b["W"]), znear=ZN, zfar=ZF)
    assert [tuple(f.shape) for f in frames] == [(45, 67, 3), (45, 67, 3), (64, 96, 3), (45, 67, 3)]
    assert torch.equal(frames[0], want_a[0]) and torch.equal(frames[1], want_a[1]) and torch.equal(frames[3], want_a[2]) and torch.equal(frames[2], want_b[0])
    with pytest.raises(ValueError, match="one size"):
        P.render_mesh(mesh, cams)
    assert torch.equal(P.render_mesh(mesh, cams[:2], znear=ZN, zfar=ZF), want_a[:2])


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


def _minicam(SV, msg):
    wvt = np.array(msg["view_matrix"], np.float32).reshape(4, 4) * np.array([1, -1, -1, 1], np.float32)
    full = np.array(msg["view_projection_matrix"], np.float32).reshape(4, 4) * np.array([1, -1, 1, 1], np.float32)
    return SV.MiniCam(msg["resolution_x"], msg["resolution_y"], msg["fov_y"], msg["fov_x"], msg["z_near"], msg["z_far"],
                      torch.from_numpy(wvt).cuda(), torch.from_numpy(full).cuda())


def test_the_viewer_serves_the_mesh_items():
    import surfel_meshview as P
    import surfel_trainer as TR
    import surfel_view as SV
    from surfel_render import render
    dev = _dev()
    model = TR.synthetic_object(800, dev, seed=0, px_scale=0.08)
    bg, pipe = torch.zeros(3, device=dev), TR.pipeline_params()
    mesh = _scene_mesh()
    W, H = 65, 49
    a, b = socket.socketpair()
    a.settimeout(10.0); b.settimeout(10.0)
    viewer = SV.Viewer.attached(a, mesh=mesh)
    assert _recv_json(b) == SV.RENDER_ITEMS + ["Mesh", "Mesh Normal"]
    for mode in range(8):
        msg = VS.message(W, H, mode, seed=3, train=1, keep_alive=1)
        b.sendall(VS.frame_message(msg))
        viewer.serve(model, pipe, bg, "/capture/path", None, 1, 10)
        assert viewer.conn is not None, mode
        image, verify, _ = _recv_frame(b, W, H)
        cam = _minicam(SV, msg)
        if mode < 6:      # the six old modes as before
            with torch.no_grad():
                want = SV.net_image(render(cam, model, pipe, bg, 1.0), mode)
        else:
            want = P.render_mesh(mesh, [cam], mode=("shaded", "normal")[mode - 6], ssaa=1)[0]
            assert len(np.unique(image.reshape(-1, 3), axis=0)) > 20 and (image == 255).all(-1).mean() > 0.2      # the object on white
        assert verify == "/capture/path" and np.array_equal(image, want.cpu().numpy()), mode
    b.sendall(VS.frame_message(VS.message(W, H, 8, seed=3, train=1)))      # a mode off the longer list drops the viewer
    viewer.serve(model, pipe, bg, "", None, 1, 10)
    assert viewer.conn is None
    b.close()
