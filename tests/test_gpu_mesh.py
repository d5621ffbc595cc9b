"""GPU checks of the TSDF mesh extraction (include/surfel_mesh.h, MESH.md) against the numpy oracle (tests/mesh_oracle.py) and
end to end through render()."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mesh_oracle as O  # noqa: E402

W, H, NV = 256, 192, 12
VS, TR, DT = 0.03, 0.12, 3.6      # voxel size, sdf_trunc, depth_trunc of the analytic scene


def _cam_block(eye, W, H, fov):
    import surfel_trainer as TR_
    R, T = TR_.look_at(eye)
    fx = W / (2 * math.tan(fov / 2))
    ext = np.concatenate([R.T, T[:, None]], 1)
    return np.concatenate([ext.reshape(-1), [fx, fx, (W - 1) / 2, (H - 1) / 2]]).astype(np.float32)


def _analytic_views(seed=0):
    """NV views of a sphere (radius 0.8 at the origin) on a plane y = 0.9, with zero depths, depths past depth_trunc and masks."""
    rng = np.random.default_rng(seed)
    views = []
    for i in range(NV):
        az, el = 2 * math.pi * (i + rng.uniform(0, 0.5)) / NV, math.radians(rng.uniform(-40, -5))
        eye = 3.0 * np.array([math.cos(el) * math.cos(az), math.sin(el), math.cos(el) * math.sin(az)])
        cam = _cam_block(eye, W, H, math.radians(55))
        R = cam[:12].reshape(3, 4)[:, :3].astype(np.float64)
        fx, fy, cx, cy = (float(x) for x in cam[12:])
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        dirc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)      # camera ray with z = 1: t = depth
        dw = dirc @ R                                                               # world direction (R^T d)
        o = eye
        b = dw @ o; a = (dw * dw).sum(-1); c = o @ o - 0.64
        disc = b * b - a * c
        ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
        tp = np.where(dw[..., 1] > 1e-9, (0.9 - o[1]) / np.where(dw[..., 1] > 1e-9, dw[..., 1], 1), np.inf)
        d = np.minimum(ts, tp)
        d = np.where(np.isfinite(d), d, 0.0).astype(np.float32)
        d[rng.random((H, W)) < 0.03] = 0.0                                          # holes
        rgb = rng.random((3, H, W)).astype(np.float32) * 1.2 - 0.1                  # outside [0, 1] too: clamped
        mask = np.ones((H, W), np.float32)
        y0, x0 = rng.integers(0, H - 40), rng.integers(0, W - 40)
        mask[y0:y0 + 30, x0:x0 + 30] = 0.2
        views.append((d, rgb, mask, cam))
    return views


def _prepared(views, dev):
    import surfel_mesh
    out = []
    for d, rgb, mask, cam in views:
        dd, rgba = surfel_mesh.prepare_view(torch.from_numpy(d).to(dev)[None], torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev), DT)
        out.append((dd, rgba, torch.from_numpy(cam).to(dev)))
    return out


@pytest.fixture(scope="module")
def fused():
    import surfel_mesh
    dev = torch.device("cuda:0")
    views = _analytic_views()
    prep = _prepared(views, dev)
    vol = surfel_mesh.fuse([p[0] for p in prep], [p[1] for p in prep], [p[2] for p in prep], VS, TR, DT, 8 << 30, dev)
    oviews = []
    for (d, rgb, mask, cam), (dd, rgba, _) in zip(views, prep):
        od = np.where((d > DT) | (mask < 0.5), 0.0, d).astype(np.float32)
        o8 = (np.clip(rgb, 0, 1) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
        assert np.array_equal(dd.cpu().numpy(), od)
        g = rgba.cpu().numpy().view(np.uint32)
        assert np.array_equal(np.stack([g & 255, (g >> 8) & 255, (g >> 16) & 255], -1).astype(np.uint8), o8)
        oviews.append((od, o8, cam))
    return vol, O.fuse(oviews, VS, TR)


def test_fusion_parity(fused):
    vol, ora = fused
    coords, trgb, wgt = vol.blocks()
    assert len(coords) > 100
    assert np.array_equal(coords, ora["coords"])
    t = trgb.cpu().numpy().reshape(-1, 4).astype(np.float64)
    w = wgt.cpu().numpy().reshape(-1)
    ex = ora["exempt"]
    print("exempt voxels: %d of %d" % (ex.sum(), ex.size))
    assert ex.mean() < 1e-3
    ok = ~ex
    assert np.array_equal(w[ok], ora["weight"][ok])
    m = ok & (w > 0)
    assert m.sum() > 10000
    assert np.max(np.abs(t[m, 0] - ora["tsdf"][m])) < 1e-5
    assert np.max(np.abs(t[m, 1:] - ora["rgb"][m])) < 1e-3


def test_extraction_parity(fused):
    vol, _ = fused
    mesh = vol.extract()
    coords, trgb, wgt = vol.blocks()
    t = trgb.cpu().numpy().reshape(-1, 4).astype(np.float64)
    verts, cols, tris = O.marching_cubes(coords, t[:, 0], wgt.cpu().numpy().reshape(-1).astype(np.float64), t[:, 1:], VS)
    assert len(tris) > 1000
    assert mesh.vertices.shape[0] == len(verts) and mesh.triangles.shape[0] == len(tris)
    assert np.array_equal(mesh.triangles.cpu().numpy(), tris)
    assert np.max(np.abs(mesh.vertices.cpu().numpy() - verts)) < 1e-5 * VS
    assert np.max(np.abs(mesh.vertex_colors.cpu().numpy() - cols)) < 1.0 / 255


def _sphere_model(dev):
    import surfel_model
    n = 6000
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), math.pi * (1 + 5 ** 0.5) * k
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    rng = np.random.default_rng(1)
    fl = np.array([0.0, -1.9, 0.3]) + 0.03 * rng.normal(size=(40, 3))      # a small detached floater
    fd = rng.normal(size=(40, 3)); fd /= np.linalg.norm(fd, axis=1, keepdims=True)
    xyz, nrm = np.concatenate([d, fl]), np.concatenate([d, fd])
    z = np.array([0.0, 0.0, 1.0])
    axis = np.cross(z, nrm); s = np.linalg.norm(axis, axis=1, keepdims=True); axis = axis / np.maximum(s, 1e-8)
    ang = np.arctan2(s[:, 0], nrm @ z)
    quat = np.concatenate([np.cos(ang / 2)[:, None], axis * np.sin(ang / 2)[:, None]], 1)
    P = len(xyz)
    scale = np.full((P, 2), math.log(0.045)); scale[n:] = math.log(0.03)
    m = surfel_model.GaussianModel(3, device=dev)
    m.set_parameters(xyz, np.full((P, 1, 3), 0.5), np.zeros((P, 15, 3)), np.full((P, 1), 6.0), scale, quat)
    return m


def _extract_sphere():
    import surfel_mesh
    import surfel_trainer as TR_
    from surfel_render import render
    dev = torch.device("cuda:0")
    model = _sphere_model(dev)
    # orbit cameras stay within 35 degrees of the equator: two more on the same orbit radius look at the poles
    cams = TR_.orbit_cameras(22, 256, 192, device=dev)
    for k, sgn in enumerate((1.0, -1.0)):
        eye = np.array([0.25, sgn, 0.1]); eye *= 4.0 / np.linalg.norm(eye)
        R, T = TR_.look_at(eye)
        cams.append(type(cams[0])(colmap_id=22 + k, R=R, T=T, FoVx=cams[0].FoVx, FoVy=cams[0].FoVy, image=torch.zeros(3, 192, 256),
                                  uid=22 + k, data_device=dev))
    ext = surfel_mesh.GaussianExtractor(model, render, TR_.pipeline_params())
    model.active_sh_degree = 0
    ext.reconstruction(cams)
    depth_trunc = 2.0 * ext.radius
    voxel = depth_trunc / 256
    mesh = ext.extract_mesh_bounded(voxel_size=voxel, sdf_trunc=5 * voxel, depth_trunc=depth_trunc)
    return ext, mesh, voxel


@pytest.fixture(scope="module")
def sphere_extraction():
    return _extract_sphere()


def test_end_to_end_sphere(sphere_extraction):
    import surfel_mesh
    ext, mesh, voxel = sphere_extraction
    assert abs(ext.radius - 4.0) < 1e-3
    post = surfel_mesh.post_process_mesh(mesh, 1).numpy()
    v, t = post.vertices.astype(np.float64), post.triangles.astype(np.int64)
    assert len(t) > 1000 and len(t) < mesh.triangles.shape[0]
    assert O.closed_oriented_manifold(t)
    assert O.euler(v, t) == 2
    r = np.linalg.norm(v, axis=1)
    assert np.mean(np.abs(r - 1.0) < 1.5 * voxel) >= 0.99
    assert v[:, 1].min() > -1.5                                  # the floater is gone
    assert np.all(np.bincount(t.reshape(-1), minlength=len(v)) > 0)
    n = O.face_normals(v, t)
    big = np.linalg.norm(n, axis=1) > 1e-12
    assert np.mean(np.einsum("ij,ij->i", n, v[t].mean(1))[big] > 0) > 0.99      # (fans over curved loops tilt a few slivers)
    volume = np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6
    assert abs(volume / (4 * math.pi / 3) - 1) < 0.05                         # outward as a whole


def test_determinism(sphere_extraction):
    ext, mesh, voxel = sphere_extraction
    again = ext.extract_mesh_bounded(voxel_size=voxel, sdf_trunc=5 * voxel, depth_trunc=2.0 * ext.radius)
    for a, b in ((mesh.vertices, again.vertices), (mesh.vertex_colors, again.vertex_colors), (mesh.triangles, again.triangles)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_budget_limit_and_empty_views():
    import surfel_mesh
    dev = torch.device("cuda:0")
    views = _analytic_views(seed=2)[:2]
    prep = _prepared(views, dev)
    args = ([p[0] for p in prep], [p[1] for p in prep], [p[2] for p in prep], VS, TR, DT)
    with pytest.raises(surfel_mesh.MeshLimitError) as e:
        surfel_mesh.fuse(*args, 1 << 20, dev)                # the table alone
    assert "budget" in str(e.value)
    vol = surfel_mesh.fuse(*args, 8 << 30, dev)
    need = int(vol.lib.surfel_tsdf_table_bytes(surfel_mesh.C.byref(vol.v))) + 10 * int(vol.lib.surfel_tsdf_block_bytes())
    assert vol.v.nblocks > 10
    with pytest.raises(surfel_mesh.MeshLimitError) as e:
        surfel_mesh.fuse(*args, need, dev)                   # the pool
    assert "voxel pool" in str(e.value)
    zero = [torch.zeros_like(p[0]) for p in prep]
    empty = surfel_mesh.fuse(zero, args[1], args[2], VS, TR, DT, 8 << 30, dev)
    assert empty.v.nblocks == 0
    mesh = empty.extract()
    assert mesh.vertices.shape == (0, 3) and mesh.triangles.shape == (0, 3)
    assert surfel_mesh.post_process_mesh(mesh, 1).triangles.shape[0] == 0
