"""GPU checks of the unbounded mesh extraction (include/surfel_mesh_unbounded.h, MESH.md §Unbounded) against the numpy oracle
(tests/mesh_unbounded_oracle.py), against an independent torch statement of the reference's fusion, and end to end through render()."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mesh_oracle as MO  # noqa: E402
import mesh_unbounded_oracle as U  # noqa: E402

SIZES = ((256, 192), (200, 152))      # two image sizes, alternating
NV = 12
RADIUS, M, R = 3.0, 97, 1.9          # normalisation radius (centre 0), lattice samples per axis, half-width
VS = 2 * RADIUS / 96                  # voxel size: sdf_trunc 0.3125 inside |s| = 1
BALL, BACK = 0.8, 12.0                # a sphere at the origin and a far backdrop (a sphere seen from inside, |s| = 1.75)


def _camera(i, eye, W, H, fovx, dev):
    import surfel_trainer as TR_
    from surfel_render import Camera
    Rm, T = TR_.look_at(eye)
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    return Camera(colmap_id=i, R=Rm, T=T, FoVx=fovx, FoVy=fovy, image=torch.zeros(3, H, W), image_name="v%02d" % i, uid=i, data_device=dev)


def _analytic_views(dev, seed=0):
    """NV views from radius 3 of the ball, every ray ending on it or on the backdrop: (full_proj_transform [4,4], z-depth [H,W],
    rgb [3,H,W])"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(NV):
        W, H = SIZES[i % 2]
        az, el = 2 * math.pi * (i + rng.uniform(0, 0.5)) / NV, math.radians(rng.uniform(-40, -5))
        eye = 3.0 * np.array([math.cos(el) * math.cos(az), math.sin(el), math.cos(el) * math.sin(az)])
        cam = _camera(i, eye, W, H, math.radians(55), dev)
        fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        dw = np.stack([(u - (W - 1) / 2) / fx, (v - (H - 1) / 2) / fy, np.ones_like(u)], -1) @ np.asarray(cam.R).T      # z = 1: t = depth
        a, b = (dw * dw).sum(-1), dw @ eye
        disc = b * b - a * (eye @ eye - BALL ** 2)
        ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
        tb = (-b + np.sqrt(b * b - a * (eye @ eye - BACK ** 2))) / a
        depth = np.minimum(ts, tb).astype(np.float32)
        rgb = (0.5 + 0.4 * np.sin(np.stack([u / 9.0, v / 7.0, (u + v) / 13.0]) + i)).astype(np.float32)
        out.append((cam.full_proj_transform.cpu().numpy(), depth, rgb))
    return out


def _pack(views, dev):
    import surfel_mesh
    return surfel_mesh.pack_views([P for P, _, _ in views], [torch.from_numpy(d).to(dev) for _, d, _ in views],
                                  [torch.from_numpy(c).to(dev) for _, _, c in views])


@pytest.fixture(scope="module")
def fused():
    import surfel_mesh
    dev = torch.device("cuda:0")
    views = _analytic_views(dev)
    packed = _pack(views, dev)
    lat = surfel_mesh.UnboundedLattice(M, R, [0.0, 0.0, 0.0], RADIUS, VS, 8 << 30, dev)
    count = torch.zeros(M ** 3, dtype=torch.int16, device=dev)
    lat.fuse(packed[0], packed[1], count)
    tsdf = lat.tsdf().cpu().numpy().astype(np.float64)
    n = count.cpu().numpy().view(np.uint16).reshape(M, M, M).astype(np.int64)
    return views, lat, tsdf, n, U.fuse(views, M, R, [0.0, 0.0, 0.0], RADIUS, VS)


def test_fusion_parity(fused):
    views, lat, tsdf, n, ora = fused
    ex = ora["exempt"]
    print("exempt samples: %d of %d (%.2e)" % (ex.sum(), ex.size, ex.mean()))
    assert ex.mean() < 1e-3
    ok = ~ex
    assert np.array_equal(n[ok], ora["count"][ok])
    # the scene reaches both sides of |s| = 1, and both signs
    mag = np.linalg.norm(U.lattice_contracted(M, R), axis=1).reshape(M, M, M)
    for part in (mag < 1, (mag > 1) & (mag < 1.9)):
        assert np.sum(part & (n > 0) & (tsdf > 0)) > 1000 and np.sum(part & (n > 0) & (tsdf < 0)) > 100
    assert np.all(tsdf[n == 0] == -1.0)
    d = np.abs(tsdf - ora["tsdf"])
    bad = ok & (ora["bound"] > 1e-5)
    print("samples with an error bound > 1e-5 (depth edges, far depths): %d; max |diff| %.3g there, %.3g elsewhere; %d differ by 1e-5 or more"
          % (bad.sum(), d[bad].max(initial=0), d[ok & ~bad].max(), np.sum(d[ok] >= 1e-5)))
    assert np.all(d[ok & ~bad] < 1e-5)
    assert np.all(d[bad] < 1e-5 + ora["bound"][bad])
    assert np.mean(d[ok] < 1e-5) >= 0.998


def _torch_fusion(views, dev):
    """The reference's compute_unbounded_tsdf (utils/mesh_utils.py:215-250) restated in torch fp32 with grid_sample, sum form."""
    F = torch.nn.functional
    j = torch.arange(M, dtype=torch.float32, device=dev)
    step = torch.tensor(2.0, device=dev) * torch.tensor(R, device=dev) / (M - 1)
    zz, yy, xx = torch.meshgrid(j, j, j, indexing="ij")
    s = torch.stack([xx, yy, zz], -1).reshape(-1, 3) * step - torch.tensor(R, device=dev)
    mag = torch.linalg.norm(s, dim=-1)
    trunc = 5 * torch.tensor(VS, device=dev) * torch.ones_like(mag)
    trunc[mag > 1] *= 1 / (2 - mag[mag > 1].clamp(max=1.9))
    p = torch.where(mag[:, None] < 1, s, 1 / (2 - mag[:, None]) * (s / mag[:, None])) * RADIUS
    total = -torch.ones_like(mag)
    n = torch.zeros_like(mag)
    for P, depth, _ in views:
        q = torch.cat([p, torch.ones_like(p[:, :1])], -1) @ torch.from_numpy(P).to(dev)
        w = q[:, 3:]
        pix = q[:, :2] / w
        vis = ((pix > -1) & (pix < 1) & (w > 0)).all(-1)
        dm = torch.from_numpy(depth).to(dev)[None, None]
        sd = F.grid_sample(dm, pix[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(-1) - w[:, 0]
        m = vis & (sd > -trunc)
        total[m] += torch.clamp(sd / trunc, -1, 1)[m]
        n[m] += 1
    return (total / (1 + n)).reshape(M, M, M).cpu().numpy()


def test_torch_cross_check(fused):
    """A wrong pixel convention or a flipped axis would move most observed samples; what differs here is the samples read across
    the ball's silhouette (a depth step of about 13 per pixel), where the two fp32 evaluations differ in the last bits of the pixel
    position."""
    views, lat, tsdf, n, ora = fused
    ref = _torch_fusion(views, torch.device("cuda:0"))
    agree = np.abs(tsdf - ref) < 1e-5
    calm = ~ora["exempt"] & (ora["bound"] <= 1e-5)
    print("torch statement: %d of %d samples differ by 1e-5 or more, %d of the %d well-conditioned ones"
          % ((~agree).sum(), agree.size, (~agree[calm]).sum(), calm.sum()))
    assert agree[calm].mean() >= 0.9999
    assert agree.mean() >= 0.998


def test_extraction_parity(fused):
    import surfel_mesh
    views, lat, tsdf, n, _ = fused
    verts, tris = lat.extract()
    ov, ot = U.marching_cubes(lat.tsdf().cpu().numpy(), R, [0.0, 0.0, 0.0], RADIUS)
    assert len(ot) > 5000
    assert lat.v.nslabs == 1
    assert verts.shape[0] == len(ov) and tris.shape[0] == len(ot)
    assert np.array_equal(tris.cpu().numpy(), ot)
    v = verts.cpu().numpy()
    assert np.all(np.abs(v - ov) <= 1e-5 * np.maximum(1.0, np.abs(ov)))
    # the same lattice in slabs of 30 cube planes: 4 slabs, the same bytes
    dev = torch.device("cuda:0")
    lat2 = surfel_mesh.UnboundedLattice(M, R, [0.0, 0.0, 0.0], RADIUS, VS, 8 << 30, dev, slab=30)
    lat2.tsdf().copy_(lat.tsdf())
    v2, t2 = lat2.extract()
    assert lat2.v.nslabs >= 3
    assert v2.cpu().numpy().tobytes() == v.tobytes() and t2.cpu().numpy().tobytes() == tris.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ end to end through render()
# The backdrop: a disk of radius 3.6 in the ceiling y = -9 (world -y is up), |s| about 1.6 in the contracted shell.  It lies outside
# every frustum of the cameras that look at the ball, so no sightline past the ball's silhouette reaches it: the bilinear depth
# sample would read across such a depth step, and the reference's fusion then pushes +1 into the ball's surface samples.  Twelve
# cameras above the ball look up at it: with the initial weight of 1 at tsdf -1, the zero crossing of a surface that n views see
# head-on sits about sdf_trunc / n in front of it, within the adaptive voxel size (sdf_trunc / 5) only for n > 5.
CEIL, DISK = -9.0, 3.6


def _scene_model(dev):
    import surfel_model
    n = 6000
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), math.pi * (1 + 5 ** 0.5) * k
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    g = np.arange(-DISK, DISK + 0.01, 0.15)
    gx, gz = np.meshgrid(g, g)
    fl = np.stack([gx.reshape(-1), np.full(gx.size, CEIL), gz.reshape(-1)], 1)
    fl = fl[np.hypot(fl[:, 0], fl[:, 2]) <= DISK]
    xyz = np.concatenate([d, fl])
    nrm = np.concatenate([d, np.tile([0.0, -1.0, 0.0], (len(fl), 1))])
    z = np.array([0.0, 0.0, 1.0])
    axis = np.cross(z, nrm); s = np.linalg.norm(axis, axis=1, keepdims=True); axis = axis / np.maximum(s, 1e-8)
    ang = np.arctan2(s[:, 0], nrm @ z)
    quat = np.concatenate([np.cos(ang / 2)[:, None], axis * np.sin(ang / 2)[:, None]], 1)
    P = len(xyz)
    scale = np.full((P, 2), math.log(0.045)); scale[n:] = math.log(0.15)
    dc = np.full((P, 1, 3), 0.5); dc[n:, 0] = [-0.6, 0.2, 0.8]
    m = surfel_model.GaussianModel(3, device=dev)
    m.set_parameters(xyz, dc, np.zeros((P, 15, 3)), np.full((P, 1), 6.0), scale, quat)
    return m


def _cameras(dev):
    import surfel_trainer as TR_
    from surfel_render import Camera
    fov = math.radians(50)
    cams = []
    for i in range(24):      # three rings around the ball: elevations -35, 0, 35 degrees, 8 views each
        az, el = 2 * math.pi * (i + 0.5 * (i // 8)) / 8, math.radians(35.0 * (i // 8 - 1))
        cams.append(_camera(i, 4.0 * np.array([math.cos(el) * math.cos(az), -math.sin(el), math.cos(el) * math.sin(az)]), 256, 192, fov, dev))
    eye = np.array([0.25, -1.0, 0.1]); eye *= 4.0 / np.linalg.norm(eye)      # the upper pole (a lower one would see the disk)
    cams.append(_camera(24, eye, 256, 192, fov, dev))
    for k in range(12):
        a = math.pi / 12 + k * math.pi / 6
        Rm, T = TR_.look_at(np.array([3 * math.cos(a), -2.0, 3 * math.sin(a)]), target=(0.0, CEIL, 0.0))
        cams.append(Camera(colmap_id=25 + k, R=Rm, T=T, FoVx=fov, FoVy=2 * math.atan(math.tan(fov / 2) * 0.75), image=torch.zeros(3, 192, 256),
                           image_name="v%02d" % (25 + k), uid=25 + k, data_device=dev))
    return cams


@pytest.fixture(scope="module")
def scene():
    import surfel_mesh
    import surfel_trainer as TR_
    from surfel_render import render
    dev = torch.device("cuda:0")
    model = _scene_model(dev)
    cams = _cameras(dev)
    ext = surfel_mesh.GaussianExtractor(model, render, TR_.pipeline_params())
    model.active_sh_degree = 0
    ext.timings = {}
    ext.reconstruction(cams)
    mesh = ext.extract_mesh_unbounded(512)
    return ext, model, cams, mesh


def _component(mesh, label, root):
    t = mesh.triangles.cpu().numpy().astype(np.int64)[label == root]
    used, inv = np.unique(t.reshape(-1), return_inverse=True)
    return mesh.vertices.cpu().numpy().astype(np.float64)[used], inv.reshape(-1, 3)


def test_end_to_end_sphere_and_backdrop(scene):
    import surfel_mesh
    ext, model, cams, mesh = scene
    assert ext.radius > 2.0
    assert set(ext.timings) >= {"render", "fuse", "extract", "color"}
    post = surfel_mesh.post_process_mesh(mesh, 50)
    label, _ = surfel_mesh.cluster_triangles(post)
    label = label.cpu().numpy()
    pv = post.vertices.cpu().numpy().astype(np.float64)
    pt = post.triangles.cpu().numpy().astype(np.int64)
    nearest = int(np.argmin(np.linalg.norm(pv, axis=1)))
    root = label[np.nonzero((pt == nearest).any(1))[0][0]]
    v, t = _component(post, label, root)
    voxel = 2 * ext.radius / 512
    assert len(t) > 1000
    assert MO.closed_oriented_manifold(t)
    assert MO.euler(v, t) == 2
    r = np.linalg.norm(v, axis=1)
    print("sphere: %d vertices, %.4f within 1.5 voxels of radius 1" % (len(v), np.mean(np.abs(r - 1) < 1.5 * voxel)))
    assert np.mean(np.abs(r - 1.0) < 1.5 * voxel) >= 0.99
    n = MO.face_normals(v, t)
    big = np.linalg.norm(n, axis=1) > 1e-12
    assert np.mean(np.einsum("ij,ij->i", n, v[t].mean(1))[big] > 0) > 0.99      # outward: toward the observed free space
    # the disk: vertices of its middle lie within the adaptive voxel size of it
    hr = np.linalg.norm(pv[:, [0, 2]], axis=1)
    fv = pv[(np.abs(pv[:, 1] - CEIL) < 1.0) & (hr < DISK - 1.0)]
    s = np.linalg.norm(U.contract((fv - ext.center.cpu().numpy()) / ext.radius), axis=1)
    assert len(fv) > 200 and s.min() > 1.0
    tol = voxel / (2 - np.minimum(s, 1.9))
    frac = np.mean(np.abs(fv[:, 1] - CEIL) <= tol)
    print("disk: %d vertices, %.4f within the adaptive voxel size of y = %g (median offset %.4g, median tolerance %.4g)"
          % (len(fv), frac, CEIL, np.median(fv[:, 1] - CEIL), np.median(tol)))
    assert frac >= 0.99


def test_vertex_colors_follow_the_oracle(scene):
    ext, model, cams, mesh = scene
    views = [(c.full_proj_transform.cpu().numpy(), d.cpu().numpy()[0], c_.cpu().numpy())
             for c, d, c_ in zip(ext.viewpoint_stack, ext.depthmaps, ext.rgbmaps)]
    v = mesh.vertices.cpu().numpy()
    ref = U.vertex_colors(v, views, 2 * ext.radius / 512)
    d = np.abs(mesh.vertex_colors.cpu().numpy() - ref).max(1)
    print("colours: %d vertices, %d differ by 1e-4 or more (max %.3g)" % (len(v), (d >= 1e-4).sum(), d.max()))
    assert np.mean(d < 1e-4) >= 0.999
    assert mesh.vertex_colors.min() >= 0 and mesh.vertex_colors.max() < 1      # sum / (1 + n) of colours in [0, 1) darkens them


def test_determinism(scene):
    ext, model, cams, mesh = scene
    again = ext.extract_mesh_unbounded(512)
    for a, b in ((mesh.vertices, again.vertices), (mesh.vertex_colors, again.vertex_colors), (mesh.triangles, again.triangles)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_limits(scene):
    import surfel_mesh
    ext, model, cams, mesh = scene
    with pytest.raises(ValueError):
        ext.extract_mesh_unbounded(768)
    budget = ext.budget_bytes
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ext.budget_bytes = 4 * 512 ** 3      # the lattice alone, without its slab scratch
    try:
        with pytest.raises(surfel_mesh.MeshLimitError) as e:
            ext.extract_mesh_unbounded(512)
    finally:
        ext.budget_bytes = budget
    assert "budget" in str(e.value)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


def test_cli_unbounded(tmp_path, scene):
    import sys
    import surfel_io
    import surfel_mesh
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import mesh_bench
    ext, model, cams, mesh = scene
    mesh_bench.write_model_dir(model, cams, str(tmp_path), 7)
    assert surfel_mesh.main(["-m", str(tmp_path), "--unbounded", "--mesh_res", "512"]) == 0
    out = tmp_path / "train" / "ours_7"
    v, t, c = surfel_io.read_triangle_mesh(str(out / "fuse_unbounded.ply"))
    vp, tp, cp = surfel_io.read_triangle_mesh(str(out / "fuse_unbounded_post.ply"))
    assert len(t) > 1000 and 0 < len(tp) <= len(t)
    assert v.shape[1] == 3 and np.all(np.abs(v) <= 32)
