"""TSDF mesh extraction on MI355X — the reference's `GaussianExtractor` (bounded and unbounded paths) and `post_process_mesh`
(utils/mesh_utils.py:22-280) and the mesh step of render.py:86-106, without Open3D, scikit-image or trimesh.

The fusion, marching cubes and the connected-component filter are HIP kernels of libsurfel_hip.so (include/surfel_mesh.h); the
rules they follow are written down in MESH.md.  Maps stay on the device; only counts cross to the host.  The unbounded path's
kernels sit behind include/surfel_mesh_unbounded.h.

    python 2d-gaussian-splatting_amd/surfel_mesh.py -m MODEL_DIR [--iteration N] [--mesh_res 1024] [--unbounded] ...
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch

import surfel_native as _n

_n.load()


MeshLimitError = _n.LimitError      # SURFEL_E_LIMIT: the volume would exceed the byte budget (raise the budget or the voxel size)


class TriangleMesh:
    """vertices [V,3] float32, triangles [F,3] int32, vertex_colors [V,3] float32 in 0..1 — Open3D's attribute names; torch
    tensors (on the device after extraction)."""

    def __init__(self, vertices, triangles, vertex_colors):
        self.vertices, self.triangles, self.vertex_colors = vertices, triangles, vertex_colors

    def numpy(self):
        return TriangleMesh(*(np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x) for x in (self.vertices, self.triangles, self.vertex_colors)))


def read_mesh(path, device):
    """the TriangleMesh of a .ply (surfel_io.read_triangle_mesh) on `device`"""
    import surfel_io
    return TriangleMesh(*(torch.from_numpy(a).to(device) for a in surfel_io.read_triangle_mesh(path)))


def mesh_arrays(who, mesh, colors=False, shapes=("[N, 3]", "[N, 3]")):
    """What a side module's kernels take of a mesh, checked in this order: (vertices fp32 [V, 3], triangles int32 [F, 3]), contiguous on
    the device; with colors also mesh.vertex_colors as fp32 [V, 3], or None where the mesh has none.  who: the calling module's name, the
    messages' prefix; shapes: how its messages write the two shapes."""
    verts = _n.rows(who, mesh.vertices, "mesh.vertices", torch.float32, shapes[0])
    tris = _n.rows(who, mesh.triangles, "mesh.triangles", torch.int32, shapes[1])
    if not colors:
        return verts, tris
    cols = getattr(mesh, "vertex_colors", None)
    if cols is not None:
        cols = _n.rows(who, cols, "mesh.vertex_colors", torch.float32)
        if cols.shape[0] != verts.shape[0]:
            raise ValueError("%s: %d colours for %d vertices" % (who, cols.shape[0], verts.shape[0]))
    return verts, tris, cols


def shown_colors(who, mesh, V):
    """mesh.vertex_colors as the modules that draw a mesh take them: fp32 [V, 3] on the device, None where the mesh has none or empty ones"""
    c = getattr(mesh, "vertex_colors", None)
    if c is None or c.numel() == 0:
        return None
    c = _n.device_tensor(who, c, "mesh.vertex_colors")
    if tuple(c.shape) != (V, 3):
        raise ValueError("%s: mesh.vertex_colors must be [V, 3], got %s" % (who, list(c.shape)))
    return c.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------ cameras
def camera_intrinsics(cam):
    """(fx, fy, cx, cy) as utils/mesh_utils.py:43-68: (projection_matrix @ ndc2pix)[:3,:3].T with cx = (W-1)/2, cy = (H-1)/2."""
    W, H = int(cam.image_width), int(cam.image_height)
    ndc2pix = np.array([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]], np.float64).T
    intr = (np.asarray(cam.projection_matrix.detach().cpu().numpy(), np.float64) @ ndc2pix)[:3, :3].T
    return float(intr[0, 0]), float(intr[1, 1]), float(intr[0, 2]), float(intr[1, 2])


def camera_block(cam):
    """The 16-float camera of include/surfel_mesh.h: extrinsic = world_view_transform.T (rows 0..2), then fx, fy, cx, cy."""
    ext = np.asarray(cam.world_view_transform.detach().cpu().numpy(), np.float64).T
    out = np.zeros(16, np.float32)
    out[:12] = ext[:3, :4].reshape(-1)
    out[12:] = camera_intrinsics(cam)
    return out


def bounding_sphere(c2ws):
    """(center, radius) from camera-to-world matrices [N,4,4]: the point nearest (least squares) to every optical axis — the line
    through the camera centre along its viewing direction, the camera's +z (the reference's poses flip y and z and look along -z,
    the same line) — and its smallest distance to a camera centre."""
    c2ws = np.asarray(c2ws, np.float64)
    o, d = c2ws[:, :3, 3], c2ws[:, :3, 2]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]       # projector onto the plane normal to each axis
    center = np.linalg.solve(P.sum(0), np.einsum("nij,nj->i", P, o))
    return center, float(np.linalg.norm(o - center, axis=1).min())


# ------------------------------------------------------------------------------------------------ the volume
class TsdfVolume:
    """Dense block table + voxel pool through the library (include/surfel_mesh.h).  `budget_bytes` bounds table + pool."""

    def __init__(self, voxel_size, sdf_trunc, origin, dims, budget_bytes, device):
        self.lib, self.device = _n.load(), torch.device(device)
        self.alloc = _n.TorchAllocator(self.device)
        self.v = _n.TsdfVolume()
        self.v.origin[:] = [int(x) for x in origin]
        self.v.dims[:] = [int(x) for x in dims]
        self.v.voxel_size, self.v.sdf_trunc, self.v.budget_bytes = float(voxel_size), float(sdf_trunc), int(budget_bytes)
        _n.call(self.device, "surfel_tsdf_init", self.v, self.alloc.cb, None)

    def mark(self, depth, cam):
        H, W = depth.shape[-2:]
        _n.call(self.device, "surfel_tsdf_mark", self.v, H, W, depth, cam)

    def allocate(self):
        return _n.call(self.device, "surfel_tsdf_allocate", self.v, self.alloc.cb, None)

    def integrate(self, depth, rgba, cam):
        H, W = depth.shape[-2:]
        _n.call(self.device, "surfel_tsdf_integrate", self.v, H, W, depth, rgba, cam)

    def extract(self):
        _n.call(self.device, "surfel_tsdf_count", self.v)
        V, F = int(self.v.nverts), int(self.v.ntris)
        verts = torch.empty((V, 3), dtype=torch.float32, device=self.device)
        cols = torch.empty((V, 3), dtype=torch.float32, device=self.device)
        tris = torch.empty((F, 3), dtype=torch.int32, device=self.device)
        _n.call(self.device, "surfel_tsdf_extract", self.v, verts, cols, tris)
        return TriangleMesh(verts, tris, cols)

    def _tensor(self, field, dtype, shape):
        """A view of one of the library's buffers (white-box access for tests and measurement)."""
        return self.alloc.view(getattr(self.v, field), dtype, shape)

    def blocks(self):
        """(block coordinates [nblocks,3] int64 in slot order = table order, tsdf_rgb [nblocks,4096,4], weight [nblocks,4096])"""
        nb = int(self.v.nblocks)
        if nb == 0:
            return np.zeros((0, 3), np.int64), torch.zeros((0, 4096, 4)), torch.zeros((0, 4096))
        keys = self._tensor("keys", torch.int32, (nb,)).cpu().numpy().astype(np.int64)
        nx, ny, _ = self.v.dims
        bc = np.stack([keys % nx, (keys // nx) % ny, keys // (nx * ny)], 1) + np.array(self.v.origin)
        return bc, self._tensor("tsdf_rgb", torch.float32, (nb, 4096, 4)), self._tensor("weight", torch.float32, (nb, 4096))


def volume_bounds(cams_blocks, depth_trunc, sdf_trunc, voxel_size):
    """Dense block table from the cameras alone: their centres' AABB grown by depth_trunc * (largest ray stretch) + sdf_trunc, in
    blocks of 16 voxels.  cams_blocks: [N,16] camera blocks with the image sizes appended ([N,18])."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for c in cams_blocks:
        ext = np.eye(4)
        ext[:3, :4] = np.asarray(c[:12], np.float64).reshape(3, 4)
        centre = np.linalg.inv(ext)[:3, 3]
        fx, fy, cx, cy, W, H = (float(x) for x in c[12:18])
        stretch = math.sqrt(1.0 + (max(cx, W - 1 - cx) / fx) ** 2 + (max(cy, H - 1 - cy) / fy) ** 2)
        g = depth_trunc * stretch + sdf_trunc
        lo, hi = np.minimum(lo, centre - g), np.maximum(hi, centre + g)
    bs = 16.0 * voxel_size
    b0 = np.floor(lo / bs).astype(np.int64) - 1
    b1 = np.floor(hi / bs).astype(np.int64) + 1
    return b0, b1 - b0 + 1


def fuse(depths, rgbas, cams, voxel_size, sdf_trunc, depth_trunc, budget_bytes, device, timings=None, touched=None):
    """TSDF fusion of prepared views (depth [H,W] with 0 = invalid, rgba [H,W] uint32, camera block [16]) into a TsdfVolume.
    touched: a list that receives every view's touched-block count (synchronises after each view; measurement only)."""
    dev = torch.device(device)
    blocks = [np.concatenate([c.cpu().numpy(), [d.shape[-1], d.shape[-2]]]) for c, d in zip(cams, depths)]
    origin, dims = volume_bounds(blocks, depth_trunc, sdf_trunc, voxel_size)
    if np.any(dims > 2 ** 20) or int(np.prod(dims)) * 8 > budget_bytes:
        raise MeshLimitError("mesh volume: the dense block table (%s blocks) exceeds the byte budget (%d)" % (list(dims), budget_bytes))
    t = _Timer(timings, dev)
    vol = TsdfVolume(voxel_size, sdf_trunc, origin, dims, budget_bytes, dev)
    for d, c in zip(depths, cams):
        vol.mark(d, c)
    vol.allocate()
    t.lap("touch")
    for d, rgba, c in zip(depths, rgbas, cams):
        vol.integrate(d, rgba, c)
        if touched is not None:
            touched.append(int(vol._tensor("list", torch.int32, (1,))[0]) if vol.v.nblocks else 0)
    t.lap("integrate")
    return vol


class _Timer:
    def __init__(self, out, dev):
        self.out, self.dev = out, dev
        if out is not None:
            torch.cuda.synchronize(dev)
            self.t = time.perf_counter()

    def lap(self, name):
        if self.out is None:
            return
        torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.out[name] = self.out.get(name, 0.0) + (now - self.t) * 1e3
        self.t = now


def prepare_view(surf_depth, rgb, mask, depth_trunc):
    """(depth [H,W] float32, rgba [H,W] int32) of one view (surfel_mesh_prepare_view)."""
    d = surf_depth.detach().contiguous().float()
    H, W = d.shape[-2:]
    rgb = rgb.detach().contiguous().float()
    m = None if mask is None else mask.detach().contiguous().float().to(d.device)
    dout = torch.empty((H, W), dtype=torch.float32, device=d.device)
    rgba = torch.empty((H, W), dtype=torch.int32, device=d.device)
    _n.call(d.device, "surfel_mesh_prepare_view", H, W, d, rgb, m, float(depth_trunc), dout, rgba)
    return dout, rgba


# ------------------------------------------------------------------------------------------------ unbounded (MESH.md §Unbounded)
def contract(x):
    """utils/mesh_utils.py:189-191: x where |x| < 1, else (2 - 1/|x|) x/|x| (last axis)."""
    mag = torch.linalg.norm(x, ord=2, dim=-1)[..., None]
    return torch.where(mag < 1, x, (2 - (1 / mag)) * (x / mag))


def uncontract(y):
    """utils/mesh_utils.py:193-195: y where |y| < 1, else y / (|y| (2 - |y|))."""
    mag = torch.linalg.norm(y, ord=2, dim=-1)[..., None]
    return torch.where(mag < 1, y, (1 / (2 - mag) * (y / mag)))


def lattice_size(resolution):
    """Distinct samples per axis of the reference's resolution/512 crops of 512 linspace samples: neighbouring crops share a plane."""
    return (int(resolution) // 512) * 511 + 1


def lattice_half_width(xyz, center, radius):
    """R = min(quantile_0.95 |contract((xyz - center) / radius)| + 0.01, 1.9) (mesh_utils.py:263-265; numpy's linear quantile)."""
    r = contract((xyz.detach().float() - center) / radius).norm(dim=-1).cpu().numpy()
    return min(float(np.quantile(r, q=0.95)) + 0.01, 1.9)


def pack_views(projs, depths, rgbs=None):
    """(views uint8 [64 n] on the device = surfel_unbounded_view[n], packed depth, packed rgb or None).  projs: full_proj_transform
    [4,4] per view (row-vector convention); depths [H,W] or [1,H,W]; rgbs [3,H,W]."""
    dev = depths[0].device
    arr = (_n.UnboundedView * len(depths))()
    off = 0
    for k, (P, d) in enumerate(zip(projs, depths)):
        P = np.asarray(P.detach().cpu().numpy() if torch.is_tensor(P) else P, np.float32)
        H, W = d.shape[-2:]
        arr[k].proj[:] = [float(x) for x in np.concatenate([P[:, 0], P[:, 1], P[:, 3]])]
        arr[k].H, arr[k].W, arr[k].offset = int(H), int(W), off
        off += int(H) * int(W)
    views = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    depth = torch.cat([d.detach().float().reshape(-1) for d in depths])
    rgb = None if rgbs is None else torch.cat([c.detach().float().reshape(-1) for c in rgbs])
    return views, depth, rgb


class UnboundedLattice:
    """The M^3 contracted lattice through the library (include/surfel_mesh_unbounded.h).  `budget_bytes` bounds the lattice, the
    slab scratch and the outputs; MeshLimitError is raised before anything is allocated for them."""

    def __init__(self, M, R, center, radius, voxel_size, budget_bytes, device, slab=0):
        self.lib, self.device = _n.load(), torch.device(device)
        self.alloc = _n.TorchAllocator(self.device)
        self.v = _n.UnboundedVolume()
        self.v.M, self.v.slab, self.v.R = int(M), int(slab), float(R)
        self.v.center[:] = [float(x) for x in np.asarray(center.detach().cpu().numpy() if torch.is_tensor(center) else center, np.float64)]
        self.v.radius, self.v.voxel_size, self.v.budget_bytes = float(radius), float(voxel_size), int(budget_bytes)
        _n.call(self.device, "surfel_unbounded_init", self.v, self.alloc.cb, None)

    def fuse(self, views, depth, count=None):
        """views / depth from pack_views; count: a uint16-sized tensor [M^3] (int16 storage) that receives every sample's view count."""
        n = views.numel() // 64
        _n.call(self.device, "surfel_unbounded_fuse", self.v, n, views, depth, count)

    def tsdf(self):
        """The lattice [M, M, M] indexed [z, y, x] (a view of the library's buffer)."""
        M = self.v.M
        return self.alloc.view(self.v.tsdf, torch.float32, (M, M, M))

    def extract(self):
        """(verts [V,3] world, clipped to +-32, tris [F,3] int32) in lattice / cube order."""
        _n.call(self.device, "surfel_unbounded_count", self.v)
        V, F = int(self.v.nverts), int(self.v.ntris)
        verts = torch.empty((V, 3), dtype=torch.float32, device=self.device)
        tris = torch.empty((F, 3), dtype=torch.int32, device=self.device)
        _n.call(self.device, "surfel_unbounded_extract", self.v, verts, tris)
        return verts, tris


def color_vertices(verts, views, depth, rgb, sdf_trunc):
    """colors [V,3] = sum of bilinear rgb / (1 + n) over the views that see a vertex within sdf_trunc (surfel_unbounded_color)."""
    V = int(verts.shape[0])
    cols = torch.empty((V, 3), dtype=torch.float32, device=verts.device)
    _n.call(verts.device, "surfel_unbounded_color", V, verts.contiguous(), views.numel() // 64, views, depth, rgb, float(sdf_trunc), cols)
    return cols


# ------------------------------------------------------------------------------------------------ the reference's interface
DEFAULT_BUDGET = 64 << 30


class GaussianExtractor:
    """utils/mesh_utils.py:72-181, bounded path: render(viewpoint_cam, gaussians, pipe, bg_color) must return the reference's dict."""

    def __init__(self, gaussians, render, pipe, bg_color=None):
        if bg_color is None:
            bg_color = [0, 0, 0]
        dev = gaussians.get_xyz.device if hasattr(gaussians, "get_xyz") else torch.device("cuda")
        self.gaussians = gaussians
        self.background = torch.tensor(bg_color, dtype=torch.float32, device=dev)
        self.render = lambda cam, g: render(cam, g, pipe, self.background)
        self.budget_bytes = DEFAULT_BUDGET
        self.timings = None
        self.clean()

    def clean(self):
        self.depthmaps, self.rgbmaps, self.viewpoint_stack = [], [], []

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack):
        """Renders every view; surf_depth and render stay on the device."""
        self.clean()
        self.viewpoint_stack = viewpoint_stack
        t = _Timer(self.timings, self.background.device)
        for cam in self.viewpoint_stack:
            pkg = self.render(cam, self.gaussians)
            self.rgbmaps.append(pkg["render"].detach())
            self.depthmaps.append(pkg["surf_depth"].detach())
        t.lap("render")
        self.estimate_bounding_sphere()

    def estimate_bounding_sphere(self):
        c2ws = np.array([np.linalg.inv(np.asarray(cam.world_view_transform.detach().cpu().numpy(), np.float64).T) for cam in self.viewpoint_stack])
        center, self.radius = bounding_sphere(c2ws)
        self.center = torch.from_numpy(center).float().to(self.background.device)
        print("The estimated bounding radius is %.2f" % self.radius)
        print("Use at least %.2f for depth_trunc" % (2.0 * self.radius))

    @torch.no_grad()
    def extract_mesh_bounded(self, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3, mask_backgrond=True):
        """TSDF fusion of every reconstructed view and marching cubes (MESH.md).  Returns a TriangleMesh on the device."""
        depths, rgbas, cams = [], [], []
        for i, cam in enumerate(self.viewpoint_stack):
            mask = getattr(cam, "gt_alpha_mask", None) if mask_backgrond else None
            d, rgba = prepare_view(self.depthmaps[i], self.rgbmaps[i], mask, depth_trunc)
            depths.append(d); rgbas.append(rgba)
            cams.append(torch.from_numpy(camera_block(cam)).to(d.device))
        vol = fuse(depths, rgbas, cams, voxel_size, sdf_trunc, depth_trunc, self.budget_bytes, self.background.device, self.timings)
        t = _Timer(self.timings, self.background.device)
        mesh = vol.extract()
        t.lap("extract")
        self.volume = vol
        return mesh

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=1024, slab=0):
        """Contracted-lattice fusion and marching cubes (MESH.md §Unbounded, utils/mesh_utils.py:184-280).  resolution must be a
        multiple of 512; the lattice holds (resolution/512) * 511 + 1 samples per axis.  Returns a TriangleMesh on the device."""
        if resolution <= 0 or resolution % 512 != 0:
            raise ValueError("extract_mesh_unbounded: resolution must be a positive multiple of 512, got %r" % (resolution,))
        dev = self.background.device
        M = lattice_size(resolution)
        voxel_size = self.radius * 2 / resolution
        R = lattice_half_width(self.gaussians.get_xyz, self.center, self.radius)
        print("Computing sdf grid resolution %d x %d x %d (lattice %d^3, half-width %.4f)" % (resolution, resolution, resolution, M, R))
        print("Define the voxel_size as %g" % voxel_size)
        lat = UnboundedLattice(M, R, self.center, self.radius, voxel_size, self.budget_bytes, dev, slab=slab)
        t = _Timer(self.timings, dev)
        views, depth, rgb = pack_views([c.full_proj_transform for c in self.viewpoint_stack], self.depthmaps, self.rgbmaps)
        lat.fuse(views, depth)
        t.lap("fuse")
        verts, tris = lat.extract()
        t.lap("extract")
        cols = color_vertices(verts, views, depth, rgb, 5 * voxel_size)
        t.lap("color")
        self.lattice = lat
        return TriangleMesh(verts, tris, cols)

    @torch.no_grad()
    def export_image(self, path, vis=False, png="pillow"):
        """utils/mesh_utils.py:282-292: path/renders/%05d.png from rgbmaps and path/gt/%05d.png from original_image[0:3], quantised as
        save_img_u8 does (render_utils.py:270-275): NaN -> 0, clip to [0, 1], times 255, truncated to uint8.  What
        surfel_metrics.evaluate reads (METRICS.md).  vis=False leaves vis/ out and converts on the host; vis=True adds
        path/vis/depth_%05d.tiff (float32, save_img_f32's values) and takes every file through the device-side conversion and the
        writer threads of surfel_path (RENDER.md): the same pixels.  png="device" encodes the PNG files on the device (PNG.md) through the
        same conversion and writer, with or without vis: the same names, files that decode to the same pixels."""
        if png not in ("pillow", "device"):
            raise ValueError("export_image: png must be 'pillow' or 'device', got %r" % (png,))
        render_path, gts_path = os.path.join(path, "renders"), os.path.join(path, "gt")
        os.makedirs(render_path, exist_ok=True)
        os.makedirs(gts_path, exist_ok=True)
        if vis or png == "device":
            import surfel_path
            vis_path = os.path.join(path, "vis")
            if vis:
                os.makedirs(vis_path, exist_ok=True)
            dev = self.background.device
            with surfel_path.FrameWriter(png=png) as fw:
                for idx, cam in enumerate(self.viewpoint_stack):
                    fw.submit(os.path.join(gts_path, "%05d.png" % idx), surfel_path.quantize_u8(cam.original_image[0:3].to(dev)))
                    fw.submit(os.path.join(render_path, "%05d.png" % idx), surfel_path.quantize_u8(self.rgbmaps[idx]))
                    if vis:
                        fw.submit(os.path.join(vis_path, "depth_%05d.tiff" % idx), self.depthmaps[idx][0])
            return
        from PIL import Image
        for idx, cam in enumerate(self.viewpoint_stack):
            for img, folder in ((cam.original_image[0:3], gts_path), (self.rgbmaps[idx], render_path)):
                a = img.detach().permute(1, 2, 0).cpu().numpy()
                u8 = (np.clip(np.nan_to_num(a), 0.0, 1.0) * 255.0).astype(np.uint8)
                Image.fromarray(u8).save(os.path.join(folder, "%05d.png" % idx), "PNG")


def cluster_triangles(mesh):
    """(label [F] = smallest triangle id of the triangle's edge-connected cluster, size [F] = triangles per label id)."""
    tris = mesh.triangles.contiguous()
    F, V = int(tris.shape[0]), int(mesh.vertices.shape[0])
    label = torch.empty(F, dtype=torch.int32, device=tris.device)
    size = torch.empty(F, dtype=torch.int32, device=tris.device)
    alloc = _n.TorchAllocator(tris.device)
    _n.call(tris.device, "surfel_mesh_clusters", alloc.cb, None, V, F, tris, label, size)
    return label, size


def post_process_mesh(mesh, cluster_to_keep=1000):
    """utils/mesh_utils.py:22-41: keeps the clusters with at least max(k-th largest cluster size, 50) triangles (50 when there are
    fewer than k clusters), then drops unreferenced vertices (order kept) and triangles that repeat an index."""
    print("post processing the mesh to have {} clusterscluster_to_kep".format(cluster_to_keep))
    dev = mesh.triangles.device
    F, V = int(mesh.triangles.shape[0]), int(mesh.vertices.shape[0])
    if F == 0:
        return TriangleMesh(mesh.vertices[:0], mesh.triangles[:0], mesh.vertex_colors[:0])
    label, size = cluster_triangles(mesh)
    counts = size[size > 0].sort().values        # one entry per cluster: a few numbers, selected on the device
    threshold = int(counts[-cluster_to_keep]) if cluster_to_keep <= counts.numel() else 0
    threshold = max(threshold, 50)
    vout = torch.empty((V, 3), dtype=torch.float32, device=dev)
    cout = torch.empty((V, 3), dtype=torch.float32, device=dev)
    tout = torch.empty((F, 3), dtype=torch.int32, device=dev)
    n = (C.c_int64 * 2)()
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_mesh_filter", alloc.cb, None, V, F, mesh.vertices.contiguous(), mesh.vertex_colors.contiguous(), mesh.triangles.contiguous(),
            label, size, threshold, vout, cout, tout, n)
    print("num vertices raw {}".format(V))
    print("num vertices post {}".format(int(n[0])))
    return TriangleMesh(vout[:n[0]], tout[:n[1]], cout[:n[0]])


# ------------------------------------------------------------------------------------------------ CLI (render.py:86-106)
def _latest_iteration(model_dir):
    its = [int(d.split("_")[-1]) for d in os.listdir(os.path.join(model_dir, "point_cloud")) if d.startswith("iteration_")]
    if not its:
        raise FileNotFoundError("no point_cloud/iteration_* under %s" % model_dir)
    return max(its)


def _scene_cameras(args, gaussians, it):
    """(train, test) cameras of the capture at args.source_path, loaded the way the training run loaded them: images folder, resolution,
    split, background and undistortion from model_path/cfg_args (surfel_trainer.write_cfg_args) where it exists."""
    from surfel_scene import Scene
    cfg = argparse.Namespace(images="images", resolution=-1, eval=False, white_background=False)
    path = os.path.join(args.model_path, "cfg_args")
    if os.path.exists(path):
        cfg = eval(open(path).read(), {"Namespace": argparse.Namespace, "__builtins__": {}})
    args.white_background = args.white_background or getattr(cfg, "white_background", False)      # renders over what the images were composited on
    scene = Scene(args.source_path, args.model_path, images=getattr(cfg, "images", "images"), resolution=getattr(cfg, "resolution", -1),
                  white_background=args.white_background, eval=getattr(cfg, "eval", False),
                  data_device=str(gaussians.device), load_iteration=it, shuffle=False, gaussians=gaussians, decode=getattr(args, "decode", "host"),
                  undistort=bool(getattr(args, "undistort", False) or getattr(cfg, "undistort", False)))
    return scene.getTrainCameras(), scene.getTestCameras()


def open_model(args, device):
    """What the tools that run a pass over a trained model's views open (surfel_prune.py, surfel_select.py), from args.model_path,
    args.iteration (< 0: the latest), args.source_path (None: the cameras of cameras.json) and args.white_background:
    (gaussians, cameras, iteration, the iteration's folder, pipe, background)."""
    import surfel_io
    import surfel_model
    it = args.iteration if args.iteration >= 0 else _latest_iteration(args.model_path)
    gaussians = surfel_model.GaussianModel(3, device=device)
    folder = os.path.join(args.model_path, "point_cloud", "iteration_%d" % it)
    if args.source_path is None:
        gaussians.load_ply(os.path.join(folder, "point_cloud.ply"))
        cams = surfel_io.read_cameras_json(os.path.join(args.model_path, "cameras.json"), device=device)
    else:
        cams, _ = _scene_cameras(args, gaussians, it)      # (loads the point cloud of iteration `it` into gaussians)
    pipe = argparse.Namespace(depth_ratio=0.0, debug=0, compute_cov3D_python=False, convert_SHs_python=False)
    background = torch.tensor([1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    return gaussians, cams, it, folder, pipe, background


def build_parser():
    ap = argparse.ArgumentParser(description="TSDF mesh of a trained model (render.py's mesh step), bounded or --unbounded. Unlike the reference, which "
                                             "fuses only the training split, every camera in cameras.json is fused.  --render_path adds "
                                             "render.py's trajectory mode (RENDER.md).")
    ap.add_argument("-m", "--model_path", required=True)
    ap.add_argument("--iteration", default=-1, type=int)
    ap.add_argument("--voxel_size", default=-1.0, type=float, help="Mesh: voxel size for TSDF (default depth_trunc / mesh_res)")
    ap.add_argument("--depth_trunc", default=-1.0, type=float, help="Mesh: max depth range for TSDF (default 2 x bounding radius)")
    ap.add_argument("--sdf_trunc", default=-1.0, type=float, help="Mesh: truncation value for TSDF (default 5 x voxel_size)")
    ap.add_argument("--num_cluster", default=50, type=int, help="Mesh: number of connected clusters to export")
    ap.add_argument("--mesh_res", default=1024, type=int, help="Mesh: resolution for unbounded mesh extraction")
    ap.add_argument("--depth_ratio", default=0.0, type=float)
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--unbounded", action="store_true", help="Mesh: unbounded mode (contracted lattice of mesh_res, a multiple of 512)")
    ap.add_argument("--budget_gb", default=DEFAULT_BUDGET / 2 ** 30, type=float, help="byte budget of the TSDF volume (GiB)")
    ap.add_argument("-s", "--source_path", default=None, help="the capture the model was trained on: cameras and ground-truth images come from it "
                    "(surfel_scene.Scene, with the model's cfg_args), only the training split is fused, and renders / gt of both splits are exported")
    ap.add_argument("--undistort", action="store_true", help="with -s: undistort the capture while it is loaded (UNDISTORT.md); implied by a model "
                    "folder that was trained with --undistort")
    ap.add_argument("--skip_train", action="store_true", help="with -s: do not export the training split's renders / gt")
    ap.add_argument("--skip_test", action="store_true", help="with -s: do not export the test split's renders / gt")
    ap.add_argument("--skip_mesh", action="store_true", help="do not extract a mesh")
    ap.add_argument("--render_path", action="store_true", help="render an elliptical fly-through of the training cameras (the capture's with -s, "
                    "cameras.json otherwise) into MODEL/traj/ours_N: renders/, vis/depth_*.tiff, video/depth/")
    ap.add_argument("--n_frames", default=240, type=int, help="Path: number of frames of --render_path")
    ap.add_argument("--vis_normals", action="store_true", help="Path: also write vis/normal_*.png")
    ap.add_argument("--video", action="store_true", help="Path: also write render_traj_{color,depth}.avi (and _normal with --vis_normals): "
                    "Motion-JPEG encoded on the device (VIDEO.md)")
    ap.add_argument("--video_only", action="store_true", help="Path: write the videos and none of the per-frame files")
    ap.add_argument("--video_quality", default=95, type=int, help="Path: JPEG quality of the videos' frames, 1 .. 100")
    ap.add_argument("--fps", default=60, type=int, help="Path: frame rate of the videos")
    ap.add_argument("--png", default="pillow", choices=["pillow", "device"], help="who encodes the PNG files of --render_path and of the renders / gt "
                    "export: Pillow on host threads (the default) or the encoder on the device (PNG.md); the same names and pixels")
    ap.add_argument("--render_mesh", action="store_true", help="Path: with --render_path, also fly the same path around the mesh this run writes "
                    "(with --skip_mesh: around the existing fuse_post.ply / fuse_unbounded_post.ply) into MODEL/traj/ours_N/mesh/ (MESHVIEW.md)")
    ap.add_argument("--mesh_modes", nargs="+", default=["shaded", "normal"], choices=["shaded", "normal", "color", "depth"],
                    help="Path: the frame sets of --render_mesh: mesh/{mode}_%%05d.png, and render_traj_mesh_{mode}.avi with --video")
    ap.add_argument("--mesh_ssaa", default=2, type=int, choices=[1, 2, 3, 4], help="Path: samples per pixel edge of --render_mesh")
    ap.add_argument("--decode", default="host", choices=["host", "device"], help="with -s: who decodes the capture's JPEG files: Pillow on the host "
                    "(the default) or the decoder on the device (JPEGDEC.md); the same cameras")
    ap.add_argument("--simplify_cell", default=None, type=float, help="Mesh: also write fuse_post_simplified.ply (fuse_unbounded_post_simplified.ply), "
                    "the post-processed mesh clustered on a grid of this many voxels per cell (SIMPLIFY.md)")
    ap.add_argument("--simplify_faces", default=None, type=int, help="Mesh: the same file, with the grid chosen so that at most this many triangles "
                    "remain")
    ap.add_argument("--texture", action="store_true", help="Mesh: also write fuse_post_textured.{obj,mtl,png} (fuse_unbounded_post_textured.*): the "
                    "post-processed mesh — the simplified one when a --simplify_* flag is given — with the fused views baked into a texture "
                    "atlas (TEXTURE.md)")
    ap.add_argument("--atlas_size", default=4096, type=int, help="Mesh: the side of --texture's atlas in texels")
    ap.add_argument("--smooth_iterations", default=None, type=int, help="Mesh: also write fuse_post_smoothed.ply (fuse_unbounded_post_smoothed.ply), "
                    "the post-processed mesh after this many filter iterations (SMOOTH.md); --simplify_* and --texture then continue from it")
    ap.add_argument("--smooth_method", default="taubin", choices=["taubin", "laplacian"], help="Mesh: the filter of --smooth_iterations")
    ap.add_argument("--smooth_boundary", default="free", choices=["free", "fixed", "curve"], help="Mesh: what --smooth_iterations does at the "
                    "mesh's border: every neighbour counts, boundary vertices stay, or they average along the border only")
    ap.add_argument("--repair", action="store_true", help="Mesh: also write fuse_post_repaired.ply (fuse_unbounded_post_repaired.ply), the "
                    "post-processed mesh with its non-manifold edges cut, its vertices split into one fan each and its small holes closed "
                    "(REPAIR.md); --smooth_iterations, --simplify_*, --texture and --render_mesh then continue from it")
    ap.add_argument("--repair_max_hole", default=32, type=int, help="Mesh: --repair closes the border loops of at most this many edges")
    return ap


def path_video_args(args):
    """render_path's video arguments from the CLI's: none at all unless a video was asked for"""
    if not (args.video or args.video_only):
        return {}
    return dict(video=True, video_only=args.video_only, video_quality=args.video_quality, fps=args.fps)


def path_png_args(args):
    """render_path's and export_image's png argument from the CLI's: none at all unless the device encoder was asked for"""
    return dict(png=args.png) if args.png != "pillow" else {}


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.simplify_cell is not None and args.simplify_faces is not None:
        raise SystemExit("give --simplify_cell or --simplify_faces, not both")
    if args.simplify_cell is not None and not args.simplify_cell > 0:
        raise SystemExit("--simplify_cell must be positive")
    if args.smooth_iterations is not None and args.smooth_iterations < 0:
        raise SystemExit("--smooth_iterations must not be negative")
    if args.repair_max_hole < 0:
        raise SystemExit("--repair_max_hole must not be negative")
    import surfel_io
    import surfel_model
    from surfel_render import render
    dev = torch.device("cuda")
    it = _latest_iteration(args.model_path) if args.iteration < 0 else args.iteration
    gaussians = surfel_model.GaussianModel(3, device=dev)
    test_cams = []
    if args.source_path is None:
        gaussians.load_ply(os.path.join(args.model_path, "point_cloud", "iteration_%d" % it, "point_cloud.ply"))
        cams = surfel_io.read_cameras_json(os.path.join(args.model_path, "cameras.json"), device=dev)
    else:
        cams, test_cams = _scene_cameras(args, gaussians, it)      # (loads the point cloud of iteration `it` into gaussians)
    pipe = argparse.Namespace(depth_ratio=args.depth_ratio, debug=0, compute_cov3D_python=False, convert_SHs_python=False)
    ext = GaussianExtractor(gaussians, render, pipe, bg_color=[1, 1, 1] if args.white_background else [0, 0, 0])
    ext.budget_bytes = int(args.budget_gb * 2 ** 30)
    out = os.path.join(args.model_path, "train", "ours_%d" % it)
    os.makedirs(out, exist_ok=True)
    if args.source_path is not None:      # render.py:68-84: renders (at the trained SH degree) / gt of both splits, where surfel_metrics.py looks for them
        for split, split_cams, skip in (("train", cams, args.skip_train), ("test", test_cams, args.skip_test)):
            if split_cams and not skip:
                ext.reconstruction(split_cams)
                ext.export_image(os.path.join(args.model_path, split, "ours_%d" % it), **path_png_args(args))
    if args.render_path:      # render.py:73-84, at the trained SH degree
        import surfel_path
        traj_dir = os.path.join(args.model_path, "traj", "ours_%d" % it)
        surfel_path.render_path(gaussians, cams, render, pipe, ext.background, traj_dir, n_frames=args.n_frames, vis_normals=args.vis_normals,
                                **path_video_args(args), **path_png_args(args))
        print("trajectory frames saved at {}".format(traj_dir))
    post_name = "fuse_unbounded_post.ply" if args.unbounded else "fuse_post.ply"

    def render_mesh_path(mesh):
        """--render_path --render_mesh: the path of the surfels' fly-through around the mesh, beside traj/ours_N/renders"""
        import surfel_meshview
        surfel_meshview.render_mesh_path(mesh, cams, traj_dir, n_frames=args.n_frames, modes=tuple(args.mesh_modes), ssaa=args.mesh_ssaa,
                                         **path_video_args(args), **path_png_args(args))
        print("mesh trajectory frames saved at {}".format(os.path.join(traj_dir, "mesh")))

    if args.skip_mesh:
        if args.render_path and args.render_mesh:
            render_mesh_path(read_mesh(os.path.join(out, post_name), dev))
        return 0
    gaussians.active_sh_degree = 0      # render.py:91: diffuse colour only
    ext.reconstruction(cams)
    if args.unbounded:
        name = "fuse_unbounded.ply"
        mesh = ext.extract_mesh_unbounded(resolution=args.mesh_res)
        voxel_size = ext.radius * 2 / args.mesh_res      # (the unbounded lattice's voxel near the centre)
    else:
        name = "fuse.ply"
        depth_trunc = ext.radius * 2.0 if args.depth_trunc < 0 else args.depth_trunc
        voxel_size = depth_trunc / args.mesh_res if args.voxel_size < 0 else args.voxel_size
        sdf_trunc = 5.0 * voxel_size if args.sdf_trunc < 0 else args.sdf_trunc
        mesh = ext.extract_mesh_bounded(voxel_size=voxel_size, sdf_trunc=sdf_trunc, depth_trunc=depth_trunc)
    surfel_io.write_triangle_mesh(os.path.join(out, name), mesh)
    print("mesh saved at {}".format(os.path.join(out, name)))
    post = post_process_mesh(mesh, cluster_to_keep=args.num_cluster)
    surfel_io.write_triangle_mesh(os.path.join(out, name.replace(".ply", "_post.ply")), post)
    print("mesh post processed saved at {}".format(os.path.join(out, name.replace(".ply", "_post.ply"))))
    if args.repair:      # before the filter, which then evens out the fill fans; the steps below continue from the repaired mesh
        import surfel_repair
        post, stats = surfel_repair.repair_mesh(post, max_hole_edges=args.repair_max_hole)
        repair_path = os.path.join(out, name.replace(".ply", "_post_repaired.ply"))
        surfel_io.write_triangle_mesh(repair_path, post)
        print("mesh repaired ({}) saved at {}".format(surfel_repair.summary(stats), repair_path))
    if args.smooth_iterations is not None:      # the steps below continue from the smoothed mesh
        import surfel_smooth
        post, stats = surfel_smooth.smooth_mesh(post, iterations=args.smooth_iterations, method=args.smooth_method, boundary=args.smooth_boundary)
        smooth_path = os.path.join(out, name.replace(".ply", "_post_smoothed.ply"))
        surfel_io.write_triangle_mesh(smooth_path, post)
        print("mesh smoothed ({}, {} steps, {} border and {} non-manifold edges) saved at {}".format(args.smooth_method, stats["steps"],
                                                                                                 stats["border_edges"], stats["nonmanifold_edges"], smooth_path))
    if args.simplify_cell is not None or args.simplify_faces is not None:
        import surfel_simplify
        cell = None if args.simplify_cell is None else args.simplify_cell * voxel_size
        simple, stats = surfel_simplify.simplify_mesh(post, cell=cell, target_faces=args.simplify_faces)
        simple_path = os.path.join(out, name.replace(".ply", "_post_simplified.ply"))
        surfel_io.write_triangle_mesh(simple_path, simple)
        print("mesh simplified ({} of {} triangles, cell {:g}) saved at {}".format(simple.triangles.shape[0], post.triangles.shape[0], stats["cell"],
                                                                                  simple_path))
    if args.texture:      # from the views reconstruction() holds: no second render
        import surfel_texture
        base = simple if (args.simplify_cell is not None or args.simplify_faces is not None) else post
        tm = surfel_texture.texture_mesh(base, cams, ext.rgbmaps, atlas_size=args.atlas_size)
        paths = surfel_texture.save_textured_mesh(os.path.join(out, name.replace(".ply", "_post_textured")), tm, png=args.png)
        print("mesh textured ({} triangles, atlas {} x {}, {} of {} owned texels seen) saved at {}".format(
            base.triangles.shape[0], tm.atlas.shape[1], tm.atlas.shape[0], tm.seen, tm.owned, paths[0]))
    if args.render_path and args.render_mesh:
        render_mesh_path(post)
    return 0


if __name__ == "__main__":
    sys.exit(main())
