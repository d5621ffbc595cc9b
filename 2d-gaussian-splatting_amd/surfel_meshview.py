"""Render an extracted mesh on MI355X — shaded, normal, colour and depth frames of fuse_post.ply, fuse_unbounded_post.ply or a *_cull.ply
without OpenGL, Open3D or a display: as a fly-through next to the surfels' own frames, as a video, or in the remote viewer.

A visibility buffer (the rasteriser of the view culling with a 64-bit key per pixel: depth bits and triangle index), angle-free vertex
normals and a shading pass are HIP kernels of libsurfel_hip.so (include/surfel_meshview.h); MESHVIEW.md states the rules and every
operation order.  The mesh, the keys and the frames stay on the device.  No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_meshview.py --ply-path MESH.ply -m MODEL_DIR [--views path|train]     -> MESH_view/mesh/
    python 2d-gaussian-splatting_amd/surfel_meshview.py --ply-path MESH.ply --traj-path TRAJ.{json,npy}
"""
import argparse
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import torch

import surfel_native as _n
import surfel_cull as _c
import surfel_path as _sp
from surfel_mesh import MeshLimitError, TriangleMesh, mesh_arrays, read_mesh, shown_colors  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

DEFAULT_BUDGET = _c.DEFAULT_BUDGET
ZNEAR, ZFAR = 0.01, 1000.0
MODES = ("shaded", "normal", "color", "depth")
TEXTURED = "textured"                                      # render_mesh's mode that takes a surfel_texture.TexturedMesh (TEXTURE.md)
_KERNEL_MODE = {"shaded": 0, "normal": 1, "color": 2}      # SURFEL_MESHVIEW_SHADED, _NORMAL, _COLOR
MAX_SSAA = 4                                               # SURFEL_MESHVIEW_MAX_SSAA
NORMAL_SCALE = 1 << 20                                     # SURFEL_MESHVIEW_NORMAL_SCALE
EMPTY_KEY = (0x7f800000 << 32) | 0xffffffff                # SURFEL_MESHVIEW_EMPTY


_dev = functools.partial(_n.device_tensor, "surfel_meshview")
_mesh_arrays = functools.partial(mesh_arrays, "surfel_meshview", shapes=("[V, 3]", "[F, 3]"))


def _device_cameras(w2c, intrinsics, dev):
    """surfel_cull._cameras, except that cameras which are on the device already — w2c float32 [n, 12], intrinsics float32 [1 | n, 4], as
    that function returns them — pass as they are: no round trip through the host, which a loop over frames would wait for"""
    if (torch.is_tensor(w2c) and torch.is_tensor(intrinsics) and w2c.is_cuda and intrinsics.is_cuda and w2c.dtype == intrinsics.dtype == torch.float32
            and w2c.ndim == 2 and w2c.shape[1] == 12 and intrinsics.ndim == 2 and intrinsics.shape[1] == 4 and intrinsics.shape[0] in (1, w2c.shape[0])):
        return w2c.contiguous(), intrinsics.contiguous()
    return _c._cameras(w2c, intrinsics, dev)


def scaled_intrinsics(intrinsics, ssaa):
    """(fx, fy, cx, cy) of the ssaa H x ssaa W sample grid, [n, 4] float64: fx s, fy s, s cx + (s - 1) / 2, s cy + (s - 1) / 2 — sample
    s x + k sits at the pixel coordinate x + (k + 0.5) / s - 0.5."""
    k = np.asarray(intrinsics.detach().cpu() if torch.is_tensor(intrinsics) else intrinsics, np.float64).reshape(-1, 4)
    s = int(ssaa)
    return np.stack([k[:, 0] * s, k[:, 1] * s, s * k[:, 2] + (s - 1) / 2, s * k[:, 3] + (s - 1) / 2], 1)


def visibility(mesh, w2c, intrinsics, H, W, znear=ZNEAR, zfar=ZFAR, small_pixels=-1, timings=None):
    """int64 keys [V, H, W] on the device: per pixel (fp32 bits of z) << 32 | triangle index of the nearest triangle its ray hits,
    EMPTY_KEY where none — surfel_cull.mesh_depth's cameras, rules and arguments (MESHVIEW.md §Visibility).  The depth half is
    mesh_depth's image bit for bit; among triangles of equal depth bits the lowest index wins; the same bits on every run."""
    verts, tris = _mesh_arrays(mesh)
    dev = verts.device
    w, k = _device_cameras(w2c, intrinsics, dev)
    key = torch.empty((w.shape[0], int(H), int(W)), dtype=torch.int64, device=dev)
    ms = (C.c_float * 3)() if timings is not None else None
    alloc = _n.TorchAllocator(dev)
    queued = _n.call(dev, "surfel_meshview_visibility", alloc.cb, None, verts.shape[0], tris.shape[0], verts, tris, w.shape[0], w, k, k.shape[0], int(H),
                     int(W), float(znear), float(zfar), int(small_pixels), key, ms)
    if timings is not None:
        timings.update(small_ms=float(ms[0]), large_ms=float(ms[1]), other_ms=float(ms[2]), large_pairs=int(queued))
    return key


def unpack(key):
    """(depth float32 with 0 where empty, triangle int32 with -1 where empty) of a key tensor"""
    key = _dev(key, "key")
    depth = (key >> 32).to(torch.int32).view(torch.float32)
    empty = torch.isinf(depth)
    tri = (key & 0xffffffff).to(torch.int32)      # (0xffffffff wraps to -1)
    return torch.where(empty, torch.zeros_like(depth), depth), torch.where(empty, torch.full_like(tri, -1), tri)


def vertex_normals(mesh, return_sums=False):
    """float32 [V, 3]: the normalised sum of the unit face normals around every vertex, accumulated in fixed point (2^-20) with integer
    atomics, so the same bits on every run (MESHVIEW.md §Vertex normals); (0, 0, 0) where nothing adds up.  return_sums: also the int64 sums."""
    verts, tris = _mesh_arrays(mesh)
    acc = torch.empty((verts.shape[0], 3), dtype=torch.int64, device=verts.device)
    normals = torch.empty((verts.shape[0], 3), dtype=torch.float32, device=verts.device)
    _n.call(verts.device, "surfel_meshview_vertex_normals", verts.shape[0], tris.shape[0], verts, tris, acc, normals)
    return (normals, acc) if return_sums else normals


def shade(mesh, key, w2c, sample_intrinsics, H, W, ssaa=1, mode="shaded", normals=None, albedo="color", background=(1.0, 1.0, 1.0), out=None):
    """uint8 [V, H, W, 3]: the frames of a key tensor [V, ssaa H, ssaa W] that visibility() made for the same mesh and cameras
    (sample_intrinsics: those of the sample grid).  normals: vertex_normals(mesh) for the smooth look, None for flat."""
    if mode not in _KERNEL_MODE:
        raise ValueError("surfel_meshview: shade() has the modes %s, got %r" % (", ".join(_KERNEL_MODE), mode))
    if albedo not in ("color", "grey"):
        raise ValueError("surfel_meshview: albedo must be 'color' or 'grey', got %r" % (albedo,))
    verts, tris = _mesh_arrays(mesh)
    dev = verts.device
    key = _dev(key, "key")
    s = int(ssaa)
    if not 1 <= s <= MAX_SSAA:
        raise ValueError("surfel_meshview: ssaa must be 1 .. %d, got %r" % (MAX_SSAA, ssaa))
    if key.dtype != torch.int64 or key.ndim != 3 or tuple(key.shape[1:]) != (int(H) * s, int(W) * s) or not key.is_contiguous():
        raise ValueError("surfel_meshview: key must be a contiguous int64 [V, %d, %d], got %s %s" % (int(H) * s, int(W) * s, key.dtype, list(key.shape)))
    w, k = _device_cameras(w2c, sample_intrinsics, dev)
    if w.shape[0] != key.shape[0]:
        raise ValueError("surfel_meshview: %d cameras for %d key images" % (w.shape[0], key.shape[0]))
    cols = shown_colors("surfel_meshview", mesh, verts.shape[0]) if albedo == "color" else None
    if normals is not None:
        normals = _dev(normals, "normals")
        if tuple(normals.shape) != (verts.shape[0], 3):
            raise ValueError("surfel_meshview: normals must be [V, 3], got %s" % list(normals.shape))
        normals = normals.detach().to(torch.float32).contiguous()
    n = key.shape[0]
    out = _n.uint8_buffer("surfel_meshview", out, n * int(H) * int(W) * 3, dev)
    bg = [float(x) for x in background]
    _n.call(dev, "surfel_meshview_shade", verts.shape[0], tris.shape[0], verts, tris, cols, normals, n, w, k, k.shape[0], int(H), int(W), s, key,
            _KERNEL_MODE[mode], bg[0], bg[1], bg[2], out)
    return out.view(n, int(H), int(W), 3)


# ------------------------------------------------------------------------------------------------ cameras
def _camera_intrinsics(cam, W, H, cache):
    if getattr(cam, "intrinsics", None) is not None:
        return tuple(float(x) for x in cam.intrinsics)
    proj = getattr(cam, "projection_matrix", None)
    if proj is None:
        return (W / (2.0 * math.tan(float(cam.FoVx) / 2.0)), H / (2.0 * math.tan(float(cam.FoVy) / 2.0)), (W - 1) / 2.0, (H - 1) / 2.0)
    key = (id(proj), W, H)      # (the cameras of a path share one projection matrix: it is read from the device once)
    if key not in cache:
        from surfel_mesh import camera_intrinsics
        cache[key] = camera_intrinsics(cam)
    return cache[key]


def camera_views(cameras):
    """[(w2c [4, 4] float32, (fx, fy, cx, cy), H, W)] of the project's cameras or viewer MiniCams: w2c is world_view_transform
    transposed; the intrinsics follow surfel_mesh.camera_intrinsics (cx = (W - 1) / 2, cy = (H - 1) / 2, the focal lengths from the
    projection matrix, or from the fields of view where the camera has none; a PoseCamera carries its own).  The matrices of all
    cameras come to the host in one copy."""
    cameras = list(cameras)
    if not cameras:
        return []
    wvt = torch.stack([c.world_view_transform.detach().to(torch.float32) for c in cameras]).cpu().numpy()
    cache, out = {}, []
    for c, m in zip(cameras, wvt):
        W, H = int(c.image_width), int(c.image_height)
        out.append((np.ascontiguousarray(m.T), _camera_intrinsics(c, W, H, cache), H, W))
    return out


def camera_view(cam):
    return camera_views([cam])[0]


def _view_groups(cameras):
    """[(H, W, [view numbers], w2c [n, 4, 4], intrinsics [n, 4] float64)] of cameras given as a list of camera objects or as
    (w2c, intrinsics, H, W); views of one size form a group, in their order"""
    if isinstance(cameras, tuple) and len(cameras) == 4 and not hasattr(cameras[0], "world_view_transform"):
        w2c, k, H, W = cameras
        w = np.asarray(w2c.detach().cpu() if torch.is_tensor(w2c) else w2c, np.float32)
        k = np.asarray(k.detach().cpu() if torch.is_tensor(k) else k, np.float64).reshape(-1, 4)
        if k.shape[0] == 1:
            k = np.repeat(k, len(w), 0)
        if k.shape[0] != len(w):
            raise ValueError("surfel_meshview: intrinsics must be (fx, fy, cx, cy) or one row per view, got %s" % list(k.shape))
        return len(w), [(int(H), int(W), list(range(len(w))), w, k)]
    views = camera_views(cameras)
    groups = []
    for size in sorted({(v[2], v[3]) for v in views}):
        ids = [i for i, v in enumerate(views) if (v[2], v[3]) == size]
        groups.append((size[0], size[1], ids, np.stack([views[i][0] for i in ids]), np.asarray([views[i][1] for i in ids], np.float64)))
    return len(views), groups


def mesh_depth_limits(depth):
    """(lo, hi) for colorize_depth: surfel_path.depth_limits over the covered pixels of a depth frame (waits on the host); (0, 1) for a
    frame that shows nothing"""
    covered = depth[depth > 0]
    return _sp.depth_limits(covered) if covered.numel() else (0.0, 1.0)


@torch.no_grad()
def render_mesh(mesh, cameras, mode="shaded", smooth=True, albedo="color", ssaa=2, background=(1.0, 1.0, 1.0), budget_bytes=DEFAULT_BUDGET,
                znear=ZNEAR, zfar=ZFAR, normals=None, depth_range=None, texture=None):
    """uint8 [n, H, W, 3] frames of the mesh (on the device).  cameras: a list of the project's cameras or MiniCams of one size, or
    (w2c [n, 3 | 4, 4], intrinsics, H, W).  mode: "shaded" (albedo x headlight), "normal" (world-space normal x 0.5 + 0.5, the convention
    of vis/normal_%05d.png), "color" (vertex colours) or "depth" (turbo of log depth, surfel_path.colorize_depth).  smooth: vertex
    normals (computed here unless `normals` passes them in), else face normals.  albedo: "color" or "grey" (0.8; also for a mesh without
    colours).  ssaa 1 .. 4: samples per pixel edge.  The views go through the device in batches whose keys and frames fit budget_bytes
    (at least one view); views of one size share their batches.  "depth" samples once per pixel; depth_range = (lo, hi) of log depth,
    default: the 3rd and 97th percentile of the first view's covered pixels (waits on the host).  mode "textured": "color" with the
    colours of texture, a surfel_texture.TexturedMesh of this mesh (its atlas and texture coordinates)."""
    _check_mode(mode, texture)
    s = 1 if mode == "depth" else int(ssaa)
    if not 1 <= s <= MAX_SSAA:
        raise ValueError("surfel_meshview: ssaa must be 1 .. %d, got %r" % (MAX_SSAA, ssaa))
    verts, _ = _mesh_arrays(mesh)
    dev = verts.device
    n, groups = _view_groups(cameras)
    if len(groups) > 1:
        raise ValueError("surfel_meshview: render_mesh returns one tensor, so the cameras must share one size (render_mesh_cameras groups sizes)")
    if smooth and normals is None and mode in ("shaded", "normal"):
        normals = vertex_normals(mesh)
    if not smooth:
        normals = None
    if n == 0:
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=dev)
    H, W, _, w2c, k = groups[0]
    w, ks = _c._cameras(w2c, scaled_intrinsics(k, s), dev)
    return _render_uploaded(mesh, w, ks, H, W, s, mode, normals, albedo, background, znear, zfar, budget_bytes, depth_range, texture)[0]


def _check_mode(mode, texture):
    if mode == TEXTURED:
        if texture is None:
            raise ValueError("surfel_meshview: mode 'textured' needs texture=, a surfel_texture.TexturedMesh")
    elif mode not in MODES:
        raise ValueError("surfel_meshview: mode must be one of %s, got %r" % (", ".join(MODES + (TEXTURED,)), mode))


def _render_uploaded(mesh, w, ks, H, W, s, mode, normals, albedo, background, znear, zfar, budget_bytes, depth_range, texture=None):
    """render_mesh behind the cameras' upload: w [n, 12] and ks [n, 4] (the sample grid's intrinsics) on the device.  Returns the frames
    and the depth range that was used.  Nothing here waits on the host, except for the depth limits when a "depth" call brings none."""
    n = w.shape[0]
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=w.device)
    step = max(1, int(budget_bytes) // (8 * H * W * s * s + 3 * H * W))
    lo_hi = depth_range
    for b in range(0, n, step):
        key = visibility(mesh, w[b:b + step], ks[b:b + step], H * s, W * s, znear, zfar)
        if mode == "depth":
            depth = unpack(key)[0]
            if lo_hi is None:
                lo_hi = mesh_depth_limits(depth[0])
            for i in range(depth.shape[0]):
                _sp.colorize_depth(depth[i], lo_hi[0], lo_hi[1], out=out[b + i])
        elif mode == TEXTURED:
            import surfel_texture
            surfel_texture.shade(texture, key, w[b:b + step], ks[b:b + step], H, W, s, background, out=out[b:b + step])
        else:
            shade(mesh, key, w[b:b + step], ks[b:b + step], H, W, s, mode, normals, albedo, background, out=out[b:b + step])
        del key
    return out, lo_hi


def render_mesh_cameras(mesh, cameras, **kw):
    """render_mesh for cameras that differ in size: a list of uint8 [H, W, 3] frames in the cameras' order; views of one size share
    their batches"""
    n, groups = _view_groups(cameras)
    frames = [None] * n
    if kw.get("smooth", True) and kw.get("normals") is None and kw.get("mode", "shaded") in ("shaded", "normal"):
        kw = dict(kw, normals=vertex_normals(mesh))
    for H, W, ids, w2c, k in groups:
        got = render_mesh(mesh, (w2c, k, H, W), **kw)
        for j, i in enumerate(ids):
            frames[i] = got[j]
    return frames


@torch.no_grad()
def render_mesh_path(mesh, cameras, out_dir, n_frames=240, modes=("shaded", "normal"), video=False, video_only=False, png="pillow", smooth=True,
                     albedo="color", ssaa=2, background=(1.0, 1.0, 1.0), workers=4, video_quality=95, fps=60, znear=ZNEAR, zfar=ZFAR, path=True,
                     timings=None, texture=None):
    """The mesh along surfel_path.generate_path's trajectory through `cameras` (the one render_path flies): out_dir/mesh/{mode}_%05d.png
    through a FrameWriter and, with video, out_dir/render_traj_mesh_{mode}.avi through a VideoWriter (video_only: the videos and no
    frame files).  path=False: one frame per camera of `cameras` instead (they may differ in size; no video then unless they share one).
    The loop does not wait on the host per frame: the one wait is frame 0's depth limits when "depth" is among the modes.  Returns the
    cameras that were rendered.  texture: the surfel_texture.TexturedMesh of the mode "textured"."""
    import time
    for m in modes:
        _check_mode(m, texture)
    traj = _sp.generate_path(cameras, n_frames=n_frames) if path else list(cameras)
    video = video or video_only
    os.makedirs(out_dir, exist_ok=True)
    folder = None if video_only else _sp._folders(out_dir, ["mesh"])[0]
    fw = None if video_only else _sp.FrameWriter(workers=workers, png=png)
    writers = {}
    normals = vertex_normals(mesh) if smooth and any(m in ("shaded", "normal") for m in modes) else None
    lo_hi = None
    # every camera is read and uploaded before the loop: per size, w2c and the intrinsics of each sample grid the modes need
    dev = _mesh_arrays(mesh)[0].device
    _, groups = _view_groups(traj)
    where = {}
    for H, W, ids, w2c, k in groups:
        grids = {g: _c._cameras(w2c, scaled_intrinsics(k, g), dev) for g in {1 if m == "depth" else int(ssaa) for m in modes}}
        for j, i in enumerate(ids):
            where[i] = (H, W, j, grids)

    def finish_videos():
        first = None
        for w in writers.values():
            try:
                w.close()
            except BaseException as e:
                first = first or e
        return first

    t0 = time.perf_counter()
    try:
        for idx in range(len(traj)):
            H, W, j, grids = where[idx]
            for m in modes:
                g = 1 if m == "depth" else int(ssaa)
                w, ks = grids[g]
                frames, used = _render_uploaded(mesh, w[j:j + 1], ks[j:j + 1], H, W, g, m, normals if m in ("shaded", "normal") else None, albedo,
                                                background, znear, zfar, DEFAULT_BUDGET, lo_hi, texture)
                frame = frames[0]
                if m == "depth":
                    lo_hi = used      # (frame 0's limits serve every frame)
                if fw is not None:
                    fw.submit(os.path.join(folder, "%s_%05d.png" % (m, idx)), frame)
                if video:
                    if m not in writers:
                        import surfel_video
                        writers[m] = surfel_video.VideoWriter(os.path.join(out_dir, "render_traj_mesh_%s.avi" % m), frame.shape[0], frame.shape[1],
                                                              fps=fps, quality=video_quality)
                    writers[m].add_frame(frame)
        if timings is not None:
            timings.update(loop_ms=(time.perf_counter() - t0) * 1e3, files=fw.frames if fw else 0, videos=sorted(writers), depth_limits=lo_hi)
    except BaseException:
        if fw is not None:
            fw._drain()
        finish_videos()
        raise
    try:
        if fw is not None:
            fw.close()
    finally:
        error = finish_videos()
    if error is not None:
        raise error
    return traj


# ------------------------------------------------------------------------------------------------ CLI
class PoseCamera:
    """what camera_view reads, for a world-to-camera matrix with explicit intrinsics (the principal point need not be the centre)"""

    def __init__(self, w2c, intrinsics, H, W):
        self.image_height, self.image_width = int(H), int(W)
        self.world_view_transform = torch.from_numpy(np.ascontiguousarray(np.asarray(w2c, np.float32).T))
        self.intrinsics = tuple(float(x) for x in intrinsics)


def build_parser():
    ap = argparse.ArgumentParser(description="Render a mesh (.ply) as shaded / normal / colour / depth frames or videos (MESHVIEW.md)")
    ap.add_argument("--ply-path", type=str, required=True, help="the mesh; frames go to MESH_view/mesh/ unless --out says otherwise")
    ap.add_argument("-m", "--model_path", type=str, default=None, help="the cameras of MODEL_DIR/cameras.json")
    ap.add_argument("--traj-path", type=str, default=None, help="instead of -m: a .npy pose stack or a transforms .json (surfel_cull.read_trajectory), "
                    "one frame per pose with the Tanks-and-Temples intrinsics or --height/--width/--fx/--fy/--cx/--cy")
    ap.add_argument("--views", type=str, default="path", choices=["path", "train"], help="with -m: the elliptical fly-through of the cameras (path), or "
                    "one frame per camera, to compare with train/ours_N/renders (train)")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--n_frames", type=int, default=240)
    ap.add_argument("--mesh_modes", nargs="+", default=["shaded", "normal"], choices=list(MODES) + [TEXTURED],
                    help="textured: --ply-path names an .obj that surfel_texture.py or surfel_mesh.py --texture wrote")
    ap.add_argument("--mesh_ssaa", type=int, default=2, choices=[1, 2, 3, 4])
    ap.add_argument("--flat", action="store_true", help="face normals instead of vertex normals")
    ap.add_argument("--albedo", type=str, default="color", choices=["color", "grey"])
    ap.add_argument("--black_background", action="store_true")
    ap.add_argument("--video", action="store_true")
    ap.add_argument("--video_only", action="store_true")
    ap.add_argument("--video_quality", type=int, default=95)
    ap.add_argument("--fps", type=int, default=60)
    ap.add_argument("--png", type=str, default="pillow", choices=["pillow", "device"])
    ap.add_argument("--height", type=int, default=_c.TNT_H)
    ap.add_argument("--width", type=int, default=_c.TNT_W)
    ap.add_argument("--fx", type=float, default=_c.TNT_INTRINSICS[0])
    ap.add_argument("--fy", type=float, default=_c.TNT_INTRINSICS[1])
    ap.add_argument("--cx", type=float, default=_c.TNT_INTRINSICS[2])
    ap.add_argument("--cy", type=float, default=_c.TNT_INTRINSICS[3])
    ap.add_argument("--near", type=float, default=ZNEAR)
    ap.add_argument("--far", type=float, default=ZFAR)
    ap.add_argument("--convention", type=str, default="opengl", choices=["opengl", "opencv"], help="axes of the trajectory's poses")
    return ap


def main(argv=None):
    import surfel_io
    args = build_parser().parse_args(argv)
    if (args.traj_path is None) == (args.model_path is None):
        raise SystemExit("give --traj-path or -m MODEL_DIR")
    dev = torch.device("cuda:0")
    texture = None
    if args.ply_path.endswith(".obj"):
        import surfel_texture
        texture = surfel_texture.load_textured_mesh(args.ply_path, dev)
        mesh = texture.mesh
    else:
        mesh = read_mesh(args.ply_path, dev)
    if TEXTURED in args.mesh_modes and texture is None:
        raise SystemExit("--mesh_modes textured needs an .obj with a texture")
    stem = args.ply_path[:-4] if args.ply_path.endswith((".ply", ".obj")) else args.ply_path
    out = args.out or stem + "_view"
    common = dict(modes=tuple(args.mesh_modes), video=args.video, video_only=args.video_only, png=args.png, smooth=not args.flat, albedo=args.albedo,
                  ssaa=args.mesh_ssaa, background=(0.0, 0.0, 0.0) if args.black_background else (1.0, 1.0, 1.0), video_quality=args.video_quality,
                  fps=args.fps, znear=args.near, zfar=args.far, texture=texture)
    if args.model_path is not None:
        cams = surfel_io.read_cameras_json(os.path.join(args.model_path, "cameras.json"), device=dev)
        traj = render_mesh_path(mesh, cams, out, n_frames=args.n_frames, path=args.views == "path", **common)
    else:
        poses = _c.read_trajectory(args.traj_path)
        w2c = _c.world_to_camera(poses, args.convention).numpy()
        k = (args.fx, args.fy, args.cx, args.cy)
        traj = render_mesh_path(mesh, [PoseCamera(m, k, args.height, args.width) for m in w2c], out, path=False, **common)
    print("%d mesh frames x %s -> %s" % (len(traj), ", ".join(args.mesh_modes), out))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
