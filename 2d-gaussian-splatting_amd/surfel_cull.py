"""Cull a mesh to what the cameras saw on MI355X — the reference's scripts/eval_tnt/cull_mesh.py (the first step of its Tanks-and-Temples
recipe), without pyrender / OpenGL, trimesh or Open3D.

The depth images of the mesh and the per-vertex view count are HIP kernels of libsurfel_hip.so (include/surfel_cull.h); the rules they
follow, and where they depart from the reference, are written down in CULL.md.  The mesh and the depth images stay on the device; the
host reads trajectories, inverts the 4 x 4 poses in fp32 and writes the culled mesh.  No CPU path: CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_cull.py --traj-path TRAJ.{json,npy} --ply-path MESH.ply          -> MESH_cull.ply
    python 2d-gaussian-splatting_amd/surfel_cull.py -m MODEL_DIR --ply-path MESH.ply                          (the cameras of cameras.json)
"""
import argparse
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import torch

import surfel_native as _n
import surfel_eval as _e
from surfel_mesh import MeshLimitError, TriangleMesh, mesh_arrays, read_mesh  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

DEFAULT_BUDGET = _e.DEFAULT_BUDGET
EPS = 0.005                     # cull_mesh.py:125
MIN_VIEWS = 20                  # cull_mesh.py:175
ZNEAR, ZFAR = 0.01, 20.0        # cull_mesh.py:40, :392
# cull_mesh.py:387-391: the Tanks-and-Temples constants
TNT_H, TNT_W = 1080, 1920
TNT_INTRINSICS = (1163.8678928442187, 1172.793101201448, 962.3120628412543, 542.0667209577691)
SMALL_PIXELS = 32               # SURFEL_CULL_SMALL_PIXELS of include/surfel_cull.h


_dev = functools.partial(_n.device_tensor, "surfel_cull")
_points = functools.partial(_n.rows, "surfel_cull", dtype=torch.float32)


def _cameras(w2c, intrinsics, dev):
    """(w2c [V, 12], intrinsics [1 | V, 4]) as fp32 device tensors from host arrays or tensors: w2c [V, 3 | 4, 4], intrinsics (fx, fy, cx, cy)
    or [V, 4]."""
    w = torch.as_tensor(np.asarray(w2c.detach().cpu() if torch.is_tensor(w2c) else w2c, np.float32))
    if w.ndim != 3 or w.shape[1] not in (3, 4) or w.shape[2] != 4:
        raise ValueError("surfel_cull: w2c must be [V, 3 | 4, 4], got %s" % list(w.shape))
    k = torch.as_tensor(np.asarray(intrinsics.detach().cpu() if torch.is_tensor(intrinsics) else intrinsics, np.float32)).reshape(-1, 4)
    if k.shape[0] not in (1, w.shape[0]):
        raise ValueError("surfel_cull: intrinsics must be (fx, fy, cx, cy) or one row per view, got %s" % list(k.shape))
    if not (torch.isfinite(w).all() and torch.isfinite(k).all() and (k[:, :2] > 0).all()):
        raise ValueError("surfel_cull: the cameras hold non-finite entries or a focal length that is not positive")
    return w[:, :3, :].reshape(-1, 12).contiguous().to(dev), k.contiguous().to(dev)


def mesh_depth(mesh, w2c, intrinsics, H, W, znear=ZNEAR, zfar=ZFAR, small_pixels=-1, timings=None):
    """Depth images [V, H, W] (float32, on the device) of the mesh seen by OpenCV cameras: per pixel the smallest camera-space z in
    [znear, zfar] over the triangles its ray hits, both faces counting, 0 where none (CULL.md §Depth).  w2c: world-to-camera [V, 3 | 4, 4];
    intrinsics: (fx, fy, cx, cy) for all views or [V, 4].  small_pixels: the size-class threshold (a test argument: the images do not
    depend on it).  timings: a dict that receives ms of the small-class, large-class and other launches and the number of (view,
    triangle) pairs of the large class (synchronises)."""
    verts, tris = mesh_arrays("surfel_cull", mesh, shapes=("[N, 3]", "[F, 3]"))
    dev = verts.device
    w, k = _cameras(w2c, intrinsics, dev)
    depth = torch.empty((w.shape[0], int(H), int(W)), dtype=torch.float32, device=dev)
    ms = (C.c_float * 3)() if timings is not None else None
    alloc = _n.TorchAllocator(dev)
    queued = _n.call(dev, "surfel_cull_mesh_depth", alloc.cb, None, verts.shape[0], tris.shape[0], verts, tris, w.shape[0], w, k, k.shape[0], int(H),
                     int(W), float(znear), float(zfar), int(small_pixels), depth, ms)
    if timings is not None:
        timings.update(small_ms=float(ms[0]), large_ms=float(ms[1]), other_ms=float(ms[2]), large_pairs=int(queued))
    return depth


def view_counts(vertices, depth, w2c, intrinsics, eps=EPS, counts=None):
    """int32 [N]: in how many of the views a vertex lies in the frustum and not behind the depth image by more than eps — the valid_num of
    Mesher.point_masks (CULL.md §Visibility).  depth [V, H, W] on the device.  counts: an earlier batch's result to add to."""
    p = _points(vertices, "vertices")
    d = _dev(depth, "depth").detach().to(torch.float32).contiguous()
    if d.ndim != 3:
        raise ValueError("surfel_cull: depth must be [V, H, W], got %s" % list(d.shape))
    w, k = _cameras(w2c, intrinsics, p.device)
    if w.shape[0] != d.shape[0]:
        raise ValueError("surfel_cull: %d cameras for %d depth images" % (w.shape[0], d.shape[0]))
    if counts is None:
        counts = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
    elif _dev(counts, "counts").dtype != torch.int32 or counts.shape != (p.shape[0],) or not counts.is_contiguous():
        raise ValueError("surfel_cull: counts must be a contiguous int32 [N]")
    _n.call(p.device, "surfel_cull_visibility", p.shape[0], p, w.shape[0], w, k, k.shape[0], d.shape[1], d.shape[2], d, float(eps), counts)
    return counts


def world_to_camera(c2w, convention="opengl"):
    """fp32 world-to-camera [V, 4, 4] of camera-to-world poses [V, 3 | 4, 4]: "opengl" flips columns 1:3 first (cull_mesh.py:136), then the
    fp32 inverse (:139) on the host."""
    if convention not in ("opengl", "opencv"):
        raise ValueError("surfel_cull: convention must be 'opengl' or 'opencv', got %r" % (convention,))
    p = torch.as_tensor(np.array(c2w.detach().cpu() if torch.is_tensor(c2w) else c2w, np.float32))
    p = p[None] if p.ndim == 2 else p
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError("surfel_cull: c2w must be [V, 3 | 4, 4], got %s" % list(p.shape))
    if p.shape[1] == 3:
        p = torch.cat([p, torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).expand(p.shape[0], 1, 4)], 1)
    p = p.clone()
    if convention == "opengl":
        p[:, :3, 1:3] *= -1
    return torch.stack([torch.inverse(m) for m in p]) if p.shape[0] else p


def cull_mesh_views(mesh, c2w, intrinsics, H, W, convention="opengl", min_views=MIN_VIEWS, eps=EPS, znear=ZNEAR, zfar=ZFAR,
                    budget_bytes=DEFAULT_BUDGET, return_counts=False):
    """Mesher.cull_mesh: the mesh without the vertices that fewer than min_views cameras saw, the triangles that lose a vertex and the
    vertices no kept triangle uses (order kept, colours carried).  c2w: camera-to-world [V, 3 | 4, 4]; the views go through the device in
    batches whose depth images fit budget_bytes (at least one view).  A triangle with an index outside the vertices is dropped."""
    verts = _points(mesh.vertices, "mesh.vertices")
    tris = _dev(mesh.triangles, "mesh.triangles").detach().to(torch.int64)
    w2c = world_to_camera(c2w, convention)
    k = np.asarray(intrinsics, np.float32).reshape(-1, 4)
    if k.shape[0] not in (1, w2c.shape[0]):
        raise ValueError("surfel_cull: intrinsics must be (fx, fy, cx, cy) or one row per view, got %s" % list(k.shape))
    step = max(1, int(budget_bytes) // (4 * int(H) * int(W)))
    counts = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device)
    for b in range(0, w2c.shape[0], step):
        kb = k if k.shape[0] == 1 else k[b:b + step]
        depth = mesh_depth(mesh, w2c[b:b + step], kb, H, W, znear, zfar)
        view_counts(verts, depth, w2c[b:b + step], kb, eps, counts)
        del depth
    inside = ((tris >= 0) & (tris < verts.shape[0])).all(dim=1)
    kept, t, cols = _e.compact_kept(verts, tris[inside], counts >= int(min_views), getattr(mesh, "vertex_colors", None))
    out = TriangleMesh(kept, t, cols)
    return (out, counts) if return_counts else out


# ------------------------------------------------------------------------------------------------ trajectories (host)
def rotation_between(a, b):
    """help_func.py:5-30 (rotation_matrix) in fp32 on the host: the rotation that turns a onto b.  Where the reference draws random noise
    (a and b exactly opposite) this raises."""
    a = torch.as_tensor(a, dtype=torch.float32)
    b = torch.as_tensor(b, dtype=torch.float32)
    a = a / torch.linalg.norm(a)
    b = b / torch.linalg.norm(b)
    v = torch.linalg.cross(a, b)
    c = torch.dot(a, b)
    # (the reference compares in fp32, where -1 + 1e-8 is -1: its noise branch runs for a rounded dot product below -1 only, and a dot
    # product of exactly -1 returns the identity, which rotates nothing; both raise here)
    if float(c) < -1 + 1e-8:
        raise ValueError("surfel_cull: the mean up vector is exactly opposite to +z; the reference perturbs it with random noise, which has no "
                         "reproducible result")
    s = torch.linalg.norm(v)
    k = torch.tensor([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=torch.float32)
    return torch.eye(3) + k + k @ k * ((1 - c) / (s ** 2 + 1e-8))


def orient_and_center(poses):
    """help_func.py:33-88 (auto_orient_and_center_poses(method='up', center_poses=True)) in fp32 on the host: [N, 4, 4] -> [N, 3, 4] with
    the mean up vector (column 1) turned onto +z and the mean position moved to the origin."""
    poses = torch.as_tensor(np.asarray(poses, np.float32))
    translation = torch.mean(poses[..., :3, 3], dim=0)
    up = torch.mean(poses[:, :3, 1], dim=0)
    up = up / torch.linalg.norm(up)
    rot = rotation_between(up, torch.tensor([0.0, 0.0, 1.0]))
    transform = torch.cat([rot, rot @ -translation[..., None]], dim=-1)
    return transform @ poses


def read_trajectory(path):
    """Camera-to-world poses [N, 4, 4] (float32) as cull_mesh.py:321-363 (get_traj) reads them: a .npy stack of (3, 4) or (4, 4) poses, or
    a transforms .json (instant-ngp / sdfstudio): frame k is the one whose file_path[13:18] reads k + 1; the poses are oriented and
    centred (orient_and_center) and scaled by 1 / max |t|."""
    if path.endswith(".npy"):
        p = np.asarray(np.load(path), np.float32)
    elif path.endswith(".json"):
        with open(path, encoding="UTF-8") as f:
            meta = json.load(f)
        by_index = {int(fr["file_path"][13:18]) - 1: np.array(fr["transform_matrix"]) for fr in meta["frames"]}
        poses = orient_and_center(np.array([by_index[i] for i in range(len(by_index))]).astype(np.float32))
        poses[:, :3, 3] *= 1.0 / float(torch.max(torch.abs(poses[:, :3, 3])))
        p = poses.numpy()
    else:
        raise ValueError("surfel_cull: a trajectory is a .npy pose stack or a transforms .json, got %r" % (path,))
    if p.ndim != 3 or p.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("surfel_cull: poses must be [N, 3 | 4, 4], got %s" % list(p.shape))
    if p.shape[1] == 3:
        p = np.concatenate([p, np.broadcast_to(np.array([[[0, 0, 0, 1]]], np.float32), (len(p), 1, 4))], 1)
    return np.ascontiguousarray(p, np.float32)


def read_model_cameras(model_dir):
    """The cameras of MODEL_DIR/cameras.json (utils/camera_utils.py:64-84 writes it) as OpenCV camera-to-world poses with their own
    intrinsics and sizes: [(c2w [4, 4], (fx, fy, cx, cy), H, W)], cx = (W - 1) / 2 and cy = (H - 1) / 2 as in surfel_mesh.camera_intrinsics."""
    with open(os.path.join(model_dir, "cameras.json")) as f:
        entries = json.load(f)
    out = []
    for e in entries:
        c2w = np.eye(4, dtype=np.float32)
        c2w[:3, :3], c2w[:3, 3] = np.asarray(e["rotation"], np.float32), np.asarray(e["position"], np.float32)
        Wd, Ht = int(e["width"]), int(e["height"])
        out.append((c2w, (float(e["fx"]), float(e["fy"]), (Wd - 1) / 2.0, (Ht - 1) / 2.0), Ht, Wd))
    return out


def cull_mesh_cameras(mesh, cameras, min_views=MIN_VIEWS, eps=EPS, znear=ZNEAR, zfar=ZFAR, budget_bytes=DEFAULT_BUDGET):
    """cull_mesh_views for OpenCV cameras that differ in size (read_model_cameras): views of one size share their batches."""
    verts = _points(mesh.vertices, "mesh.vertices")
    tris = _dev(mesh.triangles, "mesh.triangles").detach().to(torch.int64)
    counts = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device)
    sizes = sorted({(h, w) for _, _, h, w in cameras})
    for h, w in sizes:
        group = [c for c in cameras if (c[2], c[3]) == (h, w)]
        w2c = world_to_camera(np.stack([c[0] for c in group]), "opencv")
        k = np.asarray([c[1] for c in group], np.float32)
        step = max(1, int(budget_bytes) // (4 * h * w))
        for b in range(0, len(group), step):
            depth = mesh_depth(mesh, w2c[b:b + step], k[b:b + step], h, w, znear, zfar)
            view_counts(verts, depth, w2c[b:b + step], k[b:b + step], eps, counts)
            del depth
    inside = ((tris >= 0) & (tris < verts.shape[0])).all(dim=1)
    return TriangleMesh(*_e.compact_kept(verts, tris[inside], counts >= int(min_views), getattr(mesh, "vertex_colors", None)))


def main(argv=None):
    import surfel_io
    ap = argparse.ArgumentParser(description="Cull a mesh to what the cameras saw (the reference's scripts/eval_tnt/cull_mesh.py)")
    ap.add_argument("--traj-path", type=str, default=None, help="trajectory: a .npy pose stack or a transforms .json")
    ap.add_argument("-m", "--model_path", type=str, default=None, help="instead of --traj-path: the OpenCV cameras of MODEL_DIR/cameras.json, "
                    "with their own intrinsics and sizes")
    ap.add_argument("--ply-path", type=str, required=True, help="mesh to cull; MESH.ply -> MESH_cull.ply")
    ap.add_argument("--height", type=int, default=TNT_H)
    ap.add_argument("--width", type=int, default=TNT_W)
    ap.add_argument("--fx", type=float, default=TNT_INTRINSICS[0])
    ap.add_argument("--fy", type=float, default=TNT_INTRINSICS[1])
    ap.add_argument("--cx", type=float, default=TNT_INTRINSICS[2])
    ap.add_argument("--cy", type=float, default=TNT_INTRINSICS[3])
    ap.add_argument("--near", type=float, default=ZNEAR)
    ap.add_argument("--far", type=float, default=ZFAR)
    ap.add_argument("--min_views", type=int, default=MIN_VIEWS)
    ap.add_argument("--eps", type=float, default=EPS)
    ap.add_argument("--convention", type=str, default="opengl", choices=["opengl", "opencv"], help="axes of the trajectory's poses")
    args = ap.parse_args(argv)
    if (args.traj_path is None) == (args.model_path is None):
        raise SystemExit("give --traj-path or -m MODEL_DIR")
    dev = torch.device("cuda:0")
    mesh = read_mesh(args.ply_path, dev)
    if args.model_path is not None:
        cams = read_model_cameras(args.model_path)
        out = cull_mesh_cameras(mesh, cams, args.min_views, args.eps, args.near, args.far)
        views = len(cams)
    else:
        poses = read_trajectory(args.traj_path)
        out = cull_mesh_views(mesh, poses, (args.fx, args.fy, args.cx, args.cy), args.height, args.width, args.convention, args.min_views, args.eps,
                              args.near, args.far)
        views = len(poses)
    stem = surfel_io.ply_stem(args.ply_path)
    surfel_io.write_triangle_mesh(stem + "_cull.ply", out)
    print("%d views: kept %d of %d vertices, %d of %d triangles -> %s" % (views, out.vertices.shape[0], mesh.vertices.shape[0], out.triangles.shape[0],
                                                                        mesh.triangles.shape[0], stem + "_cull.ply"))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
