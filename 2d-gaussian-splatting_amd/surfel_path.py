"""Camera trajectories on MI355X — the reference's `--render_path` mode (render.py:73-84): the elliptical fly-through of
utils/render_utils.py:28-194 and the colour / depth / normal frame sequences its `create_videos` (:203-268) feeds to the video
encoder.  RENDER.md states the rules.

The path generator is host code (fp64 numpy, a few hundred 4x4 matrices).  The frames never leave the device as fp32: the
conversion to 8 bits (surfel_vis_quantize), the depth limits (surfel_vis_order_stats) and the turbo depth frame
(surfel_vis_depth_turbo) are HIP kernels of libsurfel_hip.so (include/surfel_vis.h); the finished bytes go to pinned host buffers by
non-blocking copies and are encoded by worker threads while the renderer runs ahead (FrameWriter).
"""
import copy
import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

import surfel_frames as _f
import surfel_native as _n

_n.load()

MAX_WORKERS = 8      # the scene loader's ceiling for its decoding threads (surfel_scene.py)


# ------------------------------------------------------------------------------------------------ the path (host, fp64)
def _unit(x):
    return x / np.linalg.norm(x)


def pad_poses(p):
    """[..., 3, 4] -> [..., 4, 4]: the homogeneous bottom row (0, 0, 0, 1) appended."""
    p = np.asarray(p)
    bottom = np.broadcast_to([0, 0, 0, 1.0], p[..., :1, :4].shape)
    return np.concatenate([p[..., :3, :4], bottom], axis=-2)


def viewmatrix(lookdir, up, position):
    """Look-at camera-to-world [3, 4]: columns x = up x z, y = z x x, z = lookdir (all unit), position."""
    z = _unit(lookdir)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    return np.stack([x, y, z, position], axis=1)


def focus_point_fn(poses):
    """The point nearest (least squares) to every camera's z axis; poses [N, 3, 4]."""
    d, o = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - d * np.transpose(d, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ o).mean(0)[:, 0]


def transform_poses_pca(poses):
    """(poses_recentered [N,3,4], transform [4,4]): the camera positions' mean moved to the origin and their principal axes onto x, y, z
    (largest spread first).  np.linalg.eig on t.T @ t and a descending argsort, as the reference calls them: the eigenvectors' signs
    are whatever LAPACK returns, and the two rules that follow (det < 0 flips z; a mean pose whose y axis points down flips y and z)
    depend on them."""
    t = poses[:, :3, 3]
    t_mean = t.mean(axis=0)
    t = t - t_mean
    eigval, eigvec = np.linalg.eig(t.T @ t)
    rot = eigvec[:, np.argsort(eigval)[::-1]].T
    if np.linalg.det(rot) < 0:
        rot = np.diag(np.array([1, 1, -1])) @ rot
    transform = np.concatenate([rot, rot @ -t_mean[:, None]], -1)
    recentered = (transform @ pad_poses(poses))[..., :3, :4]
    transform = np.concatenate([transform, np.eye(4)[3:]], axis=0)
    if recentered.mean(axis=0)[2, 1] < 0:
        recentered = np.diag(np.array([1, -1, -1])) @ recentered
        transform = np.diag(np.array([1, -1, -1, 1])) @ transform
    return recentered, transform


def generate_ellipse_path(poses, n_frames=120):
    """[n_frames, 3, 4] look-at poses on the ellipse in the z = 0 plane that is centred on the focus point's (x, y) and whose half
    axes are the 90th percentiles of the cameras' |position - centre|; n_frames + 1 angles from 0 to 2 pi, the duplicated last one
    dropped; every pose looks along (position - focus point) with the up vector snapped to the axis nearest the mean camera y axis.
    (The reference's z_variation is 0 in the only call it makes, so the height term is left out.)"""
    center = focus_point_fn(poses)
    offset = np.array([center[0], center[1], 0])
    sc = np.percentile(np.abs(poses[:, :3, 3] - offset), 90, axis=0)
    low, high = -sc + offset, sc + offset
    theta = np.linspace(0, 2.0 * np.pi, n_frames + 1, endpoint=True)
    positions = np.stack([low[0] + (high - low)[0] * (np.cos(theta) * 0.5 + 0.5),
                          low[1] + (high - low)[1] * (np.sin(theta) * 0.5 + 0.5),
                          np.zeros_like(theta)], -1)[:-1]
    avg_up = _unit(poses[:, :3, 1].mean(0))
    ind_up = np.argmax(np.abs(avg_up))
    up = np.eye(3)[ind_up] * np.sign(avg_up[ind_up])
    return np.stack([viewmatrix(p - center, up, p) for p in positions])


_FLIP = np.diag([1.0, -1.0, -1.0, 1.0])      # COLMAP (y down, z forward) <-> OpenGL (y up, z back) camera axes


def path_matrices(world_view_transforms, n_frames=240):
    """world_view_transform (row-vector convention, fp64 [n_frames, 4, 4]) of every path camera, from the training cameras'."""
    c2ws = np.array([np.linalg.inv(np.asarray(w).T) for w in world_view_transforms])
    pose = c2ws[:, :3, :] @ _FLIP
    recentered, transform = transform_poses_pca(pose)
    new_poses = np.linalg.inv(transform) @ pad_poses(generate_ellipse_path(recentered, n_frames=n_frames))
    return np.stack([np.linalg.inv(c2w @ _FLIP).T for c2w in new_poses])


def generate_path(cameras, n_frames=240):
    """utils/render_utils.py:173-194: n_frames copies of cameras[0] (shallow: the photograph is shared, not copied 240 times) with the
    size rounded down to even (what h264 needs), world_view_transform of the elliptical path as fp32, and full_proj_transform and
    camera_center recomputed from it in fp32."""
    first = cameras[0]
    dev = first.world_view_transform.device
    wvts = path_matrices([cam.world_view_transform.detach().cpu().numpy() for cam in cameras], n_frames)
    proj = first.projection_matrix.detach().cpu().float()
    traj = []
    for w in wvts:
        cam = copy.copy(first)
        cam.image_height = int(first.image_height / 2) * 2
        cam.image_width = int(first.image_width / 2) * 2
        wvt = torch.from_numpy(w).float()
        cam.world_view_transform = wvt.to(dev)
        cam.full_proj_transform = (wvt @ proj).to(dev)
        cam.camera_center = torch.linalg.inv(wvt)[3, :3].contiguous().to(dev)
        for cached in ("_post", "_surfel_post_consts"):      # per-camera constants derived from the matrices (surfel_render)
            if hasattr(cam, cached):
                setattr(cam, cached, None)
        traj.append(cam)
    return traj


# ------------------------------------------------------------------------------------------------ frame kernels
def _planes(img):
    return _n.device_tensor("surfel_path", img).detach().float().contiguous()


def quantize_u8(img, scale=1.0, bias=0.0, out=None):
    """[C, H, W] (or [H, W]) fp32 on the device -> [H, W, C] uint8 as save_img_u8 quantises img * scale + bias (surfel_vis_quantize).
    out: a uint8 tensor of H * W * C elements to write into (any byte alignment)."""
    p = _planes(img)
    if p.dim() == 2:
        p = p[None]
    Cn, H, W = (int(s) for s in p.shape)
    out = _n.uint8_buffer("quantize_u8", out, H * W * Cn, p.device)
    _n.call(p.device, "surfel_vis_quantize", Cn, H, W, p, float(scale), float(bias), out)
    return out.view(H, W, Cn)


_ORDER_SCRATCH = 8448      # SURFEL_VIS_ORDER_SCRATCH_BYTES


def order_stats(x, ranks):
    """float32 tensor [len(ranks)] on the device: the ranks[j]-th smallest elements of x in numpy's sort order (surfel_vis_order_stats).
    ranks ascending, at most 8.  No host synchronisation."""
    v = _planes(x).reshape(-1)
    m = len(ranks)
    out = torch.empty(m, dtype=torch.float32, device=v.device)
    scratch = torch.empty(_ORDER_SCRATCH, dtype=torch.uint8, device=v.device)
    _n.call(v.device, "surfel_vis_order_stats", v.numel(), v, m, (C.c_int64 * m)(*[int(r) for r in ranks]), out, scratch, _ORDER_SCRATCH)
    return out


def percentile_ranks(n, q):
    """(ranks, previous, next, gamma) of np.percentile's linear method on n values: virtual index (n - 1) * (q / 100), its two
    neighbouring order statistics and the weight of the upper one; ranks = their sorted union plus n - 1 (where a NaN would sort)."""
    vi = (n - 1) * np.true_divide(np.asarray(q, np.float64).reshape(-1), 100)
    prev = np.floor(vi).astype(np.intp)
    nxt = prev + 1
    above, below = vi >= n - 1, vi < 0
    prev[above] = nxt[above] = n - 1
    prev[below] = nxt[below] = 0
    ranks = sorted(set(prev.tolist()) | set(nxt.tolist()) | {n - 1})
    return ranks, prev, nxt, vi - prev


def lerp_percentiles(values, ranks, prev, nxt, gamma):
    """np.percentile's interpolation (numpy's _lerp, both of its sides) on the selected order statistics: b - a in the data's own
    precision, the rest in fp64; NaN when the largest element is NaN, as np.percentile answers then."""
    values = np.asarray(values, np.float32)
    at = dict(zip(ranks, values))
    a, b = np.array([at[int(k)] for k in prev], np.float32), np.array([at[int(k)] for k in nxt], np.float32)
    with np.errstate(invalid="ignore"):
        diff = np.subtract(b, a)
        out = np.asanyarray(np.add(a, diff * gamma))
        np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5, casting="unsafe", dtype=type(out.dtype))
    if np.isnan(values[-1]):
        out[...] = np.nan
    return out


def percentiles(x, q):
    """np.percentile(x, q) (float64 [len(q)], at most 3 percentiles) of a device tensor: exact selection on the device, numpy's
    linear interpolation in fp64 on the host (one small device-to-host copy)."""
    n = int(x.numel())
    ranks, prev, nxt, gamma = percentile_ranks(n, q)
    return lerp_percentiles(order_stats(x, ranks).cpu().numpy(), ranks, prev, nxt, gamma)


def depth_limits(depth, p=3):
    """(lo, hi) = log of the p-th and (100 - p)-th percentile of a depth frame, float64, as create_videos takes them from frame 0.
    lo is -inf when more than p % of the frame is empty (depth 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, hi = np.log(percentiles(depth, [p, 100 - p]))
    return float(lo), float(hi)


def colorize_depth(depth, lo, hi, out=None):
    """[H, W] (or [1, H, W]) fp32 depth on the device -> [H, W, 3] uint8 turbo frame (surfel_vis_depth_turbo)."""
    d = _planes(depth)
    H, W = (int(s) for s in d.shape[-2:])
    if d.numel() != H * W:
        raise ValueError("colorize_depth: one depth plane expected, got %s" % (tuple(d.shape),))
    out = _n.uint8_buffer("colorize_depth", out, H * W * 3, d.device)
    _n.call(d.device, "surfel_vis_depth_turbo", H, W, d, float(lo), float(hi), out)
    return out.view(H, W, 3)


# ------------------------------------------------------------------------------------------------ the streamed exporter
class FrameWriter:
    """Writes frames to disk behind the renderer.  submit(path, tensor) takes uint8 [H, W, C] (C = 1 or 3 -> PNG) or float32 [H, W]
    (-> float32 TIFF with save_img_f32's values: NaN -> 0, +-inf -> +-FLT_MAX) on the device or the host, copies it into one of `ring`
    pinned host buffers without blocking, records an event behind the copy and hands the buffer to a pool of `workers` threads
    (at most 8) that wait for the event and encode with Pillow.  submit blocks only when all buffers are in flight: no more than
    `ring` frames are ever retained.  close() waits for everything and re-raises the first exception a worker met.
    png="device": a uint8 frame on the device is encoded there (surfel_png.encode_png, PNG.md) into one of `ring` device buffers and its
    size word copied to pinned memory without blocking; the worker waits for the event, reads the size, copies exactly that many bytes
    into the slot's pinned buffer on a side stream and writes them: only the compressed bytes cross.  Host tensors and the TIFFs stay
    on Pillow.  png="pillow" (the default): every PNG through Pillow, as before."""

    def __init__(self, workers=4, ring=None, png="pillow"):
        if png not in ("pillow", "device"):
            raise ValueError("FrameWriter: png must be 'pillow' or 'device', got %r" % (png,))
        self.png = png
        self._device = None                     # png="device": surfel_frames.EncodedStream, made by the first device PNG
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.ring = max(1, int(ring)) if ring is not None else 2 * self.workers
        self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="frame-writer")
        self._ring = _f.SlotRing(self.ring)
        self._idle = self._ring._idle           # (the ring's own list, under the name it had here)
        self._buffers = [None] * self.ring      # uint8 host tensors of the Pillow path, grown on demand
        self._futures = []
        self.frames = 0

    wait_s = property(lambda self: self._ring.wait_s, doc="time submit() spent waiting for a free buffer (encoders behind the renderer)")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self._drain()
        return False

    def _buffer(self, slot, nbytes, pinned):
        buf = self._buffers[slot]
        if buf is None or buf.numel() < nbytes or buf.is_pinned() != pinned:
            buf = self._buffers[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=pinned)
        return buf[:nbytes]

    def submit(self, path, tensor):
        t = tensor.detach()
        if t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] in (1, 3):
            kind = "PNG"
        elif t.dtype == torch.float32 and t.dim() == 2:
            kind = "TIFF"
        else:
            raise ValueError("FrameWriter.submit: uint8 [H, W, 1 or 3] or float32 [H, W] expected, got %s %s" % (t.dtype, tuple(t.shape)))
        if self._pool is None:
            raise RuntimeError("FrameWriter.submit after close()")
        slot = self._ring.acquire()
        try:
            t = t.contiguous()
            if kind == "PNG" and self.png == "device" and t.is_cuda:
                event = self._encode_device(slot, t)
                self.frames += 1
                self._futures.append(self._pool.submit(self._write_device, slot, path, event))
                return
            host = self._buffer(slot, t.numel() * t.element_size(), t.is_cuda).view(t.dtype).view(t.shape)
            event = None
            if t.is_cuda:
                with torch.cuda.device(t.device):
                    host.copy_(t, non_blocking=True)
                    event = torch.cuda.Event()
                    event.record()
            else:
                host.copy_(t)
        except BaseException:
            self._ring.release(slot)
            raise
        self.frames += 1
        self._futures.append(self._pool.submit(self._encode, slot, path, kind, host, event))

    def _encode_device(self, slot, t):
        """the PNG file of a device frame into the slot's device buffer, its size into pinned memory; the event behind both"""
        import surfel_png
        if self._device is None:
            self._device = _f.EncodedStream(t.device, self.ring)
        elif self._device.device != t.device:
            raise ValueError("FrameWriter(png='device'): frames of one writer must live on one device (%s, then %s)" % (self._device.device, t.device))
        return self._device.encode(slot, surfel_png.capacity(*t.shape), lambda out, size: surfel_png.encode_png(t, out=out, size=size))

    def _write_device(self, slot, path, event):
        try:
            self._store(path, self._device.fetch(slot, event))
        except BaseException as e:
            self._ring.park(e)
        finally:
            self._ring.release(slot)

    def _store(self, path, data):
        with open(path, "wb") as f:
            f.write(data)

    def _encode(self, slot, path, kind, host, event):
        try:
            from PIL import Image
            if event is not None:
                event.synchronize()
            a = host.numpy()
            if kind == "PNG":
                img = Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)
            else:
                img = Image.fromarray(np.nan_to_num(a).astype(np.float32))
            with open(path, "wb") as f:
                img.save(f, kind)
        except BaseException as e:
            self._ring.park(e)
        finally:
            self._ring.release(slot)

    def _drain(self):
        pool, self._pool = self._pool, None
        if pool is not None:
            for f in self._futures:
                f.result()
            pool.shutdown(wait=True)
        self._futures = []

    def close(self):
        self._drain()
        self._ring.reraise()


def _folders(out_dir, names):
    paths = [os.path.join(out_dir, *n.split("/")) for n in names]
    for p in paths:
        os.makedirs(p, exist_ok=True)
    return paths


@torch.no_grad()
def render_path(gaussians, cameras, render, pipe, background, out_dir, n_frames=240, vis_normals=False, workers=4, timings=None,
                video=False, video_only=False, video_quality=95, fps=60, png="pillow"):
    """render.py:73-84: the elliptical path through `cameras`, rendered frame by frame and written as
    out_dir/renders/%05d.png (colour), vis/depth_%05d.tiff (surf_depth, float32), video/depth/%05d.png (the depth video's frames:
    turbo of log depth between the 3rd and 97th percentile of frame 0) and, with vis_normals, vis/normal_%05d.png (rend_normal * 0.5 +
    0.5).  Frames are converted on the device and handed to a FrameWriter: the one host wait of the loop is frame 0's depth limits.
    video: also out_dir/render_traj_color.avi, render_traj_depth.avi and, with vis_normals, render_traj_normal.avi (Motion-JPEG at
    video_quality and fps, VIDEO.md), fed from the very tensors that go to renders/, video/depth/ and vis/normal_*: create_videos'
    three videos, frame for frame, encoded on the device.  video_only: the videos and none of the per-frame files or folders.
    png: "pillow" (the default) or "device": the PNG frames encoded on the device (FrameWriter(png=...), PNG.md); same names, same pixels.
    timings: a dict that receives the loop's host time and the writers' counters.  Returns the path cameras."""
    traj = generate_path(cameras, n_frames=n_frames)
    video = video or video_only
    if video_only:
        os.makedirs(out_dir, exist_ok=True)
        renders = vis = depth_dir = None
    else:
        renders, vis, depth_dir = _folders(out_dir, ["renders", "vis", "video/depth"])
    lo = hi = None
    writers = {}
    fw = None if video_only else FrameWriter(workers=workers, png=png)      # (video_only: no encoder threads, no pinned ring)

    def emit(name, frame, folder, pattern, idx):
        if fw is not None:
            fw.submit(os.path.join(folder, pattern % idx), frame)
        if video:
            if name not in writers:
                import surfel_video
                writers[name] = surfel_video.VideoWriter(os.path.join(out_dir, "render_traj_%s.avi" % name), frame.shape[0], frame.shape[1],
                                                         fps=fps, quality=video_quality)
            writers[name].add_frame(frame)

    def finish_videos():
        """every video gets its index and headers; the first error any writer met"""
        first = None
        for w in writers.values():
            try:
                w.close()
            except BaseException as e:
                first = first or e
        return first

    t0 = time.perf_counter()
    try:
        for idx, cam in enumerate(traj):
            pkg = render(cam, gaussians, pipe, background)
            depth = pkg["surf_depth"][0]
            if idx == 0:
                lo, hi = depth_limits(depth)
            emit("color", quantize_u8(pkg["render"]), renders, "%05d.png", idx)
            if fw is not None:
                fw.submit(os.path.join(vis, "depth_%05d.tiff" % idx), depth)
            emit("depth", colorize_depth(depth, lo, hi), depth_dir, "%05d.png", idx)
            if vis_normals:
                emit("normal", quantize_u8(pkg["rend_normal"], 0.5, 0.5), vis, "normal_%05d.png", idx)
        if timings is not None:      # (the time close() then waits for the encoders is the caller's total minus loop_ms)
            timings.update(loop_ms=(time.perf_counter() - t0) * 1e3, submit_wait_ms=fw.wait_s * 1e3 if fw else 0.0, files=fw.frames if fw else 0,
                           depth_limits=(lo, hi))
            if video:
                timings.update(video_wait_ms=sum(w.wait_s for w in writers.values()) * 1e3, videos=sorted(writers))
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
