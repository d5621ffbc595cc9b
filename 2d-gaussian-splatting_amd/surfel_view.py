"""The live viewer on MI355X — the reference's gaussian_renderer/network_gui.py (the SIBR remote viewer's wire protocol), the serve
loop of train.py:146-168, view.py, MiniCam (scene/cameras.py:61-72) and utils/image_utils.py:23-61 (gradient_map, colormap,
render_net_image).  VIEWER.md states the rules and the departures.

A displayed frame is one render under no_grad, net_image() — at most three HIP launches of libsurfel_hip.so (include/surfel_view.h,
include/surfel_vis.h) that turn the render package into the interleaved bytes of the chosen mode, lo / hi of the colour-mapped modes
never leaving the device — one non-blocking copy into a pinned buffer that is reused from frame to frame, one event wait, and the
socket.  The protocol is host code.

    python surfel_view.py -m MODEL [-s CAPTURE] [--iteration N] [--ip 127.0.0.1] [--port 6009] [--mesh MESH.ply | MESH.obj]
"""
import json
import os
import socket
import struct
import time

import torch

import surfel_frames as _f
import surfel_native as _n
import surfel_path as _sp

_n.load()

RENDER_ITEMS = ["RGB", "Alpha", "Normal", "Depth", "Edge", "Curvature"]      # arguments/__init__.py:57, the order the viewer's menu indexes
MESH_ITEMS = {"Mesh": "shaded", "Mesh Normal": "normal"}      # appended to the menu of a Viewer that was given a mesh (MESHVIEW.md)
TEXTURE_ITEMS = {"Mesh Textured": "textured"}                 # and behind them for a mesh that came with a texture (TEXTURE.md)
DEFAULT_TIMEOUT = 5.0      # seconds a connected viewer may stay silent (or not read) before it is dropped


class MiniCam:
    """scene/cameras.py:61-72: what the renderer reads of a camera, from the viewer's matrices (row-vector convention).  The 4 x 4
    inverse behind camera_center is taken on the host (as Camera does) and lands on the matrices' device."""

    def __init__(self, width, height, fovy, fovx, znear, zfar, world_view_transform, full_proj_transform):
        self.image_width = width
        self.image_height = height
        self.FoVy = fovy
        self.FoVx = fovx
        self.znear = znear
        self.zfar = zfar
        self.world_view_transform = world_view_transform
        self.full_proj_transform = full_proj_transform
        view_inv = torch.inverse(world_view_transform.detach().cpu())
        self.camera_center = view_inv[3][:3].contiguous().to(world_view_transform.device)


# ------------------------------------------------------------------------------------------------ render package -> bytes
def scratch_bytes(H, W):
    """SURFEL_VIEW_SCRATCH_BYTES(H, W) of include/surfel_view.h"""
    return 64 + 4 * int(H) * int(W)


def _mode_name(mode):
    if isinstance(mode, str):
        for item in RENDER_ITEMS:
            if item.lower() == mode.lower():
                return item
        raise KeyError("net_image: no render mode %r (%s)" % (mode, ", ".join(RENDER_ITEMS)))
    return RENDER_ITEMS[mode]      # (an index off the list raises, as the reference's render_items[render_mode] does)


def net_image(render_pkg, mode, out=None):
    """uint8 [H, W, 3] on the device: the bytes the viewer draws for `mode` (an index into RENDER_ITEMS, or a name) of a render
    package — render_net_image + clamp * 255 + byte + permute of the reference.  RGB and Normal are surfel_vis_quantize; Alpha and
    Depth surfel_view_scalar; Edge and Curvature surfel_view_gradient.  out: a contiguous uint8 tensor of H * W * 3 elements to write
    into.  No host synchronisation."""
    name = _mode_name(mode)
    if name == "RGB":
        return _sp.quantize_u8(render_pkg["render"], 1.0, 0.0, out=out)
    if name == "Normal":
        return _sp.quantize_u8(render_pkg["rend_normal"], 0.5, 0.5, out=out)
    src = _sp._planes(render_pkg[{"Alpha": "rend_alpha", "Depth": "surf_depth", "Edge": "render", "Curvature": "rend_normal"}[name]])
    H, W = (int(s) for s in src.shape[-2:])
    planes = 3 if name in ("Edge", "Curvature") else 1
    if src.numel() != planes * H * W:
        raise ValueError("net_image: %s needs %d plane(s), got %s" % (name, planes, tuple(src.shape)))
    out = _n.uint8_buffer("net_image", out, H * W * 3, src.device)
    nbytes = scratch_bytes(H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    if planes == 1:
        _n.call(src.device, "surfel_view_scalar", H, W, src, out, scratch, nbytes)
    else:
        scale, bias = (1.0, 0.0) if name == "Edge" else (0.5, 0.5)
        _n.call(src.device, "surfel_view_gradient", H, W, src, scale, bias, out, scratch, nbytes)
    return out.view(H, W, 3)


# ------------------------------------------------------------------------------------------------ the wire protocol
class Connection:
    """network_gui.py's send_json_data / read / send / receive over an already connected socket object, byte for byte, with two
    hardenings: a read loops until the announced length has arrived (the reference trusts one recv), and the socket has a timeout, so
    a viewer that stalls raises socket.timeout here instead of holding the training."""

    def __init__(self, sock, timeout=DEFAULT_TIMEOUT, device="cuda"):
        self.sock = sock
        self.device = torch.device(device)
        sock.settimeout(timeout)

    def close(self):
        try:
            self.sock.close()
        except OSError:
            pass

    def _read(self, n):
        buf = bytearray()
        while len(buf) < n:
            piece = self.sock.recv(n - len(buf))
            if not piece:
                raise ConnectionError("viewer closed the connection (%d of %d bytes)" % (len(buf), n))
            buf += piece
        return bytes(buf)

    def _send_json(self, data):
        body = json.dumps(data).encode("utf-8")
        self.sock.sendall(struct.pack("<I", len(body)))
        self.sock.sendall(body)

    def send_items(self, items=RENDER_ITEMS):
        """what try_connect sends once after accept: the mode names of the viewer's menu"""
        self._send_json(list(items))

    def read(self):
        length = int.from_bytes(self._read(4), "little")
        return json.loads(self._read(length).decode("utf-8"))

    def receive(self):
        """(MiniCam, do_training, keep_alive, scaling_modifier, render_mode) of the viewer's next message; five Nones when it asks for
        an empty image.  Columns 1 and 2 of view_matrix and column 1 of view_projection_matrix change sign (the viewer's axes)."""
        message = self.read()
        width, height = message["resolution_x"], message["resolution_y"]
        if width == 0 or height == 0:
            return None, None, None, None, None
        do_training = bool(message["train"])
        keep_alive = bool(message["keep_alive"])
        world_view_transform = torch.reshape(torch.tensor(message["view_matrix"]), (4, 4))
        world_view_transform[:, 1] = -world_view_transform[:, 1]
        world_view_transform[:, 2] = -world_view_transform[:, 2]
        full_proj_transform = torch.reshape(torch.tensor(message["view_projection_matrix"]), (4, 4))
        full_proj_transform[:, 1] = -full_proj_transform[:, 1]
        cam = MiniCam(width, height, message["fov_y"], message["fov_x"], message["z_near"], message["z_far"],
                      world_view_transform.to(self.device), full_proj_transform.to(self.device))
        return cam, do_training, keep_alive, message["scaling_modifier"], message["render_mode"]

    def send(self, image_bytes, verify, metrics):
        """the frame (W * H * 3 bytes; None: no image), the length-prefixed ASCII `verify` string (the capture's path), the metrics as JSON"""
        if image_bytes is not None:
            self.sock.sendall(image_bytes)
        self.sock.sendall(len(verify).to_bytes(4, "little"))
        self.sock.sendall(bytes(verify, "ascii"))
        self._send_json(metrics)


# ------------------------------------------------------------------------------------------------ the serve loop
def open_listener(host, port):
    """A non-blocking listening socket on (host, port): accept() raises at once when no viewer is waiting."""
    listener = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    listener.bind((host, port))
    listener.listen()
    listener.settimeout(0)
    return listener


class Viewer:
    """The listener (None for a Viewer attached to a socket that is connected already) and the one connection.  serve() is what a
    training loop calls after every step, and what the stand-alone viewer calls forever."""

    def __init__(self, host="127.0.0.1", port=6009, timeout=DEFAULT_TIMEOUT, device="cuda", items=RENDER_ITEMS, listener=True, mesh=None, texture=None):
        self.timeout, self.device, self.items = timeout, device, list(items)
        self.mesh, self._mesh_normals = mesh, None      # a surfel_mesh.TriangleMesh on the device: two more items, served by surfel_meshview
        self.texture = texture                          # a surfel_texture.TexturedMesh of that mesh: one more item
        self._mesh_items = dict(MESH_ITEMS, **TEXTURE_ITEMS) if texture is not None else dict(MESH_ITEMS)
        if mesh is not None:
            self.items += list(self._mesh_items)
        self.listener = open_listener(host, port) if listener else None
        self.conn = None
        self.frames = 0
        self._pinned = None

    @classmethod
    def attached(cls, sock, timeout=DEFAULT_TIMEOUT, device="cuda", items=RENDER_ITEMS, mesh=None, texture=None):
        """A Viewer on a connected socket object (one end of a socketpair, an accepted connection): no listener, nothing is bound."""
        v = cls(timeout=timeout, device=device, items=items, listener=False, mesh=mesh, texture=texture)
        v._adopt(sock)
        return v

    def _adopt(self, sock):
        conn = Connection(sock, self.timeout, self.device)
        try:
            conn.send_items(self.items)
        except Exception:
            conn.close()
            return
        self.conn = conn

    def try_connect(self):
        if self.listener is None:
            return
        try:
            sock, _ = self.listener.accept()
        except OSError:      # nobody is waiting (BlockingIOError), or the listener is gone
            return
        self._adopt(sock)

    def drop(self):
        if self.conn is not None:
            self.conn.close()
            self.conn = None

    def close(self):
        self.drop()
        if self.listener is not None:
            self.listener.close()
            self.listener = None

    def _to_host(self, image):
        """The bytes of a device image in the pinned buffer: a non-blocking copy and a wait for the event behind it."""
        self._pinned, view = _f.to_pinned(image.reshape(-1), self._pinned)
        return view

    def _mesh_mode(self, render_mode):
        """the surfel_meshview mode of a menu entry that shows the mesh (an index into this viewer's items, or a name); None for the others"""
        if self.mesh is None:
            return None
        if isinstance(render_mode, str):
            return next((m for name, m in self._mesh_items.items() if name.lower() == render_mode.lower()), None)
        first = len(self.items) - len(self._mesh_items)      # (the mesh items are the last ones of the menu)
        return self._mesh_items[self.items[render_mode]] if first <= render_mode < len(self.items) else None

    def _mesh_image(self, cam, mode):
        """uint8 [H, W, 3] on the device: the mesh for the viewer's camera, one sample per pixel, on white (surfel_meshview.render_mesh)"""
        import surfel_meshview
        if mode == "textured":
            return surfel_meshview.render_mesh(self.mesh, [cam], mode=mode, ssaa=1, texture=self.texture)[0]
        if self._mesh_normals is None:
            self._mesh_normals = surfel_meshview.vertex_normals(self.mesh)
        return surfel_meshview.render_mesh(self.mesh, [cam], mode=mode, ssaa=1, normals=self._mesh_normals)[0]

    @torch.no_grad()
    def serve(self, gaussians, pipe, background, source_path="", metrics_fn=None, iteration=0, iterations=0):
        """train.py:146-168.  Without a connection: one accept attempt, and back.  With one: answer the viewer's messages — render its
        camera in its mode, send the bytes, the capture's path and the metrics — until it lets the training go on: `train` set and
        (iteration < iterations or not keep_alive).  Any exception on the way (a closed or stalled socket, a mode off the list) drops
        the connection and returns."""
        from surfel_render import render
        if self.conn is None:
            self.try_connect()
        while self.conn is not None:
            try:
                image_bytes = None
                cam, do_training, keep_alive, scaling_modifier, render_mode = self.conn.receive()
                if cam is not None:
                    mesh_mode = self._mesh_mode(render_mode)
                    if mesh_mode is not None:
                        image_bytes = self._to_host(self._mesh_image(cam, mesh_mode))
                    else:
                        pkg = render(cam, gaussians, pipe, background, scaling_modifier)
                        image_bytes = self._to_host(net_image(pkg, render_mode))
                    self.frames += 1
                self.conn.send(image_bytes, source_path, metrics_fn() if metrics_fn is not None else {})
                if do_training and (iteration < int(iterations) or not keep_alive):
                    break
            except Exception:
                self.drop()


# ------------------------------------------------------------------------------------------------ CLI (view.py)
def build_parser():
    import argparse
    ap = argparse.ArgumentParser(description="Serve a saved model to the SIBR remote viewer (view.py): RGB, alpha, normals, depth, edges, curvature")
    ap.add_argument("-m", "--model_path", required=True)
    ap.add_argument("-s", "--source_path", default=None, help="the capture's path, sent to the viewer with every frame (default: the one in MODEL/cfg_args)")
    ap.add_argument("--iteration", default=-1, type=int, help="point_cloud/iteration_N to load (default: the latest)")
    ap.add_argument("--depth_ratio", default=0.0, type=float)
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--ip", type=str, default="127.0.0.1")
    ap.add_argument("--port", type=int, default=6009)
    ap.add_argument("--mesh", type=str, default=None, help="a mesh (.ply) to show as two more menu items, Mesh and Mesh Normal (MESHVIEW.md); "
                    "an .obj with a texture (TEXTURE.md) adds Mesh Textured")
    return ap


def main(argv=None):
    import argparse
    import surfel_model
    from surfel_mesh import _latest_iteration
    args = build_parser().parse_args(argv)
    cfg = argparse.Namespace()
    path = os.path.join(args.model_path, "cfg_args")
    if os.path.exists(path):
        cfg = eval(open(path).read(), {"Namespace": argparse.Namespace, "__builtins__": {}})
    source = args.source_path if args.source_path is not None else getattr(cfg, "source_path", "")
    white = args.white_background or getattr(cfg, "white_background", False)
    dev = torch.device("cuda")
    it = _latest_iteration(args.model_path) if args.iteration < 0 else args.iteration
    gaussians = surfel_model.GaussianModel(getattr(cfg, "sh_degree", 3), device=dev)
    gaussians.load_ply(os.path.join(args.model_path, "point_cloud", "iteration_%d" % it, "point_cloud.ply"))
    pipe = argparse.Namespace(depth_ratio=args.depth_ratio, debug=0, compute_cov3D_python=False, convert_SHs_python=False)
    background = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    print("View: " + args.model_path)
    mesh = texture = None
    if args.mesh is not None and args.mesh.endswith(".obj"):
        import surfel_texture
        texture = surfel_texture.load_textured_mesh(args.mesh, dev)
        mesh = texture.mesh
    elif args.mesh is not None:
        from surfel_mesh import read_mesh
        mesh = read_mesh(args.mesh, dev)
    viewer = Viewer(args.ip, args.port, mesh=mesh, texture=texture)
    metrics = {"#": int(gaussians.get_opacity.shape[0])}
    try:
        while True:      # (train = 0 keeps serve() inside; a dropped viewer brings it back here to wait for the next one)
            viewer.serve(gaussians, pipe, background, source, lambda: metrics)
            if viewer.conn is None:
                time.sleep(0.05)
    except KeyboardInterrupt:
        pass
    finally:
        viewer.close()
    print("\nViewing complete.")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
