"""Generate tests/golden/ref_view.npz by IMPORTING the reference's own utils/image_utils.py, gaussian_renderer/network_gui.py and
scene/cameras.py and running them on the seeded inputs of tests/view_scenes.py.  Runs only in the build container (needs
/root/reference); the .npz (arrays only) is committed.

Stand-ins: torch.Tensor.cuda is the identity for the calls (no GPU in the build container); `plt.cm.get_cmap`, which newer matplotlib
releases no longer have, is matplotlib.colormaps[name]; network_gui.py and cameras.py are loaded by file path, so the packages around
them (which import the reference's native rasterizer) are not.  The sockets are the two ends of socket.socketpair(): nothing is bound.

Recorded:
  img/<H>x<W>/<input>            the four maps of view_scenes.package(H, W)
  img/<H>x<W>/<mode>             the reference's bytes [H, W, 3]: render_net_image, then train.py:156's clamp * 255, byte, permute
  turbo                          colormap()'s table as the reference builds it: float32 colours * 255, truncated to bytes [256, 3]
  wire/items, wire/frame, wire/noframe      the byte streams of try_connect's send_json_data(render_items), of send(image, verify,
                                 metrics) and of send(None, verify, metrics)
  wire/image, wire/verify, wire/metrics     what those sends were given (metrics as JSON text)
  recv/<k>/message               message k as it goes on the wire (k = 0: 37 x 23, mode 4; k = 1: resolution 0)
  recv/<k>/...                   what receive() made of it: is_none, world_view_transform, full_proj_transform, camera_center, size,
                                 scalars = (fovy, fovx, znear, zfar, scaling_modifier) as float64, flags = (do_training, keep_alive, mode)

Usage:  python tests/golden/make_golden_view.py
"""
import importlib.util
import json
import os
import socket
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))

import view_scenes as VS  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _drain(sock):
    sock.settimeout(0.2)
    got = b""
    try:
        while True:
            piece = sock.recv(1 << 20)
            if not piece:
                break
            got += piece
    except socket.timeout:
        pass
    return got


def main():
    import matplotlib
    import matplotlib.pyplot as plt
    if not hasattr(plt.cm, "get_cmap"):
        plt.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    sys.path.insert(0, REF)
    from utils import image_utils as IU
    scene = types.ModuleType("scene"); scene.__path__ = [os.path.join(REF, "scene")]
    sys.modules["scene"] = scene
    _load("scene.cameras", os.path.join(REF, "scene", "cameras.py"))
    NG = _load("ref_network_gui", os.path.join(REF, "gaussian_renderer", "network_gui.py"))
    NG.listener.close()      # (created at import, never bound)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        for H, W in VS.GOLDEN_SHAPES:
            pkg = VS.package(H, W)
            tp = {k: torch.from_numpy(v) for k, v in pkg.items()}
            for k, v in pkg.items():
                out["img/%dx%d/%s" % (H, W, k)] = v
            for mode, name in enumerate(VS.RENDER_ITEMS):
                net = IU.render_net_image(tp, VS.RENDER_ITEMS, mode, None)
                b = (torch.clamp(net, min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous().cpu().numpy()
                assert b.shape == (H, W, 3) and b.dtype == np.uint8
                out["img/%dx%d/%s" % (H, W, name)] = b
        colors = torch.tensor(plt.cm.get_cmap("turbo").colors)
        assert colors.dtype == torch.float32
        out["turbo"] = (torch.clamp(colors, min=0, max=1.0) * 255).byte().numpy()

        a, b = socket.socketpair()
        NG.conn = a
        NG.send_json_data(a, VS.RENDER_ITEMS)
        out["wire/items"] = np.frombuffer(_drain(b), np.uint8)
        image = out["img/23x37/Edge"]
        verify, metrics = "/data/captures/scan24", {"#": 12345, "loss": 0.03125}
        NG.send(memoryview(image), verify, metrics)
        out["wire/frame"] = np.frombuffer(_drain(b), np.uint8)
        NG.send(None, verify, metrics)
        out["wire/noframe"] = np.frombuffer(_drain(b), np.uint8)
        out["wire/image"], out["wire/verify"], out["wire/metrics"] = image, np.array(verify), np.array(json.dumps(metrics))
        msgs = [VS.message(37, 23, 4, seed=5, train=1, keep_alive=0, scaling_modifier=0.75), VS.message(0, 0, 0, seed=6)]
        for k, msg in enumerate(msgs):
            wire = VS.frame_message(msg)
            out["recv/%d/message" % k] = np.frombuffer(wire, np.uint8)
            b.sendall(wire)
            cam, do_training, keep_alive, scaling_modifier, mode = NG.receive()
            out["recv/%d/is_none" % k] = np.array(cam is None)
            if cam is None:
                assert (do_training, keep_alive, scaling_modifier, mode) == (None, None, None, None)
                continue
            out["recv/%d/world_view_transform" % k] = cam.world_view_transform.numpy()
            out["recv/%d/full_proj_transform" % k] = cam.full_proj_transform.numpy()
            out["recv/%d/camera_center" % k] = cam.camera_center.numpy()
            out["recv/%d/size" % k] = np.array([cam.image_width, cam.image_height])
            out["recv/%d/scalars" % k] = np.array([cam.FoVy, cam.FoVx, cam.znear, cam.zfar, scaling_modifier], np.float64)
            out["recv/%d/flags" % k] = np.array([int(do_training), int(keep_alive), int(mode)])
        a.close(); b.close()
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "ref_view.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
