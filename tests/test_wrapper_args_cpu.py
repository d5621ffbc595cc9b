"""The mesh tools' refusal of anything but a device tensor, word for word: every module's first-checking entry is given a CPU tensor and a
numpy array and must raise RuntimeError with the text below — the strings the modules carried before the check moved into
surfel_native.device_tensor, written out here and not derived from it.  No device is needed: the check comes before any device call.
The frame modules (PNG, video, path frames) follow: the same check without an argument's name."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

W2C, K = np.eye(4, dtype=np.float32)[None], (60.0, 60.0, 1.0, 1.0)


def _mesh(x):
    from surfel_mesh import TriangleMesh
    return TriangleMesh(x, torch.zeros((1, 3), dtype=torch.int32), None)


# module, its entry that checks first as f(module, x) for a host [4, 3] x, and the texts for a CPU tensor and for a numpy array
CASES = [
    ("surfel_cull", lambda P, x: P.mesh_depth(_mesh(x), W2C, K, 2, 2),
     "surfel_cull: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_cull: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_eval", lambda P, x: P.sample_mesh(_mesh(x), 0.2),
     "surfel_eval: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_eval: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_eval_tnt", lambda P, x: P.mesh_cloud(_mesh(x)),
     "surfel_eval_tnt: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_eval_tnt: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_meshview", lambda P, x: P.vertex_normals(_mesh(x)),
     "surfel_meshview: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_meshview: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_texture", lambda P, x: P.classify(_mesh(x), 10.0),
     "surfel_texture: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_texture: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_simplify", lambda P, x: P.simplify_mesh(_mesh(x), cell=0.5),
     "surfel_simplify: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_simplify: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_smooth", lambda P, x: P.mesh_adjacency(_mesh(x)),
     "surfel_smooth: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_smooth: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_repair", lambda P, x: P.repair_mesh(_mesh(x)),
     "surfel_repair: tensors must live on a HIP device (mesh.vertices: got cpu)",
     "surfel_repair: tensors must live on a HIP device (mesh.vertices: got ndarray)"),
    ("surfel_log", lambda P, x: P.panel("rgb", x),
     "surfel_log: tensors must live on a HIP device (planes: got cpu)",
     "surfel_log: tensors must live on a HIP device (planes: got ndarray)"),
    ("surfel_log", lambda P, x: P.append(None, None, 1, 1, x, 0.0, 0.0),
     "surfel_log: tensors must live on a HIP device (scalars: got cpu)",
     "surfel_log: tensors must live on a HIP device (scalars: got ndarray)"),
]


@pytest.mark.parametrize("name,entry,cpu_text,numpy_text", CASES, ids=[c[0] for c in CASES[:-1]] + ["surfel_log-append"])
def test_module_refuses_host_arrays(name, entry, cpu_text, numpy_text):
    P = importlib.import_module(name)
    for x, text in ((torch.zeros((4, 3)), cpu_text), (np.zeros((4, 3), np.float32), numpy_text)):
        with pytest.raises(RuntimeError) as e:
            entry(P, x)
        assert type(e.value) is RuntimeError and str(e.value) == text


def _add_frame(P, x, tmp_path):
    with P.VideoWriter(os.path.join(tmp_path, "refused.avi"), 4, 3) as vw:
        vw.add_frame(x)


# the frame modules: the entry as f(module, x, tmp_path), and the module name the message starts with
FRAME_CASES = [
    ("surfel_png", "encode_png", lambda P, x, tmp: P.encode_png(x)),
    ("surfel_png", "png_bytes", lambda P, x, tmp: P.png_bytes(x)),
    ("surfel_video", "encode_jpeg", lambda P, x, tmp: P.encode_jpeg(x)),
    ("surfel_video", "VideoWriter.add_frame", _add_frame),
    ("surfel_path", "quantize_u8", lambda P, x, tmp: P.quantize_u8(x)),
    ("surfel_path", "colorize_depth", lambda P, x, tmp: P.colorize_depth(x, 0.0, 1.0)),
    ("surfel_path", "order_stats", lambda P, x, tmp: P.order_stats(x, [0])),
]
FRAME_TEXTS = {"surfel_png": ("surfel_png: tensors must live on a HIP device (got cpu)", "surfel_png: tensors must live on a HIP device (got ndarray)"),
               "surfel_video": ("surfel_video: tensors must live on a HIP device (got cpu)", "surfel_video: tensors must live on a HIP device (got ndarray)"),
               "surfel_path": ("surfel_path: tensors must live on a HIP device (got cpu)", "surfel_path: tensors must live on a HIP device (got ndarray)")}


@pytest.mark.parametrize("name,entry", [(c[0], c[2]) for c in FRAME_CASES], ids=[c[1] for c in FRAME_CASES])
def test_frame_entry_refuses_host_arrays(name, entry, tmp_path):
    P = importlib.import_module(name)
    for x, text in zip((torch.zeros((4, 3, 3), dtype=torch.uint8), np.zeros((4, 3, 3), np.uint8)), FRAME_TEXTS[name]):
        with pytest.raises(RuntimeError) as e:
            entry(P, x, str(tmp_path))
        assert type(e.value) is RuntimeError and str(e.value) == text
