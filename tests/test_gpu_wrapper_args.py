"""The mesh tools' shape refusals on the device, word for word (the strings the modules carried before surfel_native.rows and
surfel_mesh.mesh_arrays took the checks over, written out here): vertices [4, 2], triangles [1, 2], [2, 3] colours beside [4, 3] vertices
where a module reads colours — and an empty vertex_colors, which the two modules that draw a mesh still take as "no colours".  (surfel_log
takes no mesh: its refusal is in test_wrapper_args_cpu.py.)"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from device_mesh import mesh as _mesh  # noqa: E402

W2C, K = np.eye(4, dtype=np.float32)[None], (2.0, 2.0, 0.5, 0.5)
# one triangle in front of the camera at the origin, and a fourth vertex no triangle uses
V = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2], [0, 0, 5]], np.float32)
T = np.array([[0, 1, 2]], np.int32)


def _refused(call, text):
    with pytest.raises(ValueError) as e:
        call()
    assert type(e.value) is ValueError and str(e.value) == text


# module, the entry that checks first as f(module, mesh), the text for vertices [4, 2] and for triangles [1, 2] (None: read as they come)
SHAPES = [
    ("surfel_cull", lambda P, m: P.mesh_depth(m, W2C, K, 2, 2),
     "surfel_cull: mesh.vertices must be [N, 3], got [4, 2]", "surfel_cull: mesh.triangles must be [F, 3], got [1, 2]"),
    ("surfel_eval", lambda P, m: P.sample_mesh(m, 0.2),
     "surfel_eval: mesh.vertices must be [N, 3], got [4, 2]", None),
    ("surfel_eval_tnt", lambda P, m: P.mesh_cloud(m),
     "surfel_eval_tnt: mesh.vertices must be [N, 3], got [4, 2]", None),
    ("surfel_meshview", lambda P, m: P.vertex_normals(m),
     "surfel_meshview: mesh.vertices must be [V, 3], got [4, 2]", "surfel_meshview: mesh.triangles must be [F, 3], got [1, 2]"),
    ("surfel_texture", lambda P, m: P.classify(m, 1.0),
     "surfel_texture: mesh.vertices must be [V, 3] and mesh.triangles [F, 3], got [4, 2] and [1, 3]",
     "surfel_texture: mesh.vertices must be [V, 3] and mesh.triangles [F, 3], got [4, 3] and [1, 2]"),
    ("surfel_simplify", lambda P, m: P.simplify_mesh(m, cell=0.5),
     "surfel_simplify: mesh.vertices must be [N, 3], got [4, 2]", "surfel_simplify: mesh.triangles must be [N, 3], got [1, 2]"),
    ("surfel_smooth", lambda P, m: P.mesh_adjacency(m),
     "surfel_smooth: mesh.vertices must be [N, 3], got [4, 2]", "surfel_smooth: mesh.triangles must be [N, 3], got [1, 2]"),
    ("surfel_repair", lambda P, m: P.repair_mesh(m),
     "surfel_repair: mesh.vertices must be [N, 3], got [4, 2]", "surfel_repair: mesh.triangles must be [N, 3], got [1, 2]"),
]


@pytest.mark.parametrize("name,entry,vertex_text,triangle_text", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes_of_vertices_and_triangles(name, entry, vertex_text, triangle_text):
    P = importlib.import_module(name)
    _refused(lambda: entry(P, _mesh(V[:, :2], T)), vertex_text)
    if triangle_text is not None:
        _refused(lambda: entry(P, _mesh(V, T[:, :2])), triangle_text)


def _meshview_frames(mesh):
    import surfel_meshview as P
    return P.shade(mesh, P.visibility(mesh, W2C, K, 2, 2), W2C, K, 2, 2, mode="color")


def _texture_atlas(mesh):
    import surfel_texture as P
    lay = P.atlas_layout(mesh, density=1.0, width=256)
    return P.resolve(mesh, lay, P.new_accumulator(lay))[0]


# the modules that read colours: an entry as f(mesh) and its text for [2, 3] colours beside [4, 3] vertices
COLOURS = [
    (lambda m: importlib.import_module("surfel_simplify").simplify_mesh(m, cell=0.5), "surfel_simplify: 2 colours for 4 vertices"),
    (lambda m: importlib.import_module("surfel_smooth").smooth_mesh(m, iterations=1, colors=True), "surfel_smooth: 2 colours for 4 vertices"),
    (lambda m: importlib.import_module("surfel_repair").repair_mesh(m), "surfel_repair: 2 colours for 4 vertices"),
    (_meshview_frames, "surfel_meshview: mesh.vertex_colors must be [V, 3], got [2, 3]"),
    (_texture_atlas, "surfel_texture: mesh.vertex_colors must be [V, 3], got [2, 3]"),
]


@pytest.mark.parametrize("entry,text", COLOURS, ids=["simplify", "smooth", "repair", "meshview", "texture"])
def test_two_colours_for_four_vertices(entry, text):
    _refused(lambda: entry(_mesh(V, T, V[:2])), text)


@pytest.mark.parametrize("draw", [_meshview_frames, _texture_atlas], ids=["meshview", "texture"])
def test_empty_colours_are_no_colours(draw):
    assert torch.equal(draw(_mesh(V, T, np.zeros((0, 3), np.float32))), draw(_mesh(V, T)))
