"""The mesh tools' shape refusals on the device, word for word (the strings the modules carried before surfel_native.rows and
surfel_mesh.mesh_arrays took the checks over, written out here): vertices [4, 2], triangles [1, 2], [2, 3] colours beside [4, 3] vertices
where a module reads colours — and an empty vertex_colors, which the two modules that draw a mesh still take as "no colours".  (surfel_log
takes no mesh: its refusal is in test_wrapper_args_cpu.py.)  Then the image side: every place that takes a caller's uint8 output buffer,
and the encoders' frame shapes."""
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


# ------------------------------------------------------------------------------------------------ caller-supplied output buffers
# The ten places that take a caller's uint8 buffer, each with a 4 x 4 frame.  Texts as the modules carried them before
# surfel_native.uint8_buffer took the check over.  What each place accepts and refuses:
#
#                                           one short   every 2nd byte   int8    [1, n] of n bytes   n bytes, 1-D
#   encode_png out, scratch; encode_jpeg    refused     refused          refused refused             accepted (and more than n)
#   the other seven ("of n elements")       refused     refused          refused accepted            accepted (n exactly)
def _frame(*shape):
    return torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=shape, dtype=np.uint8)).cuda()


def _planes(*shape):
    return torch.from_numpy(np.random.default_rng(6).random(shape, dtype=np.float32)).cuda()


def _shaded(out):
    import surfel_meshview as P
    m = _mesh(V, T, V)
    return P.shade(m, P.visibility(m, W2C, K, 4, 4), W2C, K, 4, 4, mode="color", out=out)


@pytest.fixture(scope="module")
def textured():
    import surfel_texture as P
    m = _mesh(V, T, V)
    lay = P.atlas_layout(m, density=1.0, width=256)
    return m, lay, P.TexturedMesh(m, lay.uv, P.resolve(m, lay, P.new_accumulator(lay))[0], lay)


def _site(name, textured):
    """(call(out), n, text, one_dimensional) of a place"""
    import surfel_log, surfel_meshview, surfel_path, surfel_png, surfel_texture, surfel_video, surfel_view
    m, lay, tm = textured
    atlas_bytes = lay.height * lay.width * 3
    return {
        "encode_png-out": (lambda b: surfel_png.encode_png(_frame(4, 4, 3), out=b), 431,
                           "encode_png: out must be a contiguous uint8 tensor of at least 431 elements", True),
        # (the scratch size is the library's to choose: the text takes it from the query)
        "encode_png-scratch": (lambda b: surfel_png.encode_png(_frame(4, 4, 3), scratch=b), surfel_png.scratch_bytes(4, 4, 3),
                               "encode_png: scratch must be a contiguous uint8 tensor of at least %d elements" % surfel_png.scratch_bytes(4, 4, 3), True),
        "encode_jpeg-out": (lambda b: surfel_video.encode_jpeg(_frame(4, 4, 3), out=b), 3129,
                            "encode_jpeg: out must be a contiguous uint8 tensor of at least 3129 elements", True),
        "quantize_u8": (lambda b: surfel_path.quantize_u8(_planes(3, 4, 4), out=b), 48,
                        "quantize_u8: out must be a contiguous uint8 tensor of 48 elements", False),
        "colorize_depth": (lambda b: surfel_path.colorize_depth(_planes(4, 4) + 1.0, 0.0, 1.0, out=b), 48,
                           "colorize_depth: out must be a contiguous uint8 tensor of 48 elements", False),
        "surfel_log.panel": (lambda b: surfel_log.panel("rgb", _planes(3, 4, 4), out=b), 48,
                             "surfel_log.panel: out must be a contiguous uint8 tensor of 48 elements", False),
        "net_image": (lambda b: surfel_view.net_image({"rend_alpha": _planes(1, 4, 4)}, "alpha", out=b), 48,
                      "net_image: out must be a contiguous uint8 tensor of 48 elements", False),
        "surfel_meshview.shade": (_shaded, 48, "surfel_meshview: out must be a contiguous uint8 tensor of 48 elements", False),
        "surfel_texture.resolve": (lambda b: surfel_texture.resolve(m, lay, surfel_texture.new_accumulator(lay), out=b)[0], atlas_bytes,
                                   "surfel_texture: out must be a contiguous uint8 tensor of %d elements" % atlas_bytes, False),
        "surfel_texture.shade": (lambda b: surfel_texture.shade(tm, surfel_meshview.visibility(m, W2C, K, 4, 4), W2C, K, 4, 4, out=b), 48,
                                 "surfel_texture: out must be a contiguous uint8 tensor of 48 elements", False),
    }[name]


SITES = ["encode_png-out", "encode_png-scratch", "encode_jpeg-out", "quantize_u8", "colorize_depth", "surfel_log.panel", "net_image",
         "surfel_meshview.shade", "surfel_texture.resolve", "surfel_texture.shade"]


@pytest.mark.parametrize("name", SITES)
def test_callers_output_buffer(name, textured):
    call, n, text, one_dimensional = _site(name, textured)
    d = torch.device("cuda:0")
    _refused(lambda: call(torch.empty(n - 1, dtype=torch.uint8, device=d)), text)
    _refused(lambda: call(torch.empty(2 * n, dtype=torch.uint8, device=d)[::2]), text)
    _refused(lambda: call(torch.empty(n, dtype=torch.int8, device=d)), text)
    if one_dimensional:
        _refused(lambda: call(torch.empty((1, n), dtype=torch.uint8, device=d)), text)
        call(torch.empty(n + 1, dtype=torch.uint8, device=d))      # more than asked for is fine
    else:
        want = call(None)
        assert torch.equal(call(torch.empty((1, n), dtype=torch.uint8, device=d)), want) and want.shape[-1] == 3      # any shape of n bytes
        _refused(lambda: call(torch.empty(n + 1, dtype=torch.uint8, device=d)), text)


def test_frame_shapes_of_the_encoders():
    import surfel_png, surfel_video
    _refused(lambda: surfel_png.encode_png(_frame(4, 4, 3).float()), "surfel_png: a uint8 [H, W, 1 or 3] frame expected, got torch.float32 (4, 4, 3)")
    _refused(lambda: surfel_png.encode_png(_frame(4, 4, 2)), "surfel_png: a uint8 [H, W, 1 or 3] frame expected, got torch.uint8 (4, 4, 2)")
    _refused(lambda: surfel_video.encode_jpeg(_frame(4, 4, 1)), "surfel_video: a uint8 [H, W, 3] frame expected, got torch.uint8 (4, 4, 1)")
    _refused(lambda: surfel_video.encode_jpeg(_frame(4, 4)), "surfel_video: a uint8 [H, W, 3] frame expected, got torch.uint8 (4, 4)")
