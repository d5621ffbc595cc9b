"""Texture an extracted mesh on MI355X — a triangle atlas and the capture's views baked into it, so that a simplified mesh keeps the
capture's detail: fuse_post_textured.{obj,mtl,png} for Blender, Unity or a web viewer.

The atlas layout (one right isosceles patch per triangle), the baking kernel, the resolve and the textured shading are HIP kernels of
libsurfel_hip.so (include/surfel_texture.h); TEXTURE.md states the rules and every operation order.  The mesh, the views, the
accumulator and the atlas stay on the device; only six class counts per probe and two texel counts cross to the host.  No CPU path:
CPU tensors raise.

    python 2d-gaussian-splatting_amd/surfel_texture.py --ply-path MESH.ply -m MODEL_DIR [-s CAPTURE --source gt]
                                                       [--atlas_size N | --density D] [--blend best] [--png device]   -> MESH_textured.{obj,mtl,png}
"""
import argparse
import ctypes as C
import functools
import os
import sys

import numpy as np
import torch

import surfel_native as _n
import surfel_cull as _c
from surfel_mesh import MeshLimitError, TriangleMesh, read_mesh, shown_colors  # noqa: F401  (MeshLimitError is part of this module's surface)

_n.load()

CLASSES = 6                     # SURFEL_TEXTURE_CLASSES
MIN_LOG2 = 2                    # SURFEL_TEXTURE_MIN_LOG2
PAD = 4                         # SURFEL_TEXTURE_PAD
MAX_SIDE = 16384                # SURFEL_TEXTURE_MAX_SIDE
BAND_INTS = 4                   # SURFEL_TEXTURE_BAND_INTS
MAX_POWER = 8                   # SURFEL_TEXTURE_MAX_POWER
BLENDS = {"average": 0, "best": 1}      # SURFEL_TEXTURE_AVERAGE, _BEST
MAX_PROBES = 40                 # classify calls of one bisection
EPS = _c.EPS                    # the visibility rule's depth margin (CULL.md §Visibility rule 5)
ZNEAR, ZFAR = 0.01, 1000.0      # the depth images' range (surfel_meshview's)
DEFAULT_BUDGET = _c.DEFAULT_BUDGET
GREY = 0.8


def legs(c):
    return 1 << (c + MIN_LOG2)


def cell_side(c):
    return legs(c) + PAD


_dev = functools.partial(_n.device_tensor, "surfel_texture")


def _mesh(mesh):      # (surfel_mesh.mesh_arrays, but one message names both shapes)
    verts = _dev(mesh.vertices, "mesh.vertices")
    tris = _dev(mesh.triangles, "mesh.triangles")
    if verts.ndim != 2 or verts.shape[1] != 3 or tris.ndim != 2 or tris.shape[1] != 3:
        raise ValueError("surfel_texture: mesh.vertices must be [V, 3] and mesh.triangles [F, 3], got %s and %s" % (list(verts.shape), list(tris.shape)))
    return verts.detach().to(torch.float32).contiguous(), tris.detach().to(torch.int32).contiguous()


def _density(density):
    d = np.float32(density)
    if not (np.isfinite(d) and d > 0):
        raise ValueError("surfel_texture: the density (texels per world unit) must be positive and finite, got %r" % (density,))
    return float(d)


# ------------------------------------------------------------------------------------------------ the band table (host)
def band_table(counts, Wa):
    """(table int32 [6, 4], Ha) of six class counts at atlas width Wa (TEXTURE.md §Layout, bands): per class (y0, cells per row, first,
    count), bands stacked largest class first; Ha >= 1.  Raises MeshLimitError as surfel_texture_layout refuses."""
    Wa = int(Wa)
    if not 1 <= Wa <= MAX_SIDE:
        raise MeshLimitError("surfel_texture: the atlas width must be 1 .. %d, got %d" % (MAX_SIDE, Wa))
    table = np.zeros((CLASSES, BAND_INTS), np.int32)
    y = first = 0
    for c in range(CLASSES - 1, -1, -1):
        cell, n = cell_side(c), int(counts[c])
        per = Wa // cell
        table[c] = (y, per, first, n)
        if n == 0:
            continue
        if per < 1:
            raise MeshLimitError("surfel_texture: an atlas %d texels wide is narrower than a cell of %d texels" % (Wa, cell))
        cells = (n + 1) // 2
        y += -(-cells // per) * cell
        first += n
        if y > MAX_SIDE:
            raise MeshLimitError("surfel_texture: the atlas would be higher than %d texels (lower the density)" % MAX_SIDE)
    return table, max(y, 1)


def atlas_height(counts, Wa):
    """band_table's Ha, or None where it raises"""
    try:
        return band_table(counts, Wa)[1]
    except MeshLimitError:
        return None


def bisect_density(probe, size, start=1.0):
    """(density, counts, probes, above): an fp32 density whose atlas fits size x size (band_table(probe(density), size)'s height is at
    most size), such that the bisection's next candidate above it, `above`, does not fit; above is None when every triangle has reached
    the largest class (no density gives a larger atlas).  probe(density) -> six class counts.  The candidate doubles or halves from
    `start` until the bracket is found, then the bracket's geometric mean (rounded to fp32) is tried until it is one of the bracket's
    ends or MAX_PROBES probes are spent.  The height is not exactly monotone in the density (a class change can pack a band's rows
    better), so the condition is the local one this search maintains."""
    size = int(size)
    f32 = lambda d: float(np.float32(d))
    probes = 0

    def fits(d):
        nonlocal probes
        probes += 1
        counts = [int(x) for x in probe(d)]
        h = atlas_height(counts, size)
        return (h is not None and h <= size), counts

    d = f32(start)
    ok, counts = fits(d)
    lo = hi = None
    if ok:
        lo = (d, counts)
        while probes < MAX_PROBES:
            if sum(lo[1][:CLASSES - 1]) == 0:      # every patch has the largest class already
                return lo[0], lo[1], probes, None
            d = f32(lo[0] * 2.0)
            ok, counts = fits(d)
            if not ok:
                hi = d
                break
            lo = (d, counts)
    else:
        hi = d
        while probes < MAX_PROBES:
            if sum(counts[1:]) == 0:               # every patch has the smallest class, and still no room
                break
            d = f32(hi / 2.0)
            ok, counts = fits(d)
            if ok:
                lo = (d, counts)
                break
            hi = d
        if lo is None:
            raise MeshLimitError("surfel_texture: the mesh does not fit an atlas of %d x %d texels at any density" % (size, size))
    while hi is not None and probes < MAX_PROBES:
        mid = f32(np.sqrt(lo[0] * hi))
        if mid <= lo[0] or mid >= hi:
            break
        ok, counts = fits(mid)
        if ok:
            lo = (mid, counts)
        else:
            hi = mid
    return lo[0], lo[1], probes, hi


# ------------------------------------------------------------------------------------------------ layout
class AtlasLayout:
    """What the kernels need to go between triangles and texels: uv [F, 3, 2] float32 (texel coordinates, texel centres at integers),
    cls [F] int32, order [F] int32 (band order -> triangle), on the device; table [6, 4] int32 and counts on the host; width, height,
    density."""

    def __init__(self, uv, cls, order, table, counts, width, height, density):
        self.uv, self.cls, self.order, self.table, self.counts = uv, cls, order, table, counts
        self.width, self.height, self.density = int(width), int(height), density
        self._ctable = (C.c_int * (CLASSES * BAND_INTS))(*[int(x) for x in np.asarray(table).reshape(-1)])


def classify(mesh, density):
    """(cls int32 [F] on the device, counts [6]): the patch class of every triangle at `density` texels per world unit, -1 for a triangle
    without a patch, and the triangles per class (TEXTURE.md §Layout, class).  Waits for the six counts."""
    verts, tris = _mesh(mesh)
    cls = torch.empty(tris.shape[0], dtype=torch.int32, device=verts.device)
    counts = (C.c_int64 * CLASSES)()
    alloc = _n.TorchAllocator(verts.device)
    _n.call(verts.device, "surfel_texture_classify", alloc.cb, None, verts.shape[0], tris.shape[0], verts, tris, _density(density), cls, counts)
    return cls, [int(x) for x in counts]


def layout(mesh, cls, counts, width, density=None):
    """AtlasLayout of the classes classify() returned, `width` texels wide.  Raises MeshLimitError before anything is written when the
    atlas would be wider or higher than MAX_SIDE or narrower than its largest cell."""
    verts, tris = _mesh(mesh)
    F = tris.shape[0]
    cls = _dev(cls, "cls")
    if cls.dtype != torch.int32 or tuple(cls.shape) != (F,) or not cls.is_contiguous():
        raise ValueError("surfel_texture: cls must be a contiguous int32 [F]")
    order = torch.empty(F, dtype=torch.int32, device=verts.device)
    uv = torch.empty((F, 3, 2), dtype=torch.float32, device=verts.device)
    return _layout_into(verts, tris, cls, counts, width, density, order, uv)


def _layout_into(verts, tris, cls, counts, width, density, order, uv):
    table = (C.c_int * (CLASSES * BAND_INTS))()
    alloc = _n.TorchAllocator(verts.device)
    Ha = _n.call(verts.device, "surfel_texture_layout", alloc.cb, None, verts.shape[0], tris.shape[0], verts, tris, cls, (C.c_int64 * CLASSES)(*counts),
                 int(width), table, order, uv)
    return AtlasLayout(uv, cls, order, np.array(table[:], np.int32).reshape(CLASSES, BAND_INTS), list(counts), width, Ha, density)


def atlas_layout(mesh, density=None, atlas_size=None, width=None, stats=None):
    """AtlasLayout of the mesh: at `density` texels per world unit and `width` (default 4096) texels wide, as high as it comes; or, with
    atlas_size = N, at the density bisect_density finds for N x N (height N, the rows below the last band unowned).  stats: a dict that
    receives the probes."""
    if (density is None) == (atlas_size is None):
        raise ValueError("surfel_texture: give density or atlas_size")
    if atlas_size is not None:
        size = int(atlas_size)
        if not cell_side(0) <= size <= MAX_SIDE:
            raise ValueError("surfel_texture: atlas_size must be %d .. %d, got %r" % (cell_side(0), MAX_SIDE, atlas_size))
        verts, _ = _mesh(mesh)
        start = _start_density(verts, size)
        density, counts, probes, above = bisect_density(lambda d: classify(mesh, d)[1], size, start)
        if stats is not None:
            stats.update(probes=probes, above=above)
        cls, counts = classify(mesh, density)
        lay = layout(mesh, cls, counts, size, density)
        lay.height = size
        return lay
    cls, counts = classify(mesh, density)
    return layout(mesh, cls, counts, 4096 if width is None else width, _density(density))


def _start_density(verts, size):
    """where the bisection starts: the atlas side over the bounding box's diagonal (any positive value would do)"""
    if verts.shape[0] == 0:
        return 1.0
    ok = torch.isfinite(verts).all(1)
    if not bool(ok.any()):
        return 1.0
    v = verts[ok]
    diag = float((v.max(0).values - v.min(0).values).norm())
    return size / diag if diag > 0 and np.isfinite(diag) else 1.0


def obj_uv(uv, width, height):
    """OBJ's vt of texel coordinates: ((u + 0.5) / width, 1 - (v + 0.5) / height) — texel centres at integers, v flipped"""
    out = torch.empty_like(uv)
    out[..., 0] = (uv[..., 0] + 0.5) / float(width)
    out[..., 1] = 1.0 - (uv[..., 1] + 0.5) / float(height)
    return out


# ------------------------------------------------------------------------------------------------ baking
def new_accumulator(lay):
    """the zeroed accumulator [Ha, Wa, 4] float32 of a layout: (r, g, b, w) per texel"""
    return torch.zeros((lay.height, lay.width, 4), dtype=torch.float32, device=lay.uv.device)


def _check_acc(acc, lay):
    acc = _dev(acc, "acc")
    if acc.dtype != torch.float32 or tuple(acc.shape) != (lay.height, lay.width, 4) or not acc.is_contiguous():
        raise ValueError("surfel_texture: acc must be a contiguous float32 [%d, %d, 4]" % (lay.height, lay.width))
    return acc


def _blend(blend):
    if blend not in BLENDS:
        raise ValueError("surfel_texture: blend must be 'average' or 'best', got %r" % (blend,))
    return BLENDS[blend]


def bake(mesh, lay, w2c, intrinsics, depth, images, acc, eps=EPS, cos_min=0.1, power=2, blend="average"):
    """acc <- acc combined with a batch of views, in view order (TEXTURE.md §Baking): depth [n, H, W] (surfel_cull.mesh_depth's images of
    this mesh and these cameras), images [n, 3, H, W] float32, both on the device.  The same bits on every run and for every batching."""
    verts, tris = _mesh(mesh)
    dev = verts.device
    acc = _check_acc(acc, lay)
    d = _dev(depth, "depth")
    im = _dev(images, "images")
    if d.ndim != 3 or im.ndim != 4 or im.shape[1] != 3 or tuple(im.shape[2:]) != tuple(d.shape[1:]) or im.shape[0] != d.shape[0]:
        raise ValueError("surfel_texture: depth must be [n, H, W] and images [n, 3, H, W], got %s and %s" % (list(d.shape), list(im.shape)))
    d, im = d.detach().to(torch.float32).contiguous(), im.detach().to(torch.float32).contiguous()
    if not 1 <= int(power) <= MAX_POWER:
        raise ValueError("surfel_texture: power must be 1 .. %d, got %r" % (MAX_POWER, power))
    from surfel_meshview import _device_cameras
    w, k = _device_cameras(w2c, intrinsics, dev)
    if w.shape[0] != d.shape[0]:
        raise ValueError("surfel_texture: %d cameras for %d depth images" % (w.shape[0], d.shape[0]))
    _n.call(dev, "surfel_texture_bake", verts.shape[0], tris.shape[0], verts, tris, lay._ctable, lay.order, lay.width, lay.height, w.shape[0], w, k,
            k.shape[0], d.shape[1], d.shape[2], d, im, float(eps), float(cos_min), int(power), _blend(blend), acc)
    return acc


def resolve(mesh, lay, acc, blend="average", background=(0.0, 0.0, 0.0), out=None):
    """(atlas uint8 [Ha, Wa, 3], stats int64 [2] = owned and seen texels), on the device (TEXTURE.md §Resolve)"""
    verts, tris = _mesh(mesh)
    acc = _check_acc(acc, lay)
    out = _n.uint8_buffer("surfel_texture", out if out is None else _dev(out, "out"), lay.height * lay.width * 3, verts.device)
    stats = torch.empty(2, dtype=torch.int64, device=verts.device)
    bg = [float(x) for x in background]
    cols = shown_colors("surfel_texture", mesh, verts.shape[0])
    _n.call(verts.device, "surfel_texture_resolve", verts.shape[0], tris.shape[0], verts, tris, cols, lay._ctable, lay.order,
            lay.width, lay.height, acc, _blend(blend), bg[0], bg[1], bg[2], out, stats)
    return out.view(lay.height, lay.width, 3), stats


class TexturedMesh:
    """A mesh with its atlas: mesh (TriangleMesh), uv [F, 3, 2] (texel coordinates), atlas uint8 [Ha, Wa, 3], all on the device; layout
    (AtlasLayout); owned, seen: texel counts."""

    def __init__(self, mesh, uv, atlas, layout=None, owned=0, seen=0):
        self.mesh, self.uv, self.atlas, self.layout, self.owned, self.seen = mesh, uv, atlas, layout, int(owned), int(seen)

    @property
    def vt(self):
        """OBJ texture coordinates [F, 3, 2] in [0, 1]"""
        return obj_uv(self.uv, self.atlas.shape[1], self.atlas.shape[0])


def shade(tmesh, key, w2c, sample_intrinsics, H, W, ssaa=1, background=(1.0, 1.0, 1.0), out=None):
    """uint8 [n, H, W, 3]: surfel_meshview.shade's "color" frames of a key tensor [n, ssaa H, ssaa W], with the colour of a sample taken
    from the atlas at the interpolated texture coordinates (TEXTURE.md §Textured shading)"""
    import surfel_meshview as mv
    verts, tris = _mesh(tmesh.mesh)
    dev = verts.device
    key = _dev(key, "key")
    s = int(ssaa)
    if not 1 <= s <= mv.MAX_SSAA:
        raise ValueError("surfel_texture: ssaa must be 1 .. %d, got %r" % (mv.MAX_SSAA, ssaa))
    if key.dtype != torch.int64 or key.ndim != 3 or tuple(key.shape[1:]) != (int(H) * s, int(W) * s) or not key.is_contiguous():
        raise ValueError("surfel_texture: key must be a contiguous int64 [n, %d, %d], got %s %s" % (int(H) * s, int(W) * s, key.dtype, list(key.shape)))
    uv = _dev(tmesh.uv, "uv")
    atlas = _dev(tmesh.atlas, "atlas")
    if uv.dtype != torch.float32 or tuple(uv.shape) != (tris.shape[0], 3, 2) or atlas.dtype != torch.uint8 or atlas.ndim != 3 or atlas.shape[2] != 3:
        raise ValueError("surfel_texture: uv must be float32 [F, 3, 2] and the atlas uint8 [Ha, Wa, 3]")
    w, k = mv._device_cameras(w2c, sample_intrinsics, dev)
    if w.shape[0] != key.shape[0]:
        raise ValueError("surfel_texture: %d cameras for %d key images" % (w.shape[0], key.shape[0]))
    n = key.shape[0]
    out = _n.uint8_buffer("surfel_texture", out, n * int(H) * int(W) * 3, dev)
    bg = [float(x) for x in background]
    _n.call(dev, "surfel_texture_shade", verts.shape[0], tris.shape[0], verts, tris, uv.contiguous(), atlas.contiguous(), atlas.shape[1], atlas.shape[0], n,
            w, k, k.shape[0], int(H), int(W), s, key, bg[0], bg[1], bg[2], out)
    return out.view(n, int(H), int(W), 3)


@torch.no_grad()
def texture_mesh(mesh, cameras, images, depth=None, atlas_size=4096, density=None, blend="average", power=2, cos_min=0.1, eps=EPS, views_per_batch=None,
                 budget_bytes=DEFAULT_BUDGET, background=(0.0, 0.0, 0.0), znear=ZNEAR, zfar=ZFAR, timings=None):
    """TexturedMesh of the mesh under the views: cameras — a list of the project's cameras, or (w2c [n, 3 | 4, 4], intrinsics, H, W);
    images — [n, 3, H, W] or a list of [3, H, W] float tensors on the device, one per camera; depth — surfel_cull.mesh_depth's images
    of the mesh for these cameras ([n, H, W] or a list), rendered here when None.  atlas_size = N: an N x N atlas at the density the
    bisection finds; density = D: that density, atlas_size wide and as high as it comes.  The views go through the device in batches of
    views_per_batch (default: as many as fit budget_bytes, at least one); the atlas does not depend on the batching.  timings: a dict
    that receives ms per stage (synchronises)."""
    import time
    import surfel_meshview as mv
    verts, _ = _mesh(mesh)
    dev = verts.device
    _blend(blend)
    n, groups = mv._view_groups(cameras)
    if len(images) != n or (depth is not None and len(depth) != n):
        raise ValueError("surfel_texture: %d cameras for %d images" % (n, len(images)))
    clock = (lambda: (torch.cuda.synchronize(dev), time.perf_counter())[1]) if timings is not None else (lambda: 0.0)
    t0 = clock()
    stats = {}
    lay = atlas_layout(mesh, atlas_size=atlas_size, stats=stats) if density is None else atlas_layout(mesh, density=density, width=atlas_size)
    t1 = clock()
    acc = new_accumulator(lay)
    depth_ms = bake_ms = 0.0
    for H, W, ids, w2c, k in groups:
        step = int(views_per_batch) if views_per_batch else max(1, int(budget_bytes) // (16 * H * W))
        w, ks = _c._cameras(w2c, k, dev)
        for b in range(0, len(ids), step):
            sel = ids[b:b + step]
            kb = ks if ks.shape[0] == 1 else ks[b:b + step]
            ta = clock()
            if depth is None:
                d = _c.mesh_depth(mesh, w2c[b:b + step], k[b:b + step], H, W, znear, zfar)
            else:
                d = torch.stack([_dev(depth[i], "depth").reshape(H, W) for i in sel])
            tb = clock()
            im = torch.stack([_dev(images[i], "images")[:3] for i in sel]).to(torch.float32)
            bake(mesh, lay, w[b:b + step], kb, d, im, acc, eps, cos_min, power, blend)
            tc = clock()
            depth_ms += (tb - ta) * 1e3
            bake_ms += (tc - tb) * 1e3
            del d, im
    t2 = clock()
    atlas, counts = resolve(mesh, lay, acc, blend, background)
    owned, seen = (int(x) for x in counts.cpu())
    t3 = clock()
    if timings is not None:
        timings.update(layout_ms=(t1 - t0) * 1e3, depth_ms=depth_ms, bake_ms=bake_ms, resolve_ms=(t3 - t2) * 1e3, probes=stats.get("probes", 0))
    return TexturedMesh(mesh, lay.uv, atlas, lay, owned, seen)


def save_textured_mesh(stem, tmesh, png="pillow"):
    """stem.obj, stem.mtl, stem.png; returns the three paths"""
    import surfel_io
    if png not in ("pillow", "device"):
        raise ValueError("surfel_texture: png must be 'pillow' or 'device', got %r" % (png,))
    paths = (stem + ".obj", stem + ".mtl", stem + ".png")
    if png == "device":
        import surfel_png
        with open(paths[2], "wb") as fh:
            fh.write(surfel_png.png_bytes(tmesh.atlas))
    else:
        from PIL import Image
        Image.fromarray(tmesh.atlas.cpu().numpy()).save(paths[2])
    surfel_io.write_obj(paths[0], tmesh.mesh.vertices, tmesh.mesh.triangles, tmesh.vt, texture=os.path.basename(paths[2]))
    return paths


def load_textured_mesh(path, device="cuda:0"):
    """TexturedMesh of an OBJ that save_textured_mesh wrote (the atlas through Pillow)"""
    import surfel_io
    from PIL import Image
    v, t, vt, tex = surfel_io.read_obj(path)
    if vt is None or tex is None:
        raise ValueError("surfel_texture: %s carries no texture coordinates or names no texture" % path)
    dev = torch.device(device)
    atlas = torch.from_numpy(np.array(Image.open(os.path.join(os.path.dirname(path), tex)).convert("RGB"))).to(dev)
    uv = torch.from_numpy(vt.astype(np.float32)).to(dev)
    texel = torch.empty_like(uv)
    texel[..., 0] = uv[..., 0] * atlas.shape[1] - 0.5
    texel[..., 1] = (1.0 - uv[..., 1]) * atlas.shape[0] - 0.5
    return TexturedMesh(TriangleMesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), None), texel.contiguous(), atlas)


# ------------------------------------------------------------------------------------------------ CLI
def build_parser():
    ap = argparse.ArgumentParser(description="Texture a mesh (.ply) from the views of a trained model or of its capture (TEXTURE.md)")
    ap.add_argument("--ply-path", type=str, required=True, help="the mesh; MESH_textured.{obj,mtl,png} are written next to it unless --out says otherwise")
    ap.add_argument("-m", "--model_path", type=str, required=True, help="the model directory (cameras.json, point_cloud/)")
    ap.add_argument("-s", "--source_path", type=str, default=None, help="the capture, for --source gt")
    ap.add_argument("--source", type=str, default="render", choices=["render", "gt"],
                    help="bake the model's renders of the training cameras (render) or the capture's own images (gt)")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--atlas_size", type=int, default=4096)
    ap.add_argument("--density", type=float, default=None, help="texels per world unit instead of the bisection; the atlas is --atlas_size wide")
    ap.add_argument("--blend", type=str, default="average", choices=sorted(BLENDS))
    ap.add_argument("--power", type=int, default=2)
    ap.add_argument("--cos_min", type=float, default=0.1)
    ap.add_argument("--png", type=str, default="pillow", choices=["pillow", "device"])
    ap.add_argument("--out", type=str, default=None, help="the stem of the three files")
    return ap


def main(argv=None):
    import surfel_io
    args = build_parser().parse_args(argv)
    if args.source == "gt" and args.source_path is None:
        raise SystemExit("--source gt needs -s CAPTURE")
    dev = torch.device("cuda:0")
    mesh = read_mesh(args.ply_path, dev)
    stem = args.out or surfel_io.ply_stem(args.ply_path) + "_textured"
    import surfel_mesh
    import surfel_model
    from surfel_render import render
    it = args.iteration if args.iteration >= 0 else surfel_mesh._latest_iteration(args.model_path)
    gaussians = surfel_model.GaussianModel(3, device=dev)
    if args.source == "gt":      # the capture's training cameras carry their images
        scene_args = argparse.Namespace(model_path=args.model_path, source_path=args.source_path, white_background=False)
        cams, _ = surfel_mesh._scene_cameras(scene_args, gaussians, it)
        images = [cam.original_image[0:3] for cam in cams]
    else:
        gaussians.load_ply(os.path.join(args.model_path, "point_cloud", "iteration_%d" % it, "point_cloud.ply"))
        cams = surfel_io.read_cameras_json(os.path.join(args.model_path, "cameras.json"), device=dev)
        pipe = argparse.Namespace(depth_ratio=0.0, debug=0, compute_cov3D_python=False, convert_SHs_python=False)
        ext = surfel_mesh.GaussianExtractor(gaussians, render, pipe, bg_color=[0, 0, 0])
        ext.reconstruction(cams)
        images = ext.rgbmaps
    timings = {}
    tm = texture_mesh(mesh, cams, images, atlas_size=args.atlas_size, density=args.density, blend=args.blend, power=args.power, cos_min=args.cos_min,
                      timings=timings)
    paths = save_textured_mesh(stem, tm, png=args.png)
    print("%d triangles, atlas %d x %d at %.4g texels per unit: %d owned texels, %d seen (%.1f %%) -> %s" %
          (tm.mesh.triangles.shape[0], tm.atlas.shape[1], tm.atlas.shape[0], tm.layout.density, tm.owned, tm.seen, 100.0 * tm.seen / max(tm.owned, 1),
           ", ".join(paths)))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
