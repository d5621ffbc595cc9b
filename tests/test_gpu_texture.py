"""GPU checks of the mesh texturing (include/surfel_texture.h, TEXTURE.md): the layout, the accumulator, the atlas and the textured
frames against the numpy restatement (tests/texture_oracle.py) bit for bit — the bake on the device's own depth images, the shading on
the device's own keys — run-to-run and batching identity, the two closed forms, the inputs the rules skip, empty inputs, the limits,
canaries around every output buffer, and the mesh CLI end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import texture_oracle as O  # noqa: E402
import texture_scenes as S  # noqa: E402
from device_mesh import dev as _dev, mesh as _mesh, to_device as _t  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_CASES = [("ellipsoid", d) for d in S.ELLIPSOID_DENSITIES] + [("cube", d) for d in S.CUBE_DENSITIES]
_CACHE = {}


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _scene(name):
    return S.ellipsoid()[:2] if name == "ellipsoid" else S.cube()


def _dirty():
    torch.empty(1 << 24, dtype=torch.uint8, device=_dev()).fill_(0xA5)      # (a different history of the allocator's memory)
    junk = [torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=_dev()) for n in (1 << 12, 1 << 16, 1 << 20)]
    del junk


def _device_layout(v, t, density, Wa):
    import surfel_texture as P
    mesh = _mesh(v, t)
    cls, counts = P.classify(mesh, density)
    return P.layout(mesh, cls, counts, Wa, density)


def _same_layout(lay, want):
    total = sum(want["counts"])
    assert lay.counts == want["counts"] and lay.height == want["Ha"] and lay.width == want["Wa"]
    assert np.array_equal(lay.table, want["table"]) and lay.table.dtype == np.int32
    assert np.array_equal(lay.cls.cpu().numpy(), want["cls"])
    assert np.array_equal(lay.order.cpu().numpy()[:total].astype(np.int64), want["order"])
    diff = np.argwhere(_bits(lay.uv) != _bits(want["uv"]))
    assert not len(diff), (len(diff), diff[:5])


# ------------------------------------------------------------------------------------------------ 1: the layout
@pytest.mark.parametrize("name,density", LAYOUT_CASES)
def test_layout_equals_the_restatement_bit_for_bit(name, density):
    v, t = _scene(name)
    want = O.layout(v, t, density, S.WA)
    a = _device_layout(v, t, density, S.WA)
    _same_layout(a, want)
    _dirty()
    b = _device_layout(v, t, density, S.WA)
    total = sum(want["counts"])
    for x, y in ((a.uv, b.uv), (a.cls, b.cls), (a.order[:total], b.order[:total])):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert np.array_equal(a.table, b.table) and a.height == b.height
    print("%s at %g: classes %s, atlas %d x %d" % (name, density, a.counts, a.width, a.height))


@pytest.mark.parametrize("F", [1, 2048])
def test_layout_at_the_scan_edges(F):
    """The layout scans six indicator words per triangle: one triangle is the shortest scan there is, 2 048 triangles are three full scan
    tiles of 4 096 (no count gives one tile exactly, 4 096 is no multiple of six)."""
    v, t = S.cube()
    density = S.CUBE_DENSITIES[0]
    _same_layout(_device_layout(v, t[:F], density, S.WA), O.layout(v, t[:F], density, S.WA))


# ------------------------------------------------------------------------------------------------ 2: the bake
def _bake_scene():
    """the ellipsoid, its device layout and the device's own depth images of the 24 arc views, computed once"""
    if "bake" not in _CACHE:
        import surfel_cull as CU
        v, t, c, w2c, intr, H, W = S.ellipsoid()
        w2c = w2c[:S.VIEWS]
        mesh = _mesh(v, t, c)
        lay = _device_layout(v, t, S.BAKE_DENSITY, S.BAKE_WA)
        want = O.layout(v, t, S.BAKE_DENSITY, S.BAKE_WA)
        _same_layout(lay, want)
        depth = CU.mesh_depth(mesh, w2c, intr, H, W, S.ZNEAR, S.ZFAR)
        _CACHE["bake"] = dict(v=v, t=t, c=c, w2c=w2c, intr=intr, H=H, W=W, mesh=mesh, lay=lay, want=want, depth=depth, depth_host=depth.cpu().numpy(),
                              images=_t(S.noise_images()), points=O.texel_points(want))
    return _CACHE["bake"]


def _device_bake(s, blend, power, batch, images=None, mesh=None, lay=None):
    import surfel_texture as P
    lay = lay or s["lay"]
    images = s["images"] if images is None else images
    acc = P.new_accumulator(lay)
    for b in range(0, len(s["w2c"]), batch):
        P.bake(mesh or s["mesh"], lay, s["w2c"][b:b + batch], s["intr"], s["depth"][b:b + batch], images[b:b + batch], acc, S.EPS, 0.1, power, blend)
    return acc


@pytest.mark.parametrize("blend", ["average", "best"])
@pytest.mark.parametrize("power", [1, 4])
def test_bake_equals_the_restatement_bit_for_bit(blend, power):
    import surfel_texture as P
    s = _bake_scene()
    code = P.BLENDS[blend]
    want_acc = O.bake(s["want"], np.zeros((s["lay"].height, s["lay"].width, 4), np.float32), s["w2c"], s["intr"], s["depth_host"], S.noise_images(),
                      S.EPS, 0.1, power, code, points=s["points"])
    want_atlas, _, owned, seen = O.resolve(s["want"], want_acc, s["c"], code, points=s["points"])
    acc = _device_bake(s, blend, power, S.BATCH)      # 24 views in batches of 7: the last batch holds 3
    diff = np.argwhere(_bits(acc) != _bits(want_acc))
    assert not len(diff), (len(diff), diff[:5], acc.cpu().numpy()[tuple(diff[0][:2])], want_acc[tuple(diff[0][:2])])
    atlas, stats = P.resolve(s["mesh"], s["lay"], acc, blend)
    assert atlas.dtype == torch.uint8 and np.array_equal(atlas.cpu().numpy(), want_atlas)
    assert stats.cpu().tolist() == [owned, seen] and 0 < seen < owned
    one = _device_bake(s, blend, power, S.VIEWS)      # all 24 views in one batch: the same bits
    assert one.cpu().numpy().tobytes() == acc.cpu().numpy().tobytes()
    _dirty()
    again = _device_bake(s, blend, power, S.BATCH)
    assert again.cpu().numpy().tobytes() == acc.cpu().numpy().tobytes()
    assert P.resolve(s["mesh"], s["lay"], again, blend)[0].cpu().numpy().tobytes() == atlas.cpu().numpy().tobytes()
    print("%s, power %d: %d owned texels, %d seen (%.1f %%)" % (blend, power, owned, seen, 100.0 * seen / owned))


# ------------------------------------------------------------------------------------------------ 3: the closed forms
def _device_pipeline(v, t, c, w2c, intr, H, W, images, density, Wa, blend="average", power=2):
    import surfel_cull as CU
    import surfel_texture as P
    mesh = _mesh(v, t, c)
    lay = _device_layout(v, t, density, Wa)
    acc = P.new_accumulator(lay)
    depth = CU.mesh_depth(mesh, w2c, intr, H, W, S.ZNEAR, S.ZFAR)
    P.bake(mesh, lay, w2c, intr, depth, _t(images), acc, S.EPS, 0.1, power, blend)
    atlas, stats = P.resolve(mesh, lay, acc, blend)
    host = {"cls": lay.cls.cpu().numpy(), "uv": lay.uv.cpu().numpy(), "Ha": lay.height, "Wa": lay.width}
    return mesh, lay, host, acc.cpu().numpy(), atlas.cpu().numpy(), stats.cpu().tolist()


def test_plate_in_closed_form_on_the_device():
    import test_texture_cpu as TC
    v, t = S.plate()
    w2c, intr, H, W = S.plate_cameras()
    images = np.broadcast_to(S.PLATE_COLORS[:, :, None, None], (5, 3, H, W)).astype(np.float32)
    _, _, host, acc, atlas, _ = _device_pipeline(v, t, None, w2c, intr, H, W, images, S.PLATE_DENSITY, 256)
    tri_of, point = TC._texel_geometry(host, v, t)
    eyes = np.array([-m[:3, :3].T @ m[:3, 3] for m in np.asarray(w2c, np.float64)])
    far = max(np.linalg.norm(np.array([sx * 0.5, sy * 0.5, 0.0]) - e) ** 2 / abs(e[2]) for e in eyes for sx in (-1, 1) for sy in (-1, 1)) / S.PLATE_SIZE[2]
    inner = (tri_of >= 0) & (np.abs(point[..., :2]).max(-1) < S.PLATE_HALF - 2 * far)
    assert inner.sum() > 2000
    w = TC._plate_weights(point[inner], w2c, 2)
    want = (w[:, :, None] * S.PLATE_COLORS.astype(np.float64)[:, None, :]).sum(0) / w.sum(0)[:, None]
    assert (acc[inner][:, 3] > 0).all()
    colour = acc[inner][:, :3] / acc[inner][:, 3:4]
    err = np.abs(colour.astype(np.float64) - want).max()
    print("plate on the device: %d interior texels, colour off by %.2e" % (inner.sum(), err))
    assert err <= 1e-4 and np.abs(acc[inner][:, 3] / w.sum(0) - 1).max() <= 1e-4
    # five equal colours: that colour within one code value
    one = np.array([0.3, 0.6, 0.9], np.float32)
    same = np.broadcast_to(one[None, :, None, None], (5, 3, H, W)).astype(np.float32)
    for blend in ("average", "best"):
        _, _, _, _, atlas, _ = _device_pipeline(v, t, None, w2c, intr, H, W, same, S.PLATE_DENSITY, 256, blend)
        assert np.abs(atlas[inner].astype(np.float64) - np.floor(one.astype(np.float64) * 255)).max() <= 1


def test_rear_plate_falls_back_on_the_device():
    import test_texture_cpu as TC
    v, t, c, first_rear = S.two_plates()
    w2c, intr, H, W = S.plate_cameras()
    w2c = w2c[:1]
    images = np.full((1, 3, H, W), 1.0, np.float32)
    _, _, host, acc, atlas, (owned, seen) = _device_pipeline(v, t, c, w2c, intr, H, W, images, S.PLATE_DENSITY, 256)
    tri_of, point = TC._texel_geometry(host, v, t)
    rear = (tri_of >= first_rear) & (np.abs(point[..., :2]).max(-1) < S.PLATE_HALF - 0.1)
    front = (tri_of >= 0) & (tri_of < first_rear) & (np.abs(point[..., :2]).max(-1) < S.PLATE_HALF - 0.1)
    assert rear.sum() > 2000 and front.sum() > 2000
    assert (acc[rear][:, 3] == 0).all() and (acc[front][:, 3] > 0).all() and 0 < seen < owned
    want = np.floor(np.clip(point[rear] @ S.PLATE_A.T + S.PLATE_B, 0, 1) * 255)
    assert np.abs(atlas[rear].astype(np.float64) - want).max() <= 1 and (atlas[front] >= 254).all()


# ------------------------------------------------------------------------------------------------ 4: skipped and empty inputs
def test_special_triangles_change_nothing():
    import surfel_cull as CU
    import surfel_texture as P
    s = _bake_scene()
    v0, t0, c0 = S.ellipsoid(False)[:3]
    assert len(t0) == len(s["t"]) - 5 and np.array_equal(t0, s["t"][:len(t0)])
    mesh = _mesh(v0, t0, c0)
    lay = _device_layout(v0, t0, S.BAKE_DENSITY, S.BAKE_WA)
    assert bool((s["lay"].cls[len(t0):] == -1).all()) and bool((s["lay"].uv[len(t0):] == 0).all())
    assert lay.counts == s["lay"].counts and lay.height == s["lay"].height and torch.equal(lay.uv, s["lay"].uv[:len(t0)])
    depth = CU.mesh_depth(mesh, s["w2c"], s["intr"], s["H"], s["W"], S.ZNEAR, S.ZFAR)
    plain = dict(s, depth=depth)
    for blend in ("average", "best"):
        a = P.resolve(mesh, lay, _device_bake(plain, blend, 2, S.BATCH, mesh=mesh, lay=lay), blend)[0]
        b = P.resolve(s["mesh"], s["lay"], _device_bake(s, blend, 2, S.BATCH), blend)[0]
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_empty_inputs_return_cleanly():
    import surfel_texture as P
    s = _bake_scene()
    H, W = s["H"], s["W"]
    # no triangles
    none = _mesh(s["v"], np.zeros((0, 3), np.int32), s["c"])
    lay = P.atlas_layout(none, density=10.0, width=64)
    assert lay.height == 1 and lay.counts == [0] * 6 and tuple(lay.uv.shape) == (0, 3, 2)
    acc = P.new_accumulator(lay)
    P.bake(none, lay, s["w2c"][:2], s["intr"], s["depth"][:2], s["images"][:2], acc)
    atlas, stats = P.resolve(none, lay, acc, background=(0.2, 0.4, 0.6))
    assert stats.cpu().tolist() == [0, 0] and bool((atlas == torch.tensor([51, 102, 153], dtype=torch.uint8, device=_dev())).all())
    nothing = _mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    tm = P.texture_mesh(nothing, (np.zeros((0, 4, 4), np.float32), s["intr"], H, W), [], atlas_size=64)
    assert tuple(tm.atlas.shape) == (64, 64, 3) and tm.owned == tm.seen == 0
    # no views: everything falls back to the vertex colours
    acc = P.new_accumulator(s["lay"])
    P.bake(s["mesh"], s["lay"], np.zeros((0, 4, 4), np.float32), s["intr"], s["depth"][:0], s["images"][:0], acc)
    assert not bool(acc.any())
    atlas, stats = P.resolve(s["mesh"], s["lay"], acc)
    want, _, owned, seen = O.resolve(s["want"], np.zeros(tuple(acc.shape), np.float32), s["c"], points=s["points"])
    assert np.array_equal(atlas.cpu().numpy(), want) and stats.cpu().tolist() == [owned, 0]
    tm = P.texture_mesh(s["mesh"], (np.zeros((0, 4, 4), np.float32), s["intr"], H, W), [], density=S.BAKE_DENSITY, atlas_size=S.BAKE_WA)
    assert np.array_equal(tm.atlas.cpu().numpy(), want) and (tm.owned, tm.seen) == (owned, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5: the limits, 6: buffers respected
def _carve(sizes, pad=4096):
    total = pad + sum(s + pad + 16 for s in sizes.values())
    big = torch.empty(total, dtype=torch.uint8, device=_dev())
    pattern = (torch.arange(total, device=_dev()) * 37 + 11).to(torch.uint8)
    big.copy_(pattern)
    off, at = {}, pad
    for name, s in sizes.items():
        at = (at + 15) // 16 * 16
        off[name] = at
        at += s + pad
    inside = torch.zeros(total, dtype=torch.bool, device=_dev())
    for name, s in sizes.items():
        inside[off[name]:off[name] + s] = True
    view = lambda name, dtype: big[off[name]:off[name] + sizes[name]].view(dtype)
    return big, pattern, inside, view


def _raw_layout(v, t, density, Wa, view, table):
    import surfel_native as N
    alloc = N.TorchAllocator(_dev())
    verts, tris = _t(np.asarray(v, np.float32)), _t(np.asarray(t, np.int32))
    counts = (C.c_int64 * 6)()
    N.call(_dev(), "surfel_texture_classify", alloc.cb, None, len(v), len(t), verts, tris, float(density), view("cls", torch.int32), counts)
    Ha = N.call(_dev(), "surfel_texture_layout", alloc.cb, None, len(v), len(t), verts, tris, view("cls", torch.int32), counts, int(Wa), table,
                view("order", torch.int32), view("uv", torch.float32))
    return Ha, list(counts)


def test_limits_are_refused_before_anything_is_written():
    import surfel_native as N
    import surfel_texture as P
    v, t = S.cube()
    sizes = {"cls": 4 * len(t), "order": 4 * len(t), "uv": 24 * len(t)}
    big, pattern, inside, view = _carve(sizes)
    table = (C.c_int * 24)(*([-7] * 24))
    with pytest.raises(N.LimitError, match=r"\(-4\): .*higher"):             # 9 600 cells of 132 texels, 7 per row
        _raw_layout(v, t, 1e6, S.WA, view, table)
    lo = int(view("cls", torch.uint8).data_ptr() - big.data_ptr())
    big[lo:lo + sizes["cls"]] = pattern[lo:lo + sizes["cls"]]                 # (classify wrote the classes; layout must write nothing)
    ve, te = S.ellipsoid()[:2]
    with pytest.raises(N.LimitError, match=r"\(-4\): .*narrower than a cell"):
        _raw_layout(ve, te, 40.0, 100, view, table)                           # the triangle beyond zfar needs a cell of 132
    torch.cuda.synchronize()
    lo_e = 4 * len(te)
    assert torch.equal(big[lo + lo_e:], pattern[lo + lo_e:]) and torch.equal(big[:lo], pattern[:lo]) and list(table) == [-7] * 24
    for call in (lambda: P.atlas_layout(_mesh(v, t), density=1e6, width=S.WA), lambda: P.atlas_layout(_mesh(ve, te), density=40.0, width=100),
                 lambda: P.atlas_layout(_mesh(v, t), density=1.0, width=16385)):
        with pytest.raises(P.MeshLimitError):
            call()


def test_canaries_around_every_output_buffer():
    """cls, order, uv, the accumulator, the atlas, the texel counts and the frames carved out of one allocation filled with a pattern: the
    pattern on both sides of each is intact after the calls, and what lies inside is the result"""
    import surfel_meshview as MV
    import surfel_native as N
    s = _bake_scene()
    v, t, want = s["v"], s["t"], s["want"]
    Wa, Ha, H, W = want["Wa"], want["Ha"], s["H"], s["W"]
    nv = 3
    sizes = {"cls": 4 * len(t), "order": 4 * len(t), "uv": 24 * len(t), "acc": 16 * Ha * Wa, "atlas": 3 * Ha * Wa, "stats": 16, "frames": 3 * nv * H * W}
    big, pattern, inside, view = _carve(sizes)
    table = (C.c_int * 24)()
    got_Ha, counts = _raw_layout(v, t, S.BAKE_DENSITY, Wa, view, table)
    assert got_Ha == Ha and counts == want["counts"] and np.array_equal(np.array(table[:]).reshape(6, 4), want["table"])
    total = sum(counts)
    verts, tris = s["mesh"].vertices, s["mesh"].triangles
    w, k = MV._device_cameras(s["w2c"], s["intr"], _dev())
    acc = view("acc", torch.float32)
    acc.zero_()
    N.call(_dev(), "surfel_texture_bake", len(v), len(t), verts, tris, table, view("order", torch.int32), Wa, Ha, S.VIEWS, w, k, 1, H, W, s["depth"], s["images"],
           S.EPS, 0.1, 2, 0, acc)
    N.call(_dev(), "surfel_texture_resolve", len(v), len(t), verts, tris, s["mesh"].vertex_colors, table, view("order", torch.int32), Wa, Ha, acc, 0,
           0.0, 0.0, 0.0, view("atlas", torch.uint8), view("stats", torch.int64))
    key = MV.visibility(s["mesh"], w[:nv], k, H, W, S.ZNEAR, S.ZFAR)
    N.call(_dev(), "surfel_texture_shade", len(v), len(t), verts, tris, view("uv", torch.float32), view("atlas", torch.uint8), Wa, Ha, nv, w[:nv], k, 1, H, W, 1,
           key, 1.0, 1.0, 1.0, view("frames", torch.uint8))
    torch.cuda.synchronize()
    assert torch.equal(big[~inside], pattern[~inside]) and int((~inside).sum()) >= 8 * 4096
    lo = int(view("order", torch.uint8).data_ptr() - big.data_ptr())      # behind the last patch the order keeps the pattern
    assert torch.equal(big[lo + 4 * total:lo + sizes["order"]], pattern[lo + 4 * total:lo + sizes["order"]]) and total < len(t)
    assert np.array_equal(_bits(view("uv", torch.float32)), _bits(want["uv"]).reshape(-1))
    want_acc = O.bake(want, np.zeros((Ha, Wa, 4), np.float32), s["w2c"], s["intr"], s["depth_host"], S.noise_images(), S.EPS, 0.1, 2, O.AVERAGE,
                      points=s["points"])
    assert np.array_equal(_bits(acc), _bits(want_acc).reshape(-1))
    want_atlas, _, owned, seen = O.resolve(want, want_acc, s["c"], points=s["points"])
    assert np.array_equal(view("atlas", torch.uint8).cpu().numpy(), want_atlas.reshape(-1)) and view("stats", torch.int64).cpu().tolist() == [owned, seen]
    keys = key.cpu().numpy().view(np.uint64)
    frames = view("frames", torch.uint8).cpu().numpy().reshape(nv, H, W, 3)
    for i in range(nv):
        assert np.array_equal(frames[i], O.shade(keys[i], v, t, want["uv"], want_atlas, s["w2c"][i], s["intr"], H, W, 1))


# ------------------------------------------------------------------------------------------------ 7: textured shading
@pytest.mark.parametrize("ssaa", [1, 2])
def test_textured_frames_equal_the_restatement(ssaa):
    import surfel_meshview as MV
    import surfel_texture as P
    s = _bake_scene()
    H, W = s["H"], s["W"]
    views = [0, 11, 23]      # the arc's ends and its middle; the last one sees the special triangles in front of it
    acc = _device_bake(s, "average", 2, S.VIEWS)
    atlas, stats = P.resolve(s["mesh"], s["lay"], acc)
    tm = P.TexturedMesh(s["mesh"], s["lay"].uv, atlas, s["lay"])
    ks = MV.scaled_intrinsics(torch.tensor([s["intr"]]), ssaa)
    key = MV.visibility(s["mesh"], s["w2c"][views], ks, H * ssaa, W * ssaa, S.ZNEAR, S.ZFAR)
    frames = P.shade(tm, key, s["w2c"][views], ks, H, W, ssaa, background=(1.0, 0.5, 0.25))
    keys = key.cpu().numpy().view(np.uint64)
    host_atlas, host_uv = atlas.cpu().numpy(), s["lay"].uv.cpu().numpy()
    hit = 0
    for j, i in enumerate(views):
        want = O.shade(keys[j], s["v"], s["t"], host_uv, host_atlas, s["w2c"][i], ks[0], H, W, ssaa, bg=(1.0, 0.5, 0.25))
        got = frames[j].cpu().numpy()
        assert np.array_equal(got, want), (i, np.argwhere(got != want)[:5])
        hit += int((keys[j] != np.uint64(MV.EMPTY_KEY)).sum())
    assert hit > 1000
    # render_mesh routes mode="textured" here, and leaves the other modes' bytes alone
    cams = (s["w2c"][views], np.asarray(s["intr"]), H, W)
    routed = MV.render_mesh(s["mesh"], cams, mode="textured", texture=tm, ssaa=ssaa, background=(1.0, 0.5, 0.25), znear=S.ZNEAR, zfar=S.ZFAR)
    assert torch.equal(routed, frames)
    with pytest.raises(ValueError, match="needs texture="):
        MV.render_mesh(s["mesh"], cams, mode="textured")


def test_a_mesh_baked_from_uniform_images_renders_uniform():
    import surfel_meshview as MV
    import surfel_texture as P
    s = _bake_scene()
    H, W = s["H"], s["W"]
    colour = np.array([0.25, 0.5, 0.75], np.float32)
    images = _t(np.broadcast_to(colour[None, :, None, None], (S.VIEWS, 3, H, W)).astype(np.float32))
    acc = _device_bake(s, "average", 2, S.BATCH, images=images)
    # (unseen texels take the colour too: vertex colours of that value)
    mesh = _mesh(s["v"], s["t"], np.broadcast_to(colour, s["v"].shape))
    atlas, _ = P.resolve(mesh, s["lay"], acc)
    tm = P.TexturedMesh(mesh, s["lay"].uv, atlas, s["lay"])
    views = [0, 11, 23]
    frames = MV.render_mesh(mesh, (s["w2c"][views], np.asarray(s["intr"]), H, W), mode="textured", texture=tm, ssaa=1, background=(0.0, 0.0, 0.0),
                            znear=S.ZNEAR, zfar=S.ZFAR).cpu().numpy()
    key = MV.visibility(mesh, s["w2c"][views], s["intr"], H, W, S.ZNEAR, S.ZFAR).cpu().numpy().view(np.uint64)
    hit = key != np.uint64(MV.EMPTY_KEY)
    code = np.floor(colour.astype(np.float64) * 255)
    assert hit.sum() > 1000 and np.abs(frames[hit].astype(np.float64) - code).max() <= 1 and (frames[~hit] == 0).all()


def test_the_viewer_serves_mesh_textured():
    """Viewer(..., mesh=, texture=): one more menu item behind Mesh and Mesh Normal, served by render_mesh(mode="textured")"""
    import socket
    import surfel_meshview as MV
    import surfel_texture as P
    import surfel_trainer as TR
    import surfel_view as SV
    import test_gpu_meshview as TMV
    s = _bake_scene()
    atlas, _ = P.resolve(s["mesh"], s["lay"], _device_bake(s, "average", 2, S.VIEWS))
    tm = P.TexturedMesh(s["mesh"], s["lay"].uv, atlas, s["lay"])
    model = TR.synthetic_object(800, _dev(), seed=0, px_scale=0.08)
    bg, pipe = torch.zeros(3, device=_dev()), TR.pipeline_params()
    W, H = 65, 49
    a, b = socket.socketpair()
    a.settimeout(10.0); b.settimeout(10.0)
    viewer = SV.Viewer.attached(a, mesh=s["mesh"], texture=tm)
    assert TMV._recv_json(b) == SV.RENDER_ITEMS + ["Mesh", "Mesh Normal", "Mesh Textured"]
    for mode in (6, 8):
        msg = TMV.VS.message(W, H, mode, seed=3, train=1, keep_alive=1)
        b.sendall(TMV.VS.frame_message(msg))
        viewer.serve(model, pipe, bg, "/capture/path", None, 1, 10)
        assert viewer.conn is not None, mode
        image, verify, _ = TMV._recv_frame(b, W, H)
        cam = TMV._minicam(SV, msg)
        want = MV.render_mesh(s["mesh"], [cam], mode="textured", texture=tm, ssaa=1)[0] if mode == 8 else MV.render_mesh(s["mesh"], [cam], mode="shaded", ssaa=1)[0]
        assert verify == "/capture/path" and np.array_equal(image, want.cpu().numpy()), mode
    b.sendall(TMV.VS.frame_message(TMV.VS.message(W, H, 9, seed=3, train=1)))      # a mode off the longer list drops the viewer
    viewer.serve(model, pipe, bg, "", None, 1, 10)
    assert viewer.conn is None
    b.close()


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_mesh_cli_writes_a_textured_mesh(tmp_path):
    """surfel_mesh.py --texture --simplify_faces on a sphere of surfels: the three files, an atlas Pillow opens at its size, an OBJ that
    holds the simplified mesh with 3 F texture coordinates in [0, 1], and frames of it"""
    from PIL import Image
    import surfel_io
    import surfel_mesh
    import surfel_meshview as MV
    import surfel_texture as P
    import surfel_trainer as TR
    import test_gpu_mesh as TM
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import mesh_bench
    dev = _dev()
    model = TM._sphere_model(dev)
    cams = TR.orbit_cameras(22, 256, 192, device=dev)
    mesh_bench.write_model_dir(model, cams, str(tmp_path), 7)
    assert surfel_mesh.main(["-m", str(tmp_path), "--mesh_res", "256", "--simplify_faces", "2000", "--num_cluster", "1", "--texture", "--atlas_size", "512"]) == 0
    out = tmp_path / "train" / "ours_7"
    assert sorted(os.listdir(out)) == ["fuse.ply", "fuse_post.ply", "fuse_post_simplified.ply", "fuse_post_textured.mtl", "fuse_post_textured.obj",
                                       "fuse_post_textured.png"]
    img = Image.open(str(out / "fuse_post_textured.png"))
    assert img.size == (512, 512) and img.mode == "RGB"
    sv, st, _ = surfel_io.read_triangle_mesh(str(out / "fuse_post_simplified.ply"))
    v, t, vt, tex = surfel_io.read_obj(str(out / "fuse_post_textured.obj"))
    assert tex == "fuse_post_textured.png" and np.array_equal(t, st) and np.array_equal(v, sv) and 100 < len(t) <= 2000
    assert vt.shape == (len(t), 3, 2) and vt.min() >= 0 and vt.max() <= 1
    pixels = np.asarray(img)
    assert pixels.reshape(-1, 3).any(1).mean() > 0.3      # the atlas holds the bake, not the background
    tm = P.load_textured_mesh(str(out / "fuse_post_textured.obj"), dev)
    MV.render_mesh_path(tm.mesh, cams, str(tmp_path / "view"), modes=("textured",), texture=tm, path=False, ssaa=1)
    names = sorted(os.listdir(tmp_path / "view" / "mesh"))
    assert names == ["textured_%05d.png" % i for i in range(len(cams))]
    frame = np.asarray(Image.open(str(tmp_path / "view" / "mesh" / names[0])))
    assert frame.shape == (192, 256, 3) and (frame != 255).any(-1).mean() > 0.05      # the sphere shows on the white background
    # the stand-alone tool on the simplified mesh: the model's renders of cameras.json, the best view per texel, the device's PNG encoder
    stem = str(tmp_path / "alone")
    assert P.main(["--ply-path", str(out / "fuse_post_simplified.ply"), "-m", str(tmp_path), "--atlas_size", "256", "--blend", "best", "--png", "device",
                   "--out", stem]) == 0
    img2 = Image.open(stem + ".png")
    v2, t2, vt2, tex2 = surfel_io.read_obj(stem + ".obj")
    assert img2.size == (256, 256) and img2.mode == "RGB" and tex2 == "alone.png" and np.array_equal(t2, st) and vt2.min() >= 0 and vt2.max() <= 1
    assert np.asarray(img2).reshape(-1, 3).any(1).mean() > 0.3
