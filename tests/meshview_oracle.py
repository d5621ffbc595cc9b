"""numpy oracles of the mesh viewer (MESHVIEW.md).  (a) A restatement of the vertex-normal and shading kernels in float32, operation by
operation, that takes a key buffer as its input.  (b) The same rules in float64 on top of cull_oracle.depth_image's nearest triangle: the
functions below take the number type as an argument, as cull_oracle's twins do.  Also the rule that says which pixels are *undecided* —
cull_oracle's own rule, the twins disagreeing on the nearest triangle, or another triangle's hit within CLOSE (relative) of the nearest —
and a closed form for the anchor quad that shares nothing with the barycentric path."""
import functools

import numpy as np

import cull_oracle as O
import path_oracle as PO

F32, F64 = np.float32, np.float64
INF_BITS = 0x7f800000
EMPTY = np.uint64((INF_BITS << 32) | 0xffffffff)       # SURFEL_MESHVIEW_EMPTY
SCALE = 1048576                                        # SURFEL_MESHVIEW_NORMAL_SCALE
MODES = {"shaded": 0, "normal": 1, "color": 2}         # SURFEL_MESHVIEW_SHADED, _NORMAL, _COLOR
GREY = 0.8
# Two hits closer than this (relative) may swap under the depth bar of CULL.md: about 1.07e-3 per hit, so two hits close 2.14e-3 at
# most; the margin is twice that.
CLOSE = 4.5e-3
CAP = 5e-3                                             # the largest share of undecided pixels an image may have


# ------------------------------------------------------------------------------------------------ keys
def pack(depth, tri):
    """uint64 keys of a depth image (0: empty) and the nearest-triangle image (-1: empty): (fp32 bits of z) << 32 | index"""
    bits = np.asarray(depth, F32).view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | (np.asarray(tri, np.int64) & 0xffffffff).astype(np.uint64)
    return np.where(np.asarray(tri) < 0, EMPTY, key)


def unpack(key):
    """(depth float32 with 0 where empty, triangle int32 with -1 where empty)"""
    key = np.asarray(key).view(np.uint64) if np.asarray(key).dtype == np.int64 else np.asarray(key, np.uint64)
    bits = (key >> np.uint64(32)).astype(np.uint32)
    empty = bits >= INF_BITS
    return np.where(empty, F32(0), bits.view(F32)), np.where(empty, -1, (key & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)


def scaled_intrinsics(intr, s):
    """the intrinsics of the s H x s W sample grid: sample (s x + k) sits at pixel coordinate x + (k + 0.5) / s - 0.5"""
    k = np.asarray(intr, np.float64).reshape(-1, 4)
    out = np.stack([k[:, 0] * s, k[:, 1] * s, s * k[:, 2] + (s - 1) / 2, s * k[:, 3] + (s - 1) / 2], 1)
    return out.astype(F32)


# ------------------------------------------------------------------------------------------------ vertex normals
def _unit_face_normals(verts, tris, T):
    """(indices [F', 3] of the triangles that count, their unit normals [F', 3] in T): fn = (p1 - p0) x (p2 - p0), u = fn / sqrt(fn . fn)"""
    v = np.asarray(verts, F32).astype(T)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    t = t[((t >= 0) & (t < len(v))).all(1)]
    with np.errstate(all="ignore"):
        a, b = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        fx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        fy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        fz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        length = np.sqrt((fx * fx + fy * fy) + fz * fz)
        ok = np.isfinite(fx) & np.isfinite(fy) & np.isfinite(fz) & np.isfinite(length) & (length > 0)
        u = np.stack([fx / length, fy / length, fz / length], 1)
    return t[ok], u[ok]


def face_quanta(verts, tris):
    """(indices [F', 3], q [F', 3] int64): q = (int64) rint(u * 2^20) in float32"""
    t, u = _unit_face_normals(verts, tris, F32)
    return t, np.rint(u * F32(SCALE)).astype(np.int64)


def normal_sums(verts, tris):
    """int64 [V, 3]: the sums the device keeps with 64-bit integer atomics"""
    t, q = face_quanta(verts, tris)
    acc = np.zeros((len(verts), 3), np.int64)
    for k in range(3):
        np.add.at(acc, t[:, k], q)
    return acc


def normals_from_sums(acc):
    """float32 [V, 3]: (float) acc / sqrt((x x + y y) + z z); a zero sum stays (0, 0, 0)"""
    a = np.asarray(acc, np.int64).astype(F32)
    with np.errstate(all="ignore"):
        length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        n = a / length[:, None]
    return np.where((length > 0)[:, None], n, F32(0)).astype(F32)


def vertex_normals(verts, tris):
    return normals_from_sums(normal_sums(verts, tris))


def vertex_normals64(verts, tris):
    """angle-free averaging in float64: the normalised sum of the unit face normals around every vertex, no fixed point"""
    t, u = _unit_face_normals(verts, tris, F64)
    acc = np.zeros((len(verts), 3), F64)
    for k in range(3):
        np.add.at(acc, t[:, k], u)
    length = np.sqrt((acc * acc).sum(1))
    with np.errstate(all="ignore"):
        return np.where((length > 0)[:, None], acc / length[:, None], 0.0)


# ------------------------------------------------------------------------------------------------ shading
def _quantize(img, T):
    """[H, W, 3] -> uint8: surfel_vis_quantize's rule with scale 1 and bias 0 (tests/path_oracle.py states it in float32)"""
    if T is F32:
        return PO.quantize(np.ascontiguousarray(img.transpose(2, 0, 1)), 1.0, 0.0)
    y = np.where(np.isnan(img), 0.0, img)
    return (np.clip(y, 0.0, 1.0) * 255.0).astype(np.uint8)


def shade(key, verts, tris, colors, normals, w2c, intr, H, W, ssaa, mode, bg=(1.0, 1.0, 1.0), T=F32):
    """One view.  key [ssaa H, ssaa W] uint64; w2c [3 | 4, 4]; intr: (fx, fy, cx, cy) of the sample grid; colors / normals [V, 3] or
    None (grey 0.8 / flat).  Returns (uint8 [H, W, 3], the float frame before quantisation).  MESHVIEW.md §Shading numbers the steps."""
    s = int(ssaa)
    sH, sW = H * s, W * s
    key = np.asarray(key, np.uint64).reshape(sH, sW)
    tri = (key & np.uint64(0xffffffff)).astype(np.int64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    live = ((key >> np.uint64(32)) < INF_BITS) & (tri < len(t))
    bgc = np.asarray(bg, F32).astype(T)
    if not live.any():
        c = np.broadcast_to(bgc, (sH, sW, 3)).astype(T)
    else:
        tt = t[np.where(live, tri, 0)]
        live &= ((tt >= 0) & (tt < len(verts))).all(-1)
        tt = np.where(live[..., None], tt, 0)
        m = np.asarray(w2c, F32)[:3].astype(T)
        fx, fy, cx, cy = (T(F32(x)) for x in np.asarray(intr).reshape(-1)[:4])
        cam = O.camera_vertices(verts, np.asarray(w2c, F32)).astype(T)                                    # 1
        with np.errstate(all="ignore"):
            (X0, Y0, Z0), (X1, Y1, Z1), (X2, Y2, Z2) = ((cam[tt[..., k], 0], cam[tt[..., k], 1], cam[tt[..., k], 2]) for k in range(3))
            n0 = (Y1 * Z2 - Z1 * Y2, Z1 * X2 - X1 * Z2, X1 * Y2 - Y1 * X2)                                # 2
            n1 = (Y2 * Z0 - Z2 * Y0, Z2 * X0 - X2 * Z0, X2 * Y0 - Y2 * X0)
            n2 = (Y0 * Z1 - Z0 * Y1, Z0 * X1 - X0 * Z1, X0 * Y1 - Y0 * X1)
            det = (X0 * n0[0] + Y0 * n0[1]) + Z0 * n0[2]
            sg = np.where(det < 0, T(-1), T(1))
            ys, xs = np.meshgrid(np.arange(sH).astype(T), np.arange(sW).astype(T), indexing="ij")
            dx, dy = (xs - cx) / fx, (ys - cy) / fy                                                       # 3
            e = [sg * ((n[0] * dx + n[1] * dy) + n[2]) for n in (n0, n1, n2)]
            w = [np.where(x > 0, x, T(0)) for x in e]                                                     # 4
            ws = (w[0] + w[1]) + w[2]
            some = ws > 0
            lam = [np.where(some, x / ws, T(1) / T(3)) for x in w]
            f = [(n0[k] + n1[k]) + n2[k] for k in range(3)]                                               # 5
            flen = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
            fok = (flen > 0) & np.isfinite(flen)
            f = [np.where(fok, x / flen, T(0)) for x in f]
            flip = (f[0] * dx + f[1] * dy) + f[2] > 0
            f = [np.where(flip, -x, x) for x in f]
            nc = list(f)
            nw = [(m[0, k] * f[0] + m[1, k] * f[1]) + m[2, k] * f[2] for k in range(3)]
            if normals is not None:                                                                      # 6
                vn = np.asarray(normals, F32).astype(T)
                sm = [(lam[0] * vn[tt[..., 0], k] + lam[1] * vn[tt[..., 1], k]) + lam[2] * vn[tt[..., 2], k] for k in range(3)]
                slen = np.sqrt((sm[0] * sm[0] + sm[1] * sm[1]) + sm[2] * sm[2])
                sok = (slen > 0) & np.isfinite(slen)
                sw = [x / slen for x in sm]
                sc = [(m[r, 0] * sw[0] + m[r, 1] * sw[1]) + m[r, 2] * sw[2] for r in range(3)]
                sflip = (sc[0] * dx + sc[1] * dy) + sc[2] > 0
                sw = [np.where(sflip, -x, x) for x in sw]
                sc = [np.where(sflip, -x, x) for x in sc]
                nw = [np.where(sok, a, b) for a, b in zip(sw, nw)]
                nc = [np.where(sok, a, b) for a, b in zip(sc, nc)]
            if mode == "normal":
                c = np.stack([x * T(0.5) + T(0.5) for x in nw], -1)
            else:
                if colors is not None:                                                                   # 7
                    col = np.asarray(colors, F32).astype(T)
                    c = [(lam[0] * col[tt[..., 0], k] + lam[1] * col[tt[..., 1], k]) + lam[2] * col[tt[..., 2], k] for k in range(3)]
                else:
                    c = [np.full((sH, sW), T(F32(GREY)))] * 3
                if mode == "shaded":                                                                     # 8
                    dlen = np.sqrt((dx * dx + dy * dy) + T(1))
                    ndl = -((nc[0] * dx + nc[1] * dy) + nc[2]) / dlen
                    fac = T(F32(0.3)) + T(F32(0.7)) * np.where(ndl > 0, ndl, T(0))
                    c = [x * fac for x in c]
                elif mode != "color":
                    raise KeyError(mode)
                c = np.stack(c, -1)
        c = np.where(live[..., None], c, bgc).astype(T)
    c = c.reshape(H, s, W, s, 3)
    acc = np.zeros((H, W, 3), T)
    with np.errstate(all="ignore"):
        for ky in range(s):                                                                              # 9: row-major
            for kx in range(s):
                acc = acc + c[:, ky, :, kx]
        out = acc * (T(1) / T(s * s))
    assert out.dtype == T
    return _quantize(out, T), out


def shade_views(keys, verts, tris, colors, normals, w2c, intr, H, W, ssaa, mode, bg=(1.0, 1.0, 1.0), T=F32):
    """shade() over a batch: keys [n, ssaa H, ssaa W]; intr [1 | n, 4] of the sample grid"""
    k = np.asarray(intr, F32).reshape(-1, 4)
    return np.stack([shade(keys[i], verts, tris, colors, normals, w2c[i], k[0 if len(k) == 1 else i], H, W, ssaa, mode, bg, T)[0]
                     for i in range(len(keys))])


# ------------------------------------------------------------------------------------------------ undecided pixels
def close_pairs(verts, tris, w2c, intr, H, W, znear, zfar, margin=CLOSE):
    """bool [H, W]: another triangle's hit lies within `margin` (relative) of the nearest one.  fp64, every triangle against every pixel
    of a band of rows (triangles in front of the near plane whose projected rows, widened by cull_oracle.GUARD, miss the band are left out)."""
    cam = O.camera_vertices(verts, w2c)
    t, _ = O.valid_triangles(verts, tris, cam)
    fx, fy, cx, cy = (F64(F32(x)) for x in intr)
    zn, zf = F64(F32(znear)), F64(F32(zfar))
    c3 = cam[t].astype(F64)
    V0, V1, V2 = c3[:, 0], c3[:, 1], c3[:, 2]
    z3 = c3[:, :, 2]
    skip = (z3 < zn).all(1) | (z3 > zf).all(1)
    N0, N1, N2 = np.cross(V1, V2), np.cross(V2, V0), np.cross(V0, V1)
    DET = (V0 * N0).sum(1)
    NS = (N0 + N1) + N2
    use = (DET != 0) & np.isfinite(DET) & ~skip
    SG = np.where(DET < 0, -1.0, 1.0)
    front = (z3 >= zn).all(1)
    with np.errstate(all="ignore"):
        pv = fy * c3[:, :, 1] / z3 + cy
    vlo, vhi = np.where(front, pv.min(1) - O.GUARD, -np.inf), np.where(front, pv.max(1) + O.GUARD, np.inf)
    out = np.zeros((H, W), bool)
    band = 8
    for y0 in range(0, H, band):
        y1 = min(y0 + band, H)
        sel = np.nonzero(use & (vhi >= y0) & (vlo <= y1 - 1))[0]
        if len(sel) < 2:
            continue
        ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
        dx, dy = (xs.reshape(-1) - cx) / fx, (ys.reshape(-1) - cy) / fy
        sg = SG[sel][:, None]
        with np.errstate(all="ignore"):
            e = [sg * ((n[sel, 0:1] * dx[None] + n[sel, 1:2] * dy[None]) + n[sel, 2:3]) for n in (N0, N1, N2)]
            sden = sg * ((NS[sel, 0:1] * dx[None] + NS[sel, 1:2] * dy[None]) + NS[sel, 2:3])
            z = (sg * DET[sel][:, None]) / sden
            hit = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & (sden > 0) & (z >= zn) & (z <= zf)
        zz = np.where(hit, z, np.inf)
        zmin = zz.min(0)
        near = (zz <= zmin * (1 + margin)) & np.isfinite(zz)
        out[y0:y1] = (near.sum(0) >= 2).reshape(y1 - y0, W)
    return out


def view_reference(verts, tris, w2c, intr, H, W, znear, zfar):
    """One view on one sample grid: dict(tri64, tri32, depth32 — the twins' nearest triangles and the fp32 twin's depth — und: undecided by
    cull_oracle's rule, by the twins disagreeing, or by a close pair; own, close: the two parts)"""
    _, a64, u64 = O.depth_image(verts, tris, w2c, intr, H, W, znear, zfar, np.float64)
    d32, a32, _ = O.depth_image(verts, tris, w2c, intr, H, W, znear, zfar, np.float32)
    own = u64 | (a64 != a32)
    close = close_pairs(verts, tris, w2c, intr, H, W, znear, zfar)
    return {"tri64": a64, "tri32": a32, "depth32": d32.astype(F32), "und": own | close, "own": own, "close": close}


@functools.lru_cache(maxsize=None)
def scene_reference(size, ssaa=1, views=None):
    """The scene of tests/cull_scenes.py at one image size and one supersampling factor, computed once and left unchanged: per view the
    twins' nearest triangles on the sample grid and the undecided samples.  views: a tuple of view numbers (None: all)."""
    import cull_scenes as S
    ref = O.scene_reference(size)
    H, W = ref["H"], ref["W"]
    k = scaled_intrinsics(ref["intr"], ssaa)[0]
    ids = tuple(range(len(ref["w2c"]))) if views is None else tuple(views)
    per = [view_reference(ref["verts"], ref["tris"], ref["w2c"][i], k, H * ssaa, W * ssaa, S.SCENE["znear"], S.SCENE["zfar"]) for i in ids]
    out = {name: np.stack([p[name] for p in per]) for name in per[0]}
    und = out["und"].reshape(len(ids), H, ssaa, W, ssaa).any((2, 4))      # a pixel is undecided when one of its samples is
    out.update(verts=ref["verts"], tris=ref["tris"], colors=ref["colors"], w2c=ref["w2c"][list(ids)], intr=ref["intr"], sample_intr=k, H=H, W=W,
               ssaa=ssaa, views=ids, pixel_und=und, normals32=vertex_normals(ref["verts"], ref["tris"]),
               normals64=vertex_normals64(ref["verts"], ref["tris"]))
    return out


# ------------------------------------------------------------------------------------------------ the anchor in closed form
def anchor_colors(verts, A, b):
    """vertex colours that are an affine function of position: c = A p + b"""
    return (np.asarray(verts, F64) @ np.asarray(A, F64).T + np.asarray(b, F64)).astype(F32)


def anchor_frames(n, d, A, b, intr, H, W):
    """(colour frame, normal frame) in float64 for the plane n . p = d under an identity camera: at every pixel the ray
    r = ((x - cx) / fx, (y - cy) / fy, 1) meets the plane at p = (d / (n . r)) r, where the colour is A p + b; the normal is the plane's,
    oriented to the camera (n . r > 0 turns it round), written as 0.5 n + 0.5."""
    fx, fy, cx, cy = (F64(F32(x)) for x in intr)
    xs, ys = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    r = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)
    nr = r @ np.asarray(n, F64)
    p = (d / nr)[..., None] * r
    color = p @ np.asarray(A, F64).T + np.asarray(b, F64)
    unit = np.asarray(n, F64) / np.linalg.norm(n)
    normal = np.where((nr > 0)[..., None], -unit, unit) * 0.5 + 0.5
    return color, normal
