"""numpy restatement of the mesh texturing (TEXTURE.md; include/surfel_texture.h): the atlas layout, the baking, the resolve and the
textured shading, fp32 where the device is fp32, operation for operation, vectorised over triangles or texels with a plain loop over the
views.  What the device must equal bit for bit; tests/test_texture_cpu.py checks it against closed forms that share nothing with it."""
import numpy as np

F32 = np.float32
CLASSES, MIN_LOG2, PAD, MAX_SIDE = 6, 2, 4, 16384
AVERAGE, BEST = 0, 1
GREY = 0.8
INF_BITS = 0x7f800000


class LimitError(RuntimeError):
    pass


def legs(c):
    return 1 << (c + MIN_LOG2)


# ------------------------------------------------------------------------------------------------ triangles
def triangles(verts, tris):
    """Per triangle: ok (it gets a patch), corner (which corner sits at the right angle), idx [F, 3] and pts [F, 3, 3] in patch order
    (a, b, c), normal [F, 3] (unit, fp32), longest2 (the squared longest edge)."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(1)
    ts = np.where(ok[:, None], t, 0)
    p = v[ts] if len(v) else np.zeros((len(t), 3, 3), F32)
    with np.errstate(all="ignore"):
        ok &= np.isfinite(p).all((1, 2))
        u, w, e = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 2] - p[:, 1]
        f = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        length = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        ok &= np.isfinite(length) & (length > 0)
        normal = f / length[:, None]
        sq = lambda d: (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        e0, e1, e2 = sq(e), sq(w), sq(u)      # edge k lies opposite corner k
    corner = np.zeros(len(t), np.int64)
    m = e0.copy()
    with np.errstate(invalid="ignore"):
        g = e1 > m
        corner[g], m[g] = 1, e1[g]
        g = e2 > m
        corner[g], m[g] = 2, e2[g]
    rot = (corner[:, None] + np.arange(3)[None]) % 3
    rows = np.arange(len(t))[:, None]
    assert normal.dtype == F32 and m.dtype == F32
    return {"ok": ok, "corner": corner, "idx": ts[rows, rot], "pts": p[rows, rot], "normal": normal, "longest2": m}


def classify(verts, tris, density):
    """(cls int32 [F], counts [6])"""
    tr = triangles(verts, tris)
    with np.errstate(all="ignore"):
        s = np.sqrt(tr["longest2"]) * F32(density)
        c = sum((s > F32(1 << k)).astype(np.int32) for k in range(MIN_LOG2, MIN_LOG2 + CLASSES - 1))
    assert s.dtype == F32
    cls = np.where(tr["ok"], c, -1).astype(np.int32)
    return cls, [int((cls == k).sum()) for k in range(CLASSES)]


def band_table(counts, Wa):
    """(table int32 [6, 4] = (y0, cells per row, first, count) per class, Ha): bands largest class first"""
    if Wa > MAX_SIDE:
        raise LimitError("width")
    table = np.zeros((CLASSES, 4), np.int32)
    y = first = 0
    for c in range(CLASSES - 1, -1, -1):
        cell = legs(c) + PAD
        per = Wa // cell
        table[c] = (y, per, first, counts[c])
        if counts[c]:
            if per < 1:
                raise LimitError("narrow")
            cells = (counts[c] + 1) // 2
            y += (cells + per - 1) // per * cell
            first += counts[c]
            if y > MAX_SIDE:
                raise LimitError("height")
    return table, max(y, 1)


def layout(verts, tris, density, Wa):
    """dict(cls, counts, table, Ha, Wa, order [sum counts], uv [F, 3, 2] fp32, tri: triangles())"""
    tr = triangles(verts, tris)
    cls, counts = classify(verts, tris, density)
    table, Ha = band_table(counts, Wa)
    F = len(cls)
    order = np.concatenate([np.nonzero(cls == c)[0] for c in range(CLASSES - 1, -1, -1)]).astype(np.int64) if F else np.zeros(0, np.int64)
    uv = np.zeros((F, 3, 2), F32)
    for c in range(CLASSES):
        ids = np.nonzero(cls == c)[0]      # triangle order is rank order
        if not len(ids):
            continue
        y0, per = int(table[c, 0]), int(table[c, 1])
        n = legs(c)
        cell = n + PAD
        rank = np.arange(len(ids))
        cellidx, half = rank // 2, rank % 2
        ox, oy = (cellidx % per) * cell, y0 + (cellidx // per) * cell
        a = np.where(half[:, None] == 1, np.stack([ox + cell - 2, oy + cell - 2], 1), np.stack([ox, oy], 1)).astype(F32)
        sign = np.where(half == 1, F32(-1), F32(1)).astype(F32)
        b = a + np.stack([sign * F32(n), np.zeros(len(ids), F32)], 1)
        cc = a + np.stack([np.zeros(len(ids), F32), sign * F32(n)], 1)
        k = tr["corner"][ids]
        uv[ids, k], uv[ids, (k + 1) % 3], uv[ids, (k + 2) % 3] = a, b, cc
    return {"cls": cls, "counts": counts, "table": table, "Ha": Ha, "Wa": Wa, "order": order, "uv": uv, "tri": tr, "density": density}


def owners(lay, Ha=None):
    """Per texel of the atlas [Ha, Wa]: tri (-1: unowned), n, du, dv (the patch coordinates before clamping) — band by y, cell, half,
    rank, triangle through `order`, as the kernels go"""
    Wa = lay["Wa"]
    Ha = lay["Ha"] if Ha is None else Ha
    ys, xs = np.meshgrid(np.arange(Ha), np.arange(Wa), indexing="ij")
    tri = -np.ones((Ha, Wa), np.int64)
    nn, du, dv = (np.zeros((Ha, Wa), np.int64) for _ in range(3))
    for c in range(CLASSES):
        y0, per, first, count = (int(x) for x in lay["table"][c])
        if not count:
            continue
        n = legs(c)
        cell = n + PAD
        rows = ((count + 1) // 2 + per - 1) // per
        inband = (ys >= y0) & (ys < y0 + rows * cell)
        row, ly, col, lx = (ys - y0) // cell, (ys - y0) % cell, xs // cell, xs % cell
        half = (lx + ly > n + 2).astype(np.int64)
        rank = 2 * (row * per + col) + half
        own = inband & (col < per) & (rank < count)
        tri[own] = lay["order"][first + rank[own]]
        nn[own] = n
        du[own] = np.where(half == 1, cell - 2 - lx, lx)[own]
        dv[own] = np.where(half == 1, cell - 2 - ly, ly)[own]
    tri[tri >= 0] = np.where(lay["tri"]["ok"][tri[tri >= 0]], tri[tri >= 0], -1)
    return tri, nn, du, dv


def bary(n, du, dv):
    """fp32 barycentrics (of a, b, c) of patch coordinates, clamped into the triangle"""
    fn = np.asarray(n).astype(F32)
    a = np.minimum(np.maximum(np.asarray(du).astype(F32), F32(0)), fn)
    b = np.minimum(np.maximum(np.asarray(dv).astype(F32), F32(0)), fn)
    s = a + b
    over = s > fn
    h = (s - fn) * F32(0.5)
    a2, b2 = np.where(over, a - h, a), np.where(over, b - h, b)
    neg = over & (a2 < 0)
    a2, b2 = np.where(neg, F32(0), a2), np.where(neg, fn, b2)
    neg = over & (b2 < 0)
    b2, a2 = np.where(neg, F32(0), b2), np.where(neg, fn, a2)
    with np.errstate(all="ignore"):
        b1, bb2 = a2 / fn, b2 / fn
    b0 = (F32(1) - b1) - bb2
    assert b0.dtype == F32
    return b0, b1, bb2


def texel_points(lay, Ha=None):
    """(owned [Ha, Wa] bool, tri, (b0, b1, b2), p [Ha, Wa, 3] fp32: the point of every owned texel)"""
    tri, n, du, dv = owners(lay, Ha)
    owned = tri >= 0
    ts = np.where(owned, tri, 0)
    b0, b1, b2 = bary(np.where(owned, n, 1), du, dv)
    pts = lay["tri"]["pts"][ts] if len(lay["tri"]["pts"]) else np.zeros(ts.shape + (3, 3), F32)
    with np.errstate(all="ignore"):
        p = (b0[..., None] * pts[..., 0, :] + b1[..., None] * pts[..., 1, :]) + b2[..., None] * pts[..., 2, :]
    assert p.dtype == F32
    return owned, ts, (b0, b1, b2), p


# ------------------------------------------------------------------------------------------------ baking
def _corners(img, x0, y0, nw, ne, sw, se):
    H, W = img.shape
    x1, y1 = x0 + 1, y0 + 1
    s = np.zeros(x0.shape, F32)
    for yy, xx, wgt in ((y0, x0, nw), (y0, x1, ne), (y1, x0, sw), (y1, x1, se)):
        inb = (xx < W) & (yy < H)
        s = np.where(inb, s + img[np.minimum(yy, H - 1), np.minimum(xx, W - 1)] * wgt, s)
    assert s.dtype == F32
    return s


def bake(lay, acc, w2c, intr, depth, images, eps=0.005, cos_min=0.1, power=2, blend=AVERAGE, points=None):
    """acc [Ha, Wa, 4] fp32 combined with the views in view order; returns the new accumulator.  w2c [n, 3 | 4, 4]; intr [1 | n, 4];
    depth [n, H, W]; images [n, 3, H, W]."""
    f = F32
    acc = np.array(acc, F32)
    Ha = acc.shape[0]
    owned, ts, _, p = points if points is not None else texel_points(lay, Ha)
    sel = np.nonzero(owned)
    P = p[sel]
    nrm = lay["tri"]["normal"][ts[sel]]
    a = acc[sel]
    depth, images = np.asarray(depth, f), np.asarray(images, f)
    K = np.asarray(intr, f).reshape(-1, 4)
    nv, H, W = depth.shape
    wm, hm = f(W - 1), f(H - 1)
    with np.errstate(all="ignore"):
        for i in range(nv):
            m = np.asarray(w2c[i], f)[:3]
            fx, fy, cx, cy = K[0 if len(K) == 1 else i]
            X, Y, Z = (((m[r, 0] * P[:, 0] + m[r, 1] * P[:, 1]) + m[r, 2] * P[:, 2]) + m[r, 3] for r in range(3))
            zz = Z + f(1e-8)
            u, v = (fx * X + cx * Z) / zz, (fy * Y + cy * Z) / zz
            live = (u >= 0) & (u <= wm) & (v >= 0) & (v <= hm) & (zz > 0)
            gx, gy = u / wm * f(2) - f(1), v / hm * f(2) - f(1)
            ix, iy = ((gx + f(1)) / f(2)) * wm, ((gy + f(1)) / f(2)) * hm
            ix, iy = np.minimum(wm, np.maximum(ix, f(0))), np.minimum(hm, np.maximum(iy, f(0)))
            ix, iy = np.where(live, ix, f(0)), np.where(live, iy, f(0))
            x0f, y0f = np.floor(ix), np.floor(iy)
            x1f, y1f = x0f + f(1), y0f + f(1)
            nw, ne, sw, se = (x1f - ix) * (y1f - iy), (ix - x0f) * (y1f - iy), (x1f - ix) * (iy - y0f), (ix - x0f) * (iy - y0f)
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            sample = _corners(depth[i], x0, y0, nw, ne, sw, se)
            live &= np.where(sample > 0, zz < sample + f(eps), True)
            nc = [(m[r, 0] * nrm[:, 0] + m[r, 1] * nrm[:, 1]) + m[r, 2] * nrm[:, 2] for r in range(3)]
            cs = np.abs((nc[0] * X + nc[1] * Y) + nc[2] * Z) / np.sqrt((X * X + Y * Y) + Z * Z)
            live &= cs >= f(cos_min)
            cp = cs
            for _ in range(1, power):
                cp = cp * cs
            w = cp / (zz * zz)
            col = np.stack([_corners(images[i, k], x0, y0, nw, ne, sw, se) for k in range(3)], 1)
            assert w.dtype == f and col.dtype == f
            if blend == AVERAGE:
                new = np.concatenate([a[:, :3] + w[:, None] * col, (a[:, 3] + w)[:, None]], 1)
            else:
                live &= w > a[:, 3]
                new = np.concatenate([col, w[:, None]], 1)
            a = np.where(live[:, None], new, a).astype(f)
    acc[sel] = a
    return acc


def quantize(x):
    """surfel_vis_quantize with scale 1, bias 0"""
    with np.errstate(all="ignore"):
        y = np.asarray(x, F32) * F32(1) + F32(0)
        y = np.where(np.isnan(y), F32(0), y)
        y = np.minimum(np.maximum(y, F32(0)), F32(1))
        return (y * F32(255)).astype(np.int32).astype(np.uint8)


def resolve(lay, acc, colors=None, blend=AVERAGE, bg=(0.0, 0.0, 0.0), points=None):
    """(atlas uint8 [Ha, Wa, 3], float colours [Ha, Wa, 3], owned count, seen count)"""
    acc = np.asarray(acc, F32)
    Ha = acc.shape[0]
    owned, ts, (b0, b1, b2), _ = points if points is not None else texel_points(lay, Ha)
    seen = owned & (acc[..., 3] > 0)
    with np.errstate(all="ignore"):
        got = acc[..., :3] / acc[..., 3:4] if blend == AVERAGE else acc[..., :3]
        if colors is not None:
            c = np.asarray(colors, F32)[lay["tri"]["idx"][ts]]
            fall = (b0[..., None] * c[..., 0, :] + b1[..., None] * c[..., 1, :]) + b2[..., None] * c[..., 2, :]
        else:
            fall = np.full(acc.shape[:2] + (3,), F32(GREY), F32)
    out = np.where(seen[..., None], got, np.where(owned[..., None], fall, np.asarray(bg, F32))).astype(F32)
    return quantize(out), out, int(owned.sum()), int(seen.sum())


# ------------------------------------------------------------------------------------------------ textured shading
def shade(key, verts, tris, uv, atlas, w2c, intr, H, W, ssaa, bg=(1.0, 1.0, 1.0)):
    """uint8 [H, W, 3] of one view's keys [ssaa H, ssaa W] (uint64): MESHVIEW.md §Shading steps 1-4 and 9, the colour from the atlas"""
    T = F32
    s = int(ssaa)
    sH, sW = H * s, W * s
    key = np.asarray(key).astype(np.uint64).reshape(sH, sW)
    tri = (key & np.uint64(0xffffffff)).astype(np.int64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    v = np.asarray(verts, T)
    atlas = np.asarray(atlas, np.uint8)
    Ha, Wa = atlas.shape[:2]
    live = ((key >> np.uint64(32)) < INF_BITS) & (tri < len(t))
    bgc = np.asarray(bg, T)
    tt = t[np.where(live, tri, 0)] if len(t) else np.zeros((sH, sW, 3), np.int64)
    live &= ((tt >= 0) & (tt < len(v))).all(-1)
    tt = np.where(live[..., None], tt, 0)
    m = np.asarray(w2c, T)[:3]
    fx, fy, cx, cy = (T(x) for x in np.asarray(intr, T).reshape(-1)[:4])
    with np.errstate(all="ignore"):
        cam = np.stack([((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3)], 1)
        (X0, Y0, Z0), (X1, Y1, Z1), (X2, Y2, Z2) = ((cam[tt[..., k], 0], cam[tt[..., k], 1], cam[tt[..., k], 2]) for k in range(3))
        n0 = (Y1 * Z2 - Z1 * Y2, Z1 * X2 - X1 * Z2, X1 * Y2 - Y1 * X2)
        n1 = (Y2 * Z0 - Z2 * Y0, Z2 * X0 - X2 * Z0, X2 * Y0 - Y2 * X0)
        n2 = (Y0 * Z1 - Z0 * Y1, Z0 * X1 - X0 * Z1, X0 * Y1 - Y0 * X1)
        det = (X0 * n0[0] + Y0 * n0[1]) + Z0 * n0[2]
        sg = np.where(det < 0, T(-1), T(1))
        ys, xs = np.meshgrid(np.arange(sH).astype(T), np.arange(sW).astype(T), indexing="ij")
        dx, dy = (xs - cx) / fx, (ys - cy) / fy
        e = [sg * ((n[0] * dx + n[1] * dy) + n[2]) for n in (n0, n1, n2)]
        w = [np.where(x > 0, x, T(0)) for x in e]
        ws = (w[0] + w[1]) + w[2]
        lam = [np.where(ws > 0, x / ws, T(1) / T(3)) for x in w]
        q = np.asarray(uv, T).reshape(-1, 3, 2)[np.where(live, tri, 0)] if len(t) else np.zeros((sH, sW, 3, 2), T)
        u = (lam[0] * q[..., 0, 0] + lam[1] * q[..., 1, 0]) + lam[2] * q[..., 2, 0]
        vv = (lam[0] * q[..., 0, 1] + lam[1] * q[..., 1, 1]) + lam[2] * q[..., 2, 1]
        u = np.minimum(np.where(np.isnan(u), T(0), np.maximum(u, T(0))), T(Wa - 1))
        vv = np.minimum(np.where(np.isnan(vv), T(0), np.maximum(vv, T(0))), T(Ha - 1))
        x0f, y0f = np.floor(u), np.floor(vv)
        x1f, y1f = x0f + T(1), y0f + T(1)
        nw, ne, sw, se = (x1f - u) * (y1f - vv), (u - x0f) * (y1f - vv), (x1f - u) * (vv - y0f), (u - x0f) * (vv - y0f)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tex = atlas.astype(T) / T(255)
        c = np.stack([_corners(tex[..., k], x0, y0, nw, ne, sw, se) for k in range(3)], -1)
    c = np.where(live[..., None], c, bgc).astype(T).reshape(H, s, W, s, 3)
    acc = np.zeros((H, W, 3), T)
    for ky in range(s):
        for kx in range(s):
            acc = acc + c[:, ky, :, kx]
    out = acc * (T(1) / T(s * s))
    assert out.dtype == T
    return quantize(out)


# ------------------------------------------------------------------------------------------------ the density search
def bisect_ok(probe, size, density, above):
    """the end condition of surfel_texture.bisect_density: `density` fits size x size; `above` (when there is one) does not"""
    def fits(d):
        try:
            return band_table(probe(d), size)[1] <= size
        except LimitError:
            return False
    return fits(density) and (above is None or (above > density and not fits(above)))
