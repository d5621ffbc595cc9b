"""numpy oracles of the view culling (CULL.md): a brute-force ray / triangle depth oracle (every triangle against every pixel, no boxes, no
classes) in fp64 with an fp32 twin that is the same code in float32, and a literal restatement of the reference's Mesher.point_masks
(scripts/eval_tnt/cull_mesh.py:96-182) in fp32.  Both also say which of their answers are *undecided*: so close to a decision boundary
that fp32 code with another operation order may decide the other way."""
import numpy as np

M_EDGE = 1e-4          # a near-hit: every normalised edge value >= -M_EDGE and the smallest < M_EDGE
M_RANGE = 1e-4         # a hit within this relative distance of znear / zfar
M_BEHIND = 1e-3        # a near-hit this far (relative) behind a clear hit decides nothing
SMALL_PIXELS = 32      # SURFEL_CULL_SMALL_PIXELS


def camera_vertices(verts, w2c):
    """fp32 camera-space vertices as the kernels compute them: ((r0 x + r1 y) + r2 z) + r3 per row."""
    v, m = np.asarray(verts, np.float32), np.asarray(w2c, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3)], 1)


def valid_triangles(verts, tris, cam):
    """the triangles the depth rule keeps: indices inside [0, V) and finite camera-space coordinates"""
    t = np.asarray(tris, np.int64)
    ok = ((t >= 0) & (t < len(verts))).all(1)
    fin = np.isfinite(cam).all(1)
    ok[ok] &= fin[t[ok]].all(1)
    return t[ok], np.nonzero(ok)[0]


TILE = 8               # the depth oracle walks the image in TILE x TILE pixel tiles
GUARD = 3.0            # pixels by which a triangle's fp64 projected box is widened before it is matched against a tile


def depth_image(verts, tris, w2c, intr, H, W, znear, zfar, dtype=np.float64):
    """(depth [H, W] in dtype with 0 where nothing is hit, nearest triangle [H, W] (-1: none), undecided [H, W] bool — the near-hit and
    range rules, evaluated in dtype) of one view.  With camera-space v0, v1, v2: n0 = v1 x v2, n1 = v2 x v0, n2 = v0 x v1, det = v0 . n0,
    d = ((x - cx) / fx, (y - cy) / fy, 1); a hit iff det != 0, every ni . d is zero or has det's sign and N . d / det > 0 with
    N = (n0 + n1) + n2; then z = det / (N . d), kept when znear <= z <= zfar.  Brute force: a pixel meets every triangle that crosses
    z = znear, and every other triangle whose projected box (fp64), widened by GUARD pixels, touches the pixel's tile."""
    T = dtype
    cam = camera_vertices(verts, w2c)
    t, ids = valid_triangles(verts, tris, cam)
    fx, fy, cx, cy = (T(np.float32(x)) for x in intr)
    zn, zf = T(np.float32(znear)), T(np.float32(zfar))
    V0, V1, V2 = (cam[t[:, k]].astype(T) for k in range(3))
    skip = ((V0[:, 2] < zn) & (V1[:, 2] < zn) & (V2[:, 2] < zn)) | ((V0[:, 2] > zf) & (V1[:, 2] > zf) & (V2[:, 2] > zf))
    N0, N1, N2 = np.cross(V1, V2), np.cross(V2, V0), np.cross(V0, V1)
    DET = (V0[:, 0] * N0[:, 0] + V0[:, 1] * N0[:, 1]) + V0[:, 2] * N0[:, 2]
    NS = (N0 + N1) + N2
    use = (DET != 0) & np.isfinite(DET) & ~skip
    SG = np.where(DET < 0, T(-1), T(1))
    # which triangles a tile meets (always in fp64, from the fp32 camera-space vertices)
    c3 = cam[t].astype(np.float64)
    front = (c3[:, :, 2] >= float(zn)).all(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pu = float(fx) * c3[:, :, 0] / c3[:, :, 2] + float(cx)
        pv = float(fy) * c3[:, :, 1] / c3[:, :, 2] + float(cy)
    ulo, uhi = np.where(front, pu.min(1) - GUARD, -np.inf), np.where(front, pu.max(1) + GUARD, np.inf)
    vlo, vhi = np.where(front, pv.min(1) - GUARD, -np.inf), np.where(front, pv.max(1) + GUARD, np.inf)
    depth = np.zeros((H, W), T)
    arg = np.full((H, W), -1, np.int64)
    und = np.zeros((H, W), bool)
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            ys, xs = np.meshgrid(np.arange(ty, min(ty + TILE, H)), np.arange(tx, min(tx + TILE, W)), indexing="ij")
            sel = np.nonzero(use & (uhi >= tx) & (ulo <= xs.max()) & (vhi >= ty) & (vlo <= ys.max()))[0]
            if not len(sel):
                continue
            dx, dy = ((xs.reshape(-1).astype(T) - cx) / fx), ((ys.reshape(-1).astype(T) - cy) / fy)
            sg = SG[sel][:, None]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                e = [sg * ((n[sel, 0:1] * dx[None] + n[sel, 1:2] * dy[None]) + n[sel, 2:3]) for n in (N0, N1, N2)]
                s = sg * ((NS[sel, 0:1] * dx[None] + NS[sel, 1:2] * dy[None]) + NS[sel, 2:3])
                z = (sg * DET[sel][:, None]) / s
                inside = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & (s > 0)
                hit = inside & (z >= zn) & (z <= zf)
                norm = np.abs(e[0]) + np.abs(e[1]) + np.abs(e[2])
                lo = np.minimum(np.minimum(e[0], e[1]), e[2]) / norm
                near = (s > 0) & (lo >= -M_EDGE) & (lo < M_EDGE) & (z >= zn * (1 - M_RANGE)) & (z <= zf * (1 + M_RANGE))
                edge = inside & ((np.abs(z - zn) <= M_RANGE * zn) | (np.abs(z - zf) <= M_RANGE * zf))
            zz = np.where(hit, z, np.inf)
            k = zz.argmin(0)
            zb = zz[k, np.arange(zz.shape[1])]
            got = np.isfinite(zb)
            depth[ys.reshape(-1), xs.reshape(-1)] = np.where(got, zb, 0)
            arg[ys.reshape(-1), xs.reshape(-1)] = np.where(got, ids[sel[k]], -1)
            # a near-hit that lies behind a hit that is none (by more than M_BEHIND, relative) cannot change the minimum
            sure = np.where(hit & ~near, z, np.inf).min(0)
            und[ys.reshape(-1), xs.reshape(-1)] = (near & (z <= sure * (1 + M_BEHIND))).any(0) | edge.any(0)
    return depth, arg, und


def depth_images(verts, tris, w2c, intr, H, W, znear, zfar):
    """All views, both twins: (fp64 depth [V, H, W], fp32 twin's depth, undecided [V, H, W]: the rules of depth_image in fp64, or the
    nearest triangle differs between the twins, or one twin hits and the other does not)."""
    d64, d32, und = [], [], []
    for m in np.asarray(w2c, np.float32):
        a, ia, ua = depth_image(verts, tris, m, intr, H, W, znear, zfar, np.float64)
        b, ib, _ = depth_image(verts, tris, m, intr, H, W, znear, zfar, np.float32)
        d64.append(a); d32.append(b); und.append(ua | (ia != ib))
    return np.stack(d64), np.stack(d32), np.stack(und)


def twin_deviation(d64, d32, und):
    """the largest relative deviation of the fp32 twin from the fp64 oracle over decided, covered pixels"""
    ok = ~und & (d64 > 0)
    return float(np.max(np.abs(d32[ok].astype(np.float64) - d64[ok]) / d64[ok])) if ok.any() else 0.0


def size_classes(verts, tris, w2c, intr, H, W, znear, zfar, small_pixels=SMALL_PIXELS):
    """(small, large): the (view, triangle) pairs per class under the kernel's box rule — all z >= znear: the projected box, one pixel
    wider on every side, clamped; crossing znear: the whole image; skipped triangles and empty boxes count in neither."""
    fx, fy, cx, cy = (np.float32(x) for x in intr)
    small = large = 0
    for m in np.asarray(w2c, np.float32):
        cam = camera_vertices(verts, m)
        t, _ = valid_triangles(verts, tris, cam)
        v = cam[t]                                    # [F, 3, 3]
        z = v[:, :, 2]
        skip = (z < znear).all(1) | (z > zfar).all(1)
        front = (z >= znear).all(1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            u, w = fx * (v[:, :, 0] / z) + cx, fy * (v[:, :, 1] / z) + cy
        x0 = np.maximum(np.ceil(np.clip(u.min(1), -2, W + 1)) - 1, 0); x1 = np.minimum(np.floor(np.clip(u.max(1), -2, W + 1)) + 1, W - 1)
        y0 = np.maximum(np.ceil(np.clip(w.min(1), -2, H + 1)) - 1, 0); y1 = np.minimum(np.floor(np.clip(w.max(1), -2, H + 1)) + 1, H - 1)
        area = np.where(front, np.maximum(x1 - x0 + 1, 0) * np.maximum(y1 - y0 + 1, 0), H * W)
        area = np.where(skip, 0, np.nan_to_num(area))
        small += int(((area > 0) & (area <= small_pixels)).sum())
        large += int((area > small_pixels).sum())
    return small, large


# ------------------------------------------------------------------------------------------------ Mesher.point_masks
def point_masks(points, depth, w2c, intr, eps=0.005, min_views=20, pixel_undecided=None):
    """cull_mesh.py:96-182 in fp32 numpy, operation by operation.  points [N, 3]; depth [V, H, W]; w2c [V, 4, 4] fp32 (the inverse of the
    OpenCV pose).  Returns a dict: valid [V, N] (in the frustum and in front), counts [N], mask [N] (counts >= min_views), undecided_pairs
    [V, N], undecided [N] (flipping its undecided pairs can move the count across min_views)."""
    f = np.float32
    p = np.asarray(points, f)
    depth = np.asarray(depth, f)
    V, H, W = depth.shape
    fx, fy, cx, cy = (f(x) for x in intr)
    wm, hm = f(W - 1), f(H - 1)
    valid = np.zeros((V, len(p)), bool)
    undp = np.zeros((V, len(p)), bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(V):
            m = np.asarray(w2c[i], f)
            X, Y, Z = (((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3))
            z = Z + f(1e-8)
            u, v = (fx * X + cx * Z) / z, (fy * Y + cy * Z) / z
            frustum = (u >= 0) & (u <= wm) & (v >= 0) & (v <= hm) & (z > 0)
            # grid_sample(depth, grid, padding_mode='border', align_corners=True)
            gx, gy = u / wm * f(2) - f(1), v / hm * f(2) - f(1)
            ix, iy = ((gx + f(1)) / f(2)) * wm, ((gy + f(1)) / f(2)) * hm
            ix, iy = np.minimum(wm, np.maximum(ix, f(0))), np.minimum(hm, np.maximum(iy, f(0)))
            ix, iy = np.where(frustum, ix, f(0)), np.where(frustum, iy, f(0))       # (outside the frustum the sample decides nothing)
            x0f, y0f = np.floor(ix), np.floor(iy)
            x1f, y1f = x0f + f(1), y0f + f(1)
            nw, ne, sw, se = (x1f - ix) * (y1f - iy), (ix - x0f) * (y1f - iy), (x1f - ix) * (iy - y0f), (ix - x0f) * (iy - y0f)
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            x1, y1 = x0 + 1, y0 + 1
            img = depth[i]

            def tap(yy, xx):
                inb = (xx < W) & (yy < H)
                return np.where(inb, img[np.minimum(yy, H - 1), np.minimum(xx, W - 1)], f(0)), inb

            sample = np.zeros(len(p), f)
            corner_und = np.zeros(len(p), bool)
            for (yy, xx), wgt in (((y0, x0), nw), ((y0, x1), ne), ((y1, x0), sw), ((y1, x1), se)):
                val, inb = tap(yy, xx)
                sample = np.where(inb, sample + val * wgt, sample)
                if pixel_undecided is not None:
                    corner_und |= inb & pixel_undecided[i][np.minimum(yy, H - 1), np.minimum(xx, W - 1)]
            front = np.where(sample > 0, z < sample + f(eps), True)
            valid[i] = frustum & front
            near_bound = (np.abs(u) < 1e-3) | (np.abs(u - wm) < 1e-3) | (np.abs(v) < 1e-3) | (np.abs(v - hm) < 1e-3) | (np.abs(z) < 1e-6)
            near_front = frustum & ((np.abs(z.astype(np.float64) - (sample.astype(np.float64) + eps)) < 1e-4 * np.maximum(1.0, z)) | (np.abs(sample) < 1e-6))
            undp[i] = (np.isfinite(u) & np.isfinite(v) & near_bound) | near_front | (frustum & corner_und)
    counts = valid.sum(0).astype(np.int32)
    lo = (valid & ~undp).sum(0)
    hi = lo + undp.sum(0)
    return {"valid": valid, "counts": counts, "mask": counts >= min_views, "undecided_pairs": undp, "undecided": (lo < min_views) & (hi >= min_views)}


def compact(verts, tris, keep, colors=None):
    """Mesher.cull_mesh's tail (cull_mesh.py:246-249) in plain loops: the triangles whose three vertices are kept, then the vertices some kept
    triangle uses, in their order.  Triangles with an index outside the vertices are dropped first."""
    new_t, used = [], set()
    for t in np.asarray(tris, np.int64).tolist():
        if all(0 <= i < len(verts) for i in t) and all(keep[i] for i in t):
            new_t.append(t)
            used.update(t)
    order = sorted(used)
    remap = {old: new for new, old in enumerate(order)}
    v = np.asarray(verts)[order].reshape(-1, 3)
    c = None if colors is None else np.asarray(colors)[order].reshape(-1, 3)
    return v, np.array([[remap[i] for i in t] for t in new_t], np.int32).reshape(-1, 3), c


# ------------------------------------------------------------------------------------------------ the scene's references, computed once
import functools  # noqa: E402


def world_to_camera(c2w_opencv):
    """fp32 inverse of every pose, by torch on the host as the reference inverts them (cull_mesh.py:139)"""
    import torch
    return np.stack([torch.inverse(torch.from_numpy(np.asarray(m, np.float32))).numpy() for m in c2w_opencv])


@functools.lru_cache(maxsize=None)
def scene_reference(size, special=True):
    """Everything the tests compare against at one image size of tests/cull_scenes.py: the mesh, w2c, the intrinsics, both twins' depth
    images, the undecided pixels, and per min_views the point-mask oracle on the fp32 image of the fp64 depth."""
    import cull_scenes as S
    v, t, c = S.mesh(special)
    H, W = S.SIZES[size][:2]
    k = S.intrinsics(size)
    w2c = world_to_camera(S.cameras())
    zn, zf, eps = S.SCENE["znear"], S.SCENE["zfar"], S.SCENE["eps"]
    d64, d32, und = depth_images(v, t, w2c, k, H, W, zn, zf)
    masks = {mv: point_masks(v, d64.astype(np.float32), w2c, k, eps, mv, und) for mv in S.MIN_VIEWS}
    return {"verts": v, "tris": t, "colors": c, "H": H, "W": W, "intr": k, "w2c": w2c, "d64": d64, "d32": d32, "und": und, "masks": masks,
            "deviation": twin_deviation(d64, d32, und)}
