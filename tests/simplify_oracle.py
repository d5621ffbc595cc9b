"""The numpy restatement of the mesh simplification (SIMPLIFY.md §Rules, §Operation order): fp32 for the cell index, fp64 for everything
else, np.add.at for the ordered sums (it accumulates one term at a time in the order of its index array), stable argsorts for the sorts.
Rule for rule and operation for operation what csrc/mesh_simplify.hip does; the device's result must equal this one bit for bit."""
import numpy as np

AXIS_BITS = 21
N_MAX = 1 << 20


class LimitError(ValueError):
    pass


def bounds(verts):
    """(lo, hi) of the vertices whose three coordinates are finite, or None"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    fin = np.isfinite(verts).all(1)
    if not fin.any():
        return None
    return verts[fin].min(0), verts[fin].max(0)


def cell_indices(verts, origin, cell):
    """rule 2: (index [V, 3] int64, finite [V]); raises LimitError when a finite vertex's index does not fit"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    fin = np.isfinite(verts).all(1)
    with np.errstate(all="ignore"):
        q = np.floor((verts - np.asarray(origin, np.float32)) / np.float32(cell))
    assert q.dtype == np.float32
    fits = (q >= 0) & (q < float(1 << AXIS_BITS))
    if (fin & ~fits.all(1)).any():
        raise LimitError("a cell index does not fit %d bits" % AXIS_BITS)
    return np.where(fin[:, None], q, 0).astype(np.int64), fin


def clusters(verts, cell, origin=None):
    """rule 3: (cluster [V] int32, index of every cluster [nc, 3], origin)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    b = bounds(verts)
    if b is None:
        return -np.ones(len(verts), np.int32), np.zeros((0, 3), np.int64), np.zeros(3, np.float32)
    origin = b[0] if origin is None else np.asarray(origin, np.float32)
    idx, fin = cell_indices(verts, origin, cell)
    key = (idx[:, 2].astype(np.uint64) << np.uint64(2 * AXIS_BITS)) | (idx[:, 1].astype(np.uint64) << np.uint64(AXIS_BITS)) | idx[:, 0].astype(np.uint64)
    key[~fin] = np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    valid = fin[order]
    head = valid & np.concatenate([[True], ks[1:] != ks[:-1]])
    number = np.cumsum(head) - 1
    cluster = -np.ones(len(verts), np.int32)
    cluster[order[valid]] = number[valid]
    return cluster, idx[order[head]], origin


def remap_triangles(tris, cluster, nc):
    """rules 1 and 7: (ok [F] rule 1 passed, cells [F, 3], survivors' rotated triples in their original order, counts)"""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = len(cluster)
    ok = ((tris >= 0) & (tris < V)).all(1)
    cells = np.where(ok[:, None], cluster[np.clip(tris, 0, max(V - 1, 0))] if V else -1, -1)
    ok &= (cells >= 0).all(1)
    distinct = ok & (cells[:, 0] != cells[:, 1]) & (cells[:, 1] != cells[:, 2]) & (cells[:, 0] != cells[:, 2])
    c = cells[distinct]
    r = np.argmin(c, 1)
    rows = np.arange(len(c))
    trip = np.stack([c[rows, r], c[rows, (r + 1) % 3], c[rows, (r + 2) % 3]], 1)
    order = np.argsort(trip[:, 2], kind="stable")
    order = order[np.argsort(trip[order, 1], kind="stable")]
    order = order[np.argsort(trip[order, 0], kind="stable")]
    ts = trip[order]
    first = np.concatenate([[True], (ts[1:] != ts[:-1]).any(1)]) if len(ts) else np.zeros(0, bool)
    keep = np.zeros(len(trip), bool)
    keep[order[first]] = True
    counts = {"dropped": int((~ok).sum()), "collapsed": int(ok.sum() - distinct.sum()), "duplicates": int(len(trip) - keep.sum())}
    return ok, cells, trip[keep], np.nonzero(distinct)[0][keep], counts


def solve(A, b, m, lam):
    """rule 6 for every row: A [n, 6] = (xx, xy, xz, yy, yz, zz), b [n, 3], m [n, 3] -> x [n, 3] (before the clamp)"""
    tr = (A[:, 0] + A[:, 3]) + A[:, 5]
    with np.errstate(all="ignore"):
        a, bb, c = A[:, 0] / tr + lam, A[:, 1] / tr, A[:, 2] / tr
        d, e, f = A[:, 3] / tr + lam, A[:, 4] / tr, A[:, 5] / tr + lam
        r0, r1, r2 = b[:, 0] / tr + lam * m[:, 0], b[:, 1] / tr + lam * m[:, 1], b[:, 2] / tr + lam * m[:, 2]
        c00, c01, c02 = d * f - e * e, c * e - bb * f, bb * e - c * d
        c11, c12, c22 = a * f - c * c, bb * c - a * e, a * d - bb * bb
        det = (a * c00 + bb * c01) + c * c02
        q = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
    use = (tr != 0.0) & np.isfinite(q).all(1)
    return np.where(use[:, None], q, m)


def quadrics(verts, tris, ok, cells, centre):
    """rules 4 and 5: A [nc, 6], b [nc, 3]; the incidences in ascending 3 t + corner, one addition per term"""
    nc = len(centre)
    A, b = np.zeros((nc, 6)), np.zeros((nc, 3))
    t = np.asarray(tris, np.int64).reshape(-1, 3)[ok]
    p = np.asarray(verts, np.float32).astype(np.float64)[t]
    u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    cl = cells[ok].reshape(-1)                      # row-major: ascending 3 t + corner
    n3 = np.repeat(n, 3, axis=0)
    d = np.repeat(p[:, 0], 3, axis=0) - centre[cl]
    s = (n3[:, 0] * d[:, 0] + n3[:, 1] * d[:, 1]) + n3[:, 2] * d[:, 2]
    np.add.at(A, cl, np.stack([n3[:, 0] * n3[:, 0], n3[:, 0] * n3[:, 1], n3[:, 0] * n3[:, 2], n3[:, 1] * n3[:, 1], n3[:, 1] * n3[:, 2],
                               n3[:, 2] * n3[:, 2]], 1))
    np.add.at(b, cl, n3 * s[:, None])
    return A, b


def simplify(verts, tris, cell, colors=None, origin=None, lam=1e-3, full=False):
    """(verts' [V', 3] float32, tris' [F', 3] int32, colors' or None, cluster [V] int32, stats); full: also the per-cluster intermediate
    values (centre, mean, A, b, position before compaction) for the closed-form checks"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    cell = np.float32(cell)
    cluster, index, origin = clusters(verts, cell, origin)
    nc = len(index)
    ok, cells, trip, survivors, counts = remap_triangles(tris, cluster, nc)
    used = np.zeros(nc, bool)
    used[trip.reshape(-1)] = True
    newid = np.cumsum(used) - 1
    stats = dict(counts, clusters=nc, vertices=int(used.sum()), triangles=len(trip))
    centre = origin.astype(np.float64) + (index.astype(np.float64) + 0.5) * np.float64(cell)
    member = np.nonzero(cluster >= 0)[0]                        # ascending vertex id
    S = np.zeros((nc, 3))
    np.add.at(S, cluster[member], verts[member].astype(np.float64) - centre[cluster[member]])
    cnt = np.bincount(cluster[member], minlength=nc).astype(np.float64)
    m = S / cnt[:, None]
    A, b = quadrics(verts, tris, ok, cells, centre)
    h = np.float64(cell) * 0.5
    x = np.clip(solve(A, b, m, np.float64(lam)), -h, h)
    pos = (centre + x).astype(np.float32)
    cols = None
    if colors is not None:
        C = np.zeros((nc, 3))
        np.add.at(C, cluster[member], np.asarray(colors, np.float32).astype(np.float64)[member])
        cols = (C / cnt[:, None]).astype(np.float32)[used]
    out = (pos[used], newid[trip].astype(np.int32).reshape(-1, 3), cols, cluster, stats)
    if full:
        return out + (dict(centre=centre, mean=m, A=A, b=b, pos=pos, used=used, newid=np.where(used, newid, -1), survivors=survivors, origin=origin),)
    return out


def count_faces(verts, tris, cell, origin=None):
    cluster, index, _ = clusters(verts, cell, origin)
    return len(remap_triangles(tris, cluster, len(index))[2])


def grid_cell(verts, n):
    """rule 8: the smallest fp32 cell >= fp32(longest extent / n) that puts the maximum into cell n - 1 (the quotient advanced by an ulp
    or two: n cells along the longest extent, not n and a layer that holds the extreme vertices alone); fp32 throughout"""
    lo, hi = bounds(verts)
    ext = np.float32((hi - lo).max())
    if not ext > 0:
        return np.float32(1.0)
    cell = ext / np.float32(n)
    while np.floor(ext / cell) >= n:
        cell = np.nextafter(cell, np.float32(np.inf))
    assert cell.dtype == np.float32
    return cell


def bisect(faces, target):
    """rule 8's search, the same probes in the same order as surfel_simplify.bisect_resolution: (n, probes) with faces(n) <= target <
    faces(n + 1) (n = N_MAX where even that grid stays at or below the target)"""
    lo, hi, probes = 1, 2, 0          # faces(1) = 0: one cell
    while True:
        probes += 1
        if faces(hi) > target:
            break
        lo = hi
        if hi == N_MAX:
            return lo, probes
        hi = min(2 * hi, N_MAX)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        if faces(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo, probes


def simplify_target(verts, tris, target, colors=None, lam=1e-3):
    """rule 8: the mesh unchanged when target >= F, else simplify at the bisected resolution; stats["n"]"""
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    if target >= len(tris):
        return np.asarray(verts, np.float32), tris, colors, None, {"n": 0, "triangles": len(tris)}
    n, probes = bisect(lambda k: count_faces(verts, tris, grid_cell(verts, k)), target)
    out = simplify(verts, tris, grid_cell(verts, n), colors, None, lam)
    out[4].update(n=n, probes=probes)
    return out
