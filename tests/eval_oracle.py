"""Plain-numpy restatement of EVAL.md's rules 1-7 (the DTU mesh evaluation), the oracle of tests/test_eval_cpu.py and
tests/test_gpu_eval.py.  fp64 where the reference is fp64; a second fp32 path repeats the kernels' operation order for the thinning's
pair test on coordinates re-based to the grid origin.  numpy only: it runs wherever the tests run."""
import numpy as np


# ------------------------------------------------------------------------------------------------ rule 1
def sample_mesh(verts, tris, density):
    """(points [V + S, 3] float64: the vertices, then the samples in triangle order; samples per triangle [F] int64)."""
    verts = np.asarray(verts, np.float64)
    tris = np.asarray(tris, np.int64)
    tv = verts[tris]
    v1, v2 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    l1, l2 = np.linalg.norm(v1, axis=-1), np.linalg.norm(v2, axis=-1)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1)
    counts = np.zeros(len(tris), np.int64)
    out = [verts]
    with np.errstate(divide="ignore", invalid="ignore"):
        thr = density * np.sqrt(l1 * l2 / area2)
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
    for t in np.nonzero(area2 > 0)[0]:
        a, b = n1[t], n2[t]
        c0 = (np.arange(a + 1) + 0.5) / max(a, 1e-7)
        c1 = (np.arange(b + 1) + 0.5) / max(b, 1e-7)
        m = (c0[:, None] + c1[None, :]) < 1
        i, j = np.nonzero(m)                      # i outer, j inner
        counts[t] = len(i)
        if len(i):
            out.append(v1[t] * c0[i, None] + v2[t] * c1[j, None] + tv[t, 0])
    return np.concatenate(out, 0), counts


# ------------------------------------------------------------------------------------------------ neighbours within a radius
def _pair_mask(pi, pj, r, f32):
    if f32:      # the kernel: fp32, no contraction, (dx^2 + dy^2) + dz^2 <= r * r
        d = pi - pj
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r32 = np.float32(r)
        return d2 <= r32 * r32
    d = pi - pj
    return np.sqrt((d * d).sum(1)) <= r


def rebase(points, f32):
    """Coordinates relative to the cloud's minimum corner: fp32 subtraction of fp32 values (the kernels) or the fp64 points."""
    if not f32:
        return np.asarray(points, np.float64)
    p = np.asarray(points, np.float32)
    return p - p.min(0) if len(p) else p


def radius_pairs_brute(points, r, f32=False, chunk=1024):
    """Directed pairs (i, j), i != j, within r (<=), brute force in chunks."""
    p = rebase(points, f32)
    ii, jj = [], []
    for s in range(0, len(p), chunk):
        a = p[s:s + chunk]
        i, j = np.nonzero(np.ones((len(a), len(p)), bool))
        m = _pair_mask(a[i], p[j], r, f32) & (i + s != j)
        ii.append(i[m] + s); jj.append(j[m])
    return np.concatenate(ii) if ii else np.zeros(0, np.int64), np.concatenate(jj) if jj else np.zeros(0, np.int64)


def radius_pairs(points, r, f32=False):
    """The same pairs through a cell hash (cell edge 1.01 r): candidates from the 27 cells around each point, then the exact test."""
    p = rebase(points, f32)
    n = len(p)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p64 = np.asarray(p, np.float64)
    c = np.floor((p64 - p64.min(0)) / (1.01 * float(r))).astype(np.int64) + 1
    dims = c.max(0) + 2
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    order = np.argsort(key, kind="stable")
    uk, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    ii, jj = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nk = key + (dz * dims[1] + dy) * dims[0] + dx
                pos = np.searchsorted(uk, nk)
                pos[pos >= len(uk)] = 0
                has = uk[pos] == nk
                src = np.nonzero(has)[0]
                k = cnt[pos[src]]
                i = np.repeat(src, k)
                first = np.repeat(start[pos[src]], k)
                within = np.arange(len(i)) - np.repeat(np.cumsum(k) - k, k)
                j = order[first + within]
                m = _pair_mask(p[i], p[j], r, f32) & (i != j)
                ii.append(i[m]); jj.append(j[m])
    return np.concatenate(ii), np.concatenate(jj)


# ------------------------------------------------------------------------------------------------ rules 2, 3
def shuffle_order(n, seed):
    """order[k] = index of the k-th point of the thinning order"""
    return np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)


def thin_sequential(n, pairs, order):
    """The reference's loop, literally: walk the order; a point still marked drops every neighbour and stays."""
    i, j = pairs
    o = np.argsort(i, kind="stable")
    i, j = i[o], j[o]
    start = np.searchsorted(i, np.arange(n + 1))
    mask = np.ones(n, bool)
    for cur in order:
        if mask[cur]:
            mask[j[start[cur]:start[cur + 1]]] = False
            mask[cur] = True
    return mask


def thin_rounds(n, pairs, order):
    """The same set as the lexicographically-first maximal independent set, in rounds: a point is kept when every earlier neighbour is
    dropped, dropped when one earlier neighbour is kept.  Returns (mask, rounds)."""
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    i, j = pairs
    e = rank[j] < rank[i]
    i, j = i[e], j[e]                              # j is an earlier neighbour of i
    state = np.zeros(n, np.int8)                   # 0 undecided, 1 kept, 2 dropped
    rounds = 0
    while True:
        rounds += 1
        und = state == 0
        if not und.any():
            break
        kept_nb = np.zeros(n, bool); open_nb = np.zeros(n, bool)
        kept_nb[i[state[j] == 1]] = True
        open_nb[i[state[j] == 0]] = True
        new = state.copy()
        new[und & kept_nb] = 2
        new[und & ~kept_nb & ~open_nb] = 1
        state = new
    return state == 1, rounds


def thin(points, density, seed, f32=False):
    n = len(points)
    return thin_sequential(n, radius_pairs(points, density, f32), shuffle_order(n, seed))


# ------------------------------------------------------------------------------------------------ rule 4
def obs_masks(points, bb, patch, res, obs_mask):
    """(inbound [N], in_obs [N]) of fp64 points; bb float32 [2, 3]."""
    p = np.asarray(points, np.float64)
    bb = np.asarray(bb, np.float32)
    inbound = ((p >= bb[:1] - np.float32(patch)) & (p < bb[1:] + np.float32(patch * 2))).sum(-1) == 3
    g = np.around((p - bb[:1]) / float(res))
    ok = inbound & (((g >= 0) & (g < np.array(obs_mask.shape)[None])).sum(-1) == 3)
    gi = g[ok].astype(np.int64)
    in_obs = np.zeros(len(p), bool)
    in_obs[np.nonzero(ok)[0]] = obs_mask[gi[:, 0], gi[:, 1], gi[:, 2]] != 0
    return inbound, in_obs


def above_plane(points, plane):
    p = np.asarray(points, np.float64)
    return (np.asarray(plane, np.float64).reshape(1, 4) * np.concatenate([p, np.ones_like(p[:, :1])], -1)).sum(-1) > 0


# ------------------------------------------------------------------------------------------------ rule 5
def _nearest_in_cells(q, c, cell):
    """fp64 distance of every query to the nearest cloud point among the 27 cells (edge `cell`) around it, inf when they are empty.
    Every cloud point within `cell` of a query lies in those cells, so a result <= cell is the exact nearest distance."""
    lo = np.minimum(q.min(0), c.min(0))
    cq, cc = np.floor((q - lo) / cell).astype(np.int64) + 1, np.floor((c - lo) / cell).astype(np.int64) + 1
    dims = np.maximum(cq.max(0), cc.max(0)) + 2
    kq, kc = (cq[:, 2] * dims[1] + cq[:, 1]) * dims[0] + cq[:, 0], (cc[:, 2] * dims[1] + cc[:, 1]) * dims[0] + cc[:, 0]
    order = np.argsort(kc, kind="stable")
    uk, start, cnt = np.unique(kc[order], return_index=True, return_counts=True)
    best = np.full(len(q), np.inf)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nk = kq + (dz * dims[1] + dy) * dims[0] + dx
                pos = np.searchsorted(uk, nk)
                pos[pos >= len(uk)] = 0
                src = np.nonzero(uk[pos] == nk)[0]
                k = cnt[pos[src]]
                i = np.repeat(src, k)
                j = order[np.repeat(start[pos[src]], k) + np.arange(len(i)) - np.repeat(np.cumsum(k) - k, k)]
                d = q[i] - c[j]
                np.minimum.at(best, i, np.sqrt((d * d).sum(1)))
    return best


def nearest(queries, cloud, chunk=512):
    """fp64 distance of every query to its nearest cloud point (inf for an empty cloud).  Exact: a cell hash answers the queries whose
    neighbour is within a cell edge (three edges are tried), brute force in chunks the rest; there the candidate comes from the
    expanded form |q|^2 + |c|^2 - 2 q.c on centred coordinates (one matrix product per chunk), the distance from the difference."""
    q, c = np.asarray(queries, np.float64), np.asarray(cloud, np.float64)
    out = np.full(len(q), np.inf)
    if len(c) == 0 or len(q) == 0:
        return out
    cell = 4.0 * float((c.max(0) - c.min(0)).max()) / np.sqrt(len(c))
    todo = np.arange(len(q))
    for _ in range(3 if cell > 0 else 0):
        near = np.abs(q[todo] - np.clip(q[todo], c.min(0), c.max(0))).max(1) <= cell      # (far queries would only widen the hash)
        d = _nearest_in_cells(q[todo[near]], c, cell) if near.any() else np.zeros(0)
        done = d <= cell
        out[todo[near][done]] = d[done]
        todo = np.concatenate([todo[~near], todo[near][~done]])
        cell *= 2
        if len(todo) == 0:
            return out
    mid = c.mean(0)
    q0, c0 = q - mid, c - mid
    cc = (c0 * c0).sum(1)
    for s in range(0, len(todo), chunk):
        t = todo[s:s + chunk]
        j = np.argmin(cc[None] - 2.0 * (q0[t] @ c0.T), axis=1)
        d = q[t] - c[j]
        out[t] = np.sqrt((d * d).sum(1))
    return out


def nearest_exact(queries, cloud, chunk=256):
    """The same by differences only (slow; for small cases and cross-checks)."""
    q, c = np.asarray(queries, np.float64), np.asarray(cloud, np.float64)
    if len(c) == 0:
        return np.full(len(q), np.inf)
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None] - c[None]
        out[s:s + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def evaluate_dtu(points, stl, obs_mask, bb, res, plane, density, patch, max_dist, seed, f32=False, keep=None):
    """Rules 2-5 on a cloud (fp64 values; sample a mesh with sample_mesh first).  keep: a thinning mask to use instead of computing one.
    Returns the means, the stage sizes under the reference's names and the distances."""
    points = np.asarray(points, np.float64)
    if keep is None:
        keep = thin(points.astype(np.float32) if f32 else points, density, seed, f32)
    down = points[keep]
    inbound, in_obs = obs_masks(down, bb, patch, res, obs_mask)
    data_in, data_in_obs = down[inbound], down[in_obs]
    stl = np.asarray(stl, np.float64)
    above = above_plane(stl, plane)
    d2s = nearest(data_in_obs, stl)
    s2d = nearest(stl[above], data_in)
    m1, m2 = (d[d < max_dist].mean() if (d < max_dist).any() else np.nan for d in (d2s, s2d))
    return dict(mean_d2s=float(m1), mean_s2d=float(m2), overall=float((m1 + m2) / 2), data_pcd=len(points), data_down=int(keep.sum()),
                data_in=len(data_in), data_in_obs=len(data_in_obs), stl_above=int(above.sum()), keep=keep, d2s=d2s, s2d=s2d)


# ------------------------------------------------------------------------------------------------ rule 6
def fscore(d2s, s2d, tau):
    p = float(np.mean(np.asarray(d2s) < tau)) if len(d2s) else 0.0
    r = float(np.mean(np.asarray(s2d) < tau)) if len(s2d) else 0.0
    return dict(precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0)


# ------------------------------------------------------------------------------------------------ rule 7
def dilate(mask, r):
    """(mask != 0) dilated by the disk dx^2 + dy^2 <= r^2 (zero outside the image), by shifting."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = np.zeros_like(m)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > r * r:
                continue
            ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
            xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
            out[yd, xd] |= m[ys, xs]
    return out


def cull_vertices(verts, proj, dilated, margins=False):
    """Kept mask of rule 7 in fp64 from proj [V, 12] (rows 0..2 of K . w2c) and dilated masks [V, H, W].  margins: also a mask of the
    vertices an fp32 evaluation may decide differently: in some view the ndc lies within 1e-5 of +-1, or a sampled pixel coordinate lies
    within 1e-3 of a half-integer and the dilated mask differs between the pixels on either side."""
    v = np.asarray(verts, np.float64)
    vh = np.concatenate([v, np.ones_like(v[:, :1])], 1)
    keep = np.ones(len(v), bool)
    near = np.zeros(len(v), bool)
    nv, H, W = dilated.shape

    def sample(k, gx, gy, valid):
        inside = valid & (gx >= 0) & (gx <= W - 1) & (gy >= 0) & (gy <= H - 1)
        ix, iy = np.where(inside, gx, 0).astype(np.int64), np.where(inside, gy, 0).astype(np.int64)
        return inside & (dilated[k][iy, ix] != 0)

    for k in range(nv):
        x = vh @ np.asarray(proj[k], np.float64).reshape(3, 4).T
        with np.errstate(divide="ignore", invalid="ignore"):
            pix = x[:, :2] / (x[:, 2:] + 1e-6)
            ndc = (pix / np.array([W - 1, H - 1]) - 0.5) * 2
            valid = ((ndc > -1) & (ndc < 1)).all(1)
            f = (ndc + 1) / 2 * np.array([W - 1, H - 1])
        f = np.where(np.isfinite(f), f, -1e9)
        g = np.around(f)
        keep &= sample(k, g[:, 0], g[:, 1], valid) | ~valid
        if margins:
            lo = np.floor(f)
            half = np.abs(f - lo - 0.5) < 1e-3
            hits = [sample(k, np.where(half[:, 0], lo[:, 0] + a, g[:, 0]), np.where(half[:, 1], lo[:, 1] + b, g[:, 1]), valid) for a in (0, 1) for b in (0, 1)]
            with np.errstate(invalid="ignore"):
                near |= (np.abs(np.abs(ndc) - 1) < 1e-5).any(1) | (valid & ~(hits[0] == hits[1]) | ~(hits[0] == hits[2]) | ~(hits[0] == hits[3]))
    return (keep, near) if margins else keep


def cull_mesh(verts, tris, keep, scale=1.0, offset=0.0):
    tris = np.asarray(tris, np.int64)
    tk = keep[tris].all(1)
    t = tris[tk]
    used = np.zeros(len(verts), bool)
    used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return np.asarray(verts, np.float64)[used] * scale + offset, remap[t]
