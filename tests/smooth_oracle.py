"""The numpy restatement of the mesh smoothing (SMOOTH.md §Rules): stable argsorts for the sort, run heads and a cumulative sum for the
unique directed edges, and a filter step that is vectorised over the vertices and sequential over the neighbour's rank in its row — the
r-th pass adds the r-th neighbour of every row that has one, so every row's fp64 sum is formed one addition at a time in the row's order.
Rule for rule and operation for operation what csrc/mesh_smooth.hip does; the device's result must equal this one bit for bit."""
import numpy as np

FLAG_BOUNDARY, FLAG_NONMANIFOLD, FLAG_ISOLATED = 1, 2, 4
METHODS = ("taubin", "laplacian")
BOUNDARY = ("free", "fixed", "curve")
COUNTS = ("kept", "dropped", "directed_edges", "border_edges", "nonmanifold_edges", "boundary_vertices", "isolated_vertices", "max_degree")
SRC_CORNER, DST_CORNER = (0, 1, 1, 2, 2, 0), (1, 0, 2, 1, 0, 2)      # a->b, b->a, b->c, c->b, c->a, a->c


class LimitError(ValueError):
    pass


def kept_triangles(verts, tris):
    """rule 1: [F] bool"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = len(verts)
    ok = ((tris >= 0) & (tris < V)).all(1)
    ok &= (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])
    fin = np.isfinite(verts).all(1)
    ok[ok] = fin[tris[ok]].all(1)
    return ok


def adjacency(verts, tris):
    """rules 1-3: dict(offsets [V + 1] int32, neighbors [E2] int32, multiplicity [E2] int32, flags [V] uint8, stats)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V, F = len(verts), len(tris)
    if V >= 2 ** 31 or 6 * F >= 2 ** 31:
        raise LimitError("V and 6 F must stay below 2^31")
    ok = kept_triangles(verts, tris)
    t = tris[ok]
    src = t[:, SRC_CORNER].reshape(-1)
    dst = t[:, DST_CORNER].reshape(-1)
    order = np.argsort(dst, kind="stable")                       # the low word
    order = order[np.argsort(src[order], kind="stable")]         # then the high word
    s, d = src[order], dst[order]
    n = len(s)
    head = np.ones(n, bool)
    head[1:] = (s[1:] != s[:-1]) | (d[1:] != d[:-1])
    start = np.nonzero(head)[0]
    esrc, nbr = s[start], d[start]
    mult = np.diff(np.concatenate([start, [n]]))
    offsets = np.searchsorted(esrc, np.arange(V + 1), side="left")
    deg = np.diff(offsets)
    one = np.bincount(esrc[mult == 1], minlength=V)[:V] if V else np.zeros(0, np.int64)
    many = np.bincount(esrc[mult > 2], minlength=V)[:V] if V else np.zeros(0, np.int64)
    flags = (np.where(one > 0, FLAG_BOUNDARY, 0) | np.where(many > 0, FLAG_NONMANIFOLD, 0) | np.where(deg == 0, FLAG_ISOLATED, 0)).astype(np.uint8)
    stats = dict(kept=int(ok.sum()), dropped=int(F - ok.sum()), directed_edges=int(len(start)), border_edges=int((mult == 1).sum()) // 2,
                 nonmanifold_edges=int((mult > 2).sum()) // 2, boundary_vertices=int((one > 0).sum()), isolated_vertices=int((deg == 0).sum()),
                 max_degree=int(deg.max()) if V else 0)
    return dict(offsets=offsets.astype(np.int32), neighbors=nbr.astype(np.int32), multiplicity=mult.astype(np.int32), flags=flags, stats=stats)


def plan(adj, boundary):
    """The rows a step sums under a boundary mode, by rank: (pinned [V] bool, count [V], [(rows, neighbours) of rank 0, of rank 1, ...])"""
    offsets = adj["offsets"].astype(np.int64)
    V = len(offsets) - 1
    deg = np.diff(offsets)
    row = np.repeat(np.arange(V), deg)
    is_boundary = (adj["flags"] & FLAG_BOUNDARY) != 0
    use = np.ones(len(row), bool)
    if boundary == "curve":
        use = ~is_boundary[row] | (adj["multiplicity"] == 1)
    row, nbr = row[use], adj["neighbors"].astype(np.int64)[use]
    count = np.bincount(row, minlength=V)[:V] if V else np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(count)])[:-1]
    rank = np.arange(len(row)) - first[row]
    by_rank = np.argsort(rank, kind="stable")
    cuts = np.searchsorted(rank[by_rank], np.arange((rank.max() + 2) if len(rank) else 1))
    passes = [(row[by_rank[a:b]], nbr[by_rank[a:b]]) for a, b in zip(cuts[:-1], cuts[1:])]
    pinned = count == 0
    if boundary == "fixed":
        pinned = pinned | is_boundary
    return pinned, count, passes


def step(p, the_plan, f):
    """rule 4: one step with factor f over p [V, 3] float32"""
    p = np.ascontiguousarray(p, np.float32)
    pinned, count, passes = the_plan
    p64 = p.astype(np.float64)
    s = np.zeros_like(p64)                       # +0.0
    for rows, nbrs in passes:                    # one addition per term, the row's order (a rank holds every row at most once)
        s[rows] = s[rows] + p64[nbrs]
    with np.errstate(all="ignore"):
        m = s / count.astype(np.float64)[:, None]
        d = m - p64
        fd = np.float64(f) * d
        out = (p64 + fd).astype(np.float32)
    bits = np.where(pinned[:, None], p.view(np.uint32), out.view(np.uint32))      # a pinned vertex keeps its bit pattern
    return bits.view(np.float32)


def factors(iterations, method="taubin", lam=0.5, mu=-0.53, boundary="free"):
    """rule 5: the checked arguments' list of step factors"""
    if method not in METHODS or boundary not in BOUNDARY:
        raise ValueError("method / boundary")
    if int(iterations) != iterations or iterations < 0 or not 0.0 < lam <= 1.0:
        raise ValueError("iterations / lam")
    if method == "laplacian":
        return [float(lam)] * int(iterations)
    if not mu < -lam or not np.isfinite(mu):
        raise ValueError("mu")
    return [float(lam), float(mu)] * int(iterations)


def smooth(p, adj, iterations=10, method="taubin", lam=0.5, mu=-0.53, boundary="free"):
    """rules 4-6: the attribute p [V, 3] after the schedule; the input is not written"""
    fs = factors(iterations, method, lam, mu, boundary)
    the_plan = plan(adj, boundary)
    out = np.array(p, np.float32, copy=True).reshape(-1, 3)
    for f in fs:
        out = step(out, the_plan, f)
    return out
