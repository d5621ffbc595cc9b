"""The numpy restatement of the mesh repair (REPAIR.md §Rules): stable argsorts for the half-edge sort, run lengths for the cut, the same
pointer jumping as csrc/mesh_repair.hip for the fans and the border loops (so label_rounds comes out the same), and a centroid sum
that is vectorised over the loops and sequential over the position in the loop — the k-th pass adds the k-th vertex of every filled loop
that has one, so every fp64 sum is formed one addition at a time in the loop's order.  The device's result must equal this one exactly:
the integers as integers, positions and colours as bit patterns."""
import numpy as np

import smooth_oracle as SO

COUNTS = ("kept", "dropped", "cut_triangles", "nonmanifold_edges", "misoriented_edges", "split_vertices", "loops", "border_edges",
          "longest_loop", "filled_loops", "fill_triangles", "fill_vertices", "border_edges_after", "label_rounds")
HEAD_BIT = 1 << 31


class LimitError(ValueError):
    pass


def check_cap(max_hole_edges):
    if isinstance(max_hole_edges, (bool, np.bool_)) or not isinstance(max_hole_edges, (int, float, np.integer, np.floating)):
        raise ValueError("max_hole_edges must be a whole number >= 0")
    if not 0 <= max_hole_edges < 2 ** 62 or int(max_hole_edges) != max_hole_edges:
        raise ValueError("max_hole_edges must be a whole number >= 0")
    return int(max_hole_edges)


def orbits(ptr, key):
    """Pointer jumping over a successor array of in- and out-degree at most one (a terminal element points at itself): after round r
    lab[i] is the smallest key among the 2^r elements from i on and off[i] the distance to its first occurrence.  A round is one
    launch on the device; the rounds stop after the first one that changes no label.  (lab, off, rounds)"""
    ptr = np.asarray(ptr, np.int64).copy()
    lab = np.asarray(key, np.int64).copy()
    off = np.zeros(len(ptr), np.int64)
    step, rounds = 1, 0
    while len(ptr):
        rounds += 1
        take = lab[ptr] < lab
        lab, off, ptr = np.where(take, lab[ptr], lab), np.where(take, off[ptr] + step, off), ptr[ptr]
        step *= 2
        if not take.any():
            break
    return lab, off, rounds


def _exclusive(a):
    return np.cumsum(a) - a


def repair(verts, tris, colors=None, max_hole_edges=32):
    """rules 1-7: dict(vertices, colors, triangles, vertex_source, triangle_source, loop_lengths, stats) and, for border_loops, the
    border half-edges of the split mesh in ascending order with their loop and position (half_edge, loop, position)"""
    cap = check_cap(max_hole_edges)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    cols = None if colors is None else np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    V, F = len(verts), len(tris)
    if 3 * F >= 2 ** 31 or V + 3 * F >= 2 ** 31:
        raise LimitError("3 F and V + 3 F must stay below 2^31")
    # ---- 1, 2: kept triangles, their half-edges 3 m + k
    ok = SO.kept_triangles(verts, tris)
    kt = np.nonzero(ok)[0]
    t = tris[kt]
    src, dst = t.reshape(-1), t[:, (1, 2, 0)].reshape(-1)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    # ---- 3: the sort by (lo, hi), the runs, the cut
    order = np.argsort(hi, kind="stable")
    order = order[np.argsort(lo[order], kind="stable")]
    slo, shi, fwd = lo[order], hi[order], (src[order] == lo[order]).astype(np.int64)
    n = len(order)
    head = np.ones(n, bool)
    head[1:] = (slo[1:] != slo[:-1]) | (shi[1:] != shi[:-1])
    start = np.nonzero(head)[0]
    length = np.diff(np.concatenate([start, [n]]))
    nfwd = np.add.reduceat(fwd, start) if n else np.zeros(0, np.int64)
    bad = (length > 2) | (nfwd > 1) | (length - nfwd > 1)
    run = np.cumsum(head) - 1
    cut = np.zeros(len(t), bool)
    cut[order[bad[run]] // 3] = True
    surv = ~cut
    spos = _exclusive(surv.astype(np.int64))
    ts, tsrc = t[surv], kt[surv]
    Fs = len(ts)
    renum = lambda h: 3 * spos[h // 3] + h % 3      # the survivors' half-edges, numbered again 3 m + k
    twin = -np.ones(3 * Fs, np.int64)
    pair = start[(length == 2) & ~bad]
    a, b = order[pair], order[pair + 1]
    both = surv[a // 3] & surv[b // 3]
    twin[renum(a[both])] = renum(b[both])
    twin[renum(b[both])] = renum(a[both])
    # ---- 4: fans are the orbits of r = twin o prev; the head of an open fan carries the smallest key
    h = np.arange(3 * Fs)
    prev = h - h % 3 + (h % 3 + 2) % 3
    nxt = h - h % 3 + (h % 3 + 1) % 3
    tp = twin[prev]
    is_head = tp < 0
    fan, _, _ = orbits(np.where(is_head, h, tp), np.where(is_head, h, h | HEAD_BIT))
    fan = fan & (HEAD_BIT - 1)
    hsrc = ts.reshape(-1)
    rep = fan == h
    first = np.full(V, 3 * Fs, np.int64)
    np.minimum.at(first, hsrc[rep], h[rep])
    eh = h[rep & (first[hsrc] != h)]                      # the extra fans' labels, ascending
    by_vertex = np.argsort(hsrc[eh], kind="stable")      # ascending (u, label)
    S = len(eh)
    new_index = np.zeros(3 * Fs, np.int64)
    new_index[eh[by_vertex]] = V + np.arange(S)
    split_source = hsrc[eh[by_vertex]]
    corner = np.where(first[hsrc] == fan, hsrc, new_index[fan])
    # ---- 5: border loops on the split mesh, in the compacted numbering b of the border half-edges
    bh = np.nonzero(twin < 0)[0]
    nb = len(bh)
    bsrc, bdst = corner[bh], corner[nxt[bh]]
    border_out = -np.ones(V + S, np.int64)
    border_out[bsrc] = np.arange(nb)
    assert len(np.unique(bsrc)) == nb, "a vertex with two border half-edges leaving it"
    succ = border_out[bdst]
    assert (succ >= 0).all()
    lab, off, rounds = orbits(succ, np.arange(nb))
    starts = np.nonzero(lab == np.arange(nb))[0]
    lengths = off[succ[starts]] + 1
    loop_of_start = -np.ones(nb, np.int64)
    loop_of_start[starts] = np.arange(len(starts))
    loop = loop_of_start[lab]
    position = (lengths[loop] - off) % lengths[loop] if nb else np.zeros(0, np.int64)
    # ---- 6: fill
    filled = lengths <= cap
    gofs = _exclusive(np.where(filled, lengths, 0))
    tcount = np.where(filled, np.where(lengths == 3, 1, lengths), 0)
    tofs = _exclusive(tcount)
    has_c = filled & (lengths > 3)
    cofs = _exclusive(has_c.astype(np.int64))
    G, Ff, Cn = int(np.where(filled, lengths, 0).sum()), int(tcount.sum()), int(has_c.sum())
    fsrc = np.zeros(G, np.int64)
    sel = filled[loop] if nb else np.zeros(0, bool)
    fsrc[gofs[loop[sel]] + position[sel]] = bsrc[sel]
    vsource = np.concatenate([np.arange(V), split_source, -np.ones(Cn, np.int64)]).astype(np.int64)

    def attribute(p):
        bits = p.view(np.uint32)
        out = np.concatenate([bits, bits[split_source], np.zeros((Cn, 3), np.uint32)]).view(np.float32)      # copies as integers
        p64 = np.concatenate([bits, bits[split_source]]).view(np.float32).astype(np.float64)
        loops_c = np.nonzero(has_c)[0]
        s = np.zeros((Cn, 3), np.float64)      # +0.0
        L = lengths[loops_c]
        for k in range(int(L.max()) if Cn else 0):      # one addition per term, in position order
            rows = np.nonzero(k < L)[0]
            s[rows] = s[rows] + p64[fsrc[gofs[loops_c[rows]] + k]]
        with np.errstate(all="ignore"):
            out[V + S:] = (s / L.astype(np.float64)[:, None]).astype(np.float32)
        return out

    ftris = np.zeros((Ff, 3), np.int64)
    fsource = np.zeros(Ff, np.int64)
    for l in np.nonzero(filled)[0]:
        L, g, o = int(lengths[l]), int(gofs[l]), int(tofs[l])
        if L == 3:
            ftris[o] = (fsrc[g], fsrc[g + 2], fsrc[g + 1])
        else:
            k = np.arange(L)
            ftris[o:o + L] = np.stack([fsrc[g + (k + 1) % L], fsrc[g + k], np.full(L, V + S + cofs[l])], 1)
        fsource[o:o + tcount[l]] = -1 - l
    stats = dict(kept=int(ok.sum()), dropped=int(F - ok.sum()), cut_triangles=int(cut.sum()), nonmanifold_edges=int((length > 2).sum()),
                 misoriented_edges=int(((length == 2) & (nfwd != 1)).sum()), split_vertices=S, loops=len(starts), border_edges=nb,
                 longest_loop=int(lengths.max()) if len(starts) else 0, filled_loops=int(filled.sum()), fill_triangles=Ff, fill_vertices=Cn,
                 border_edges_after=nb - G, label_rounds=rounds)
    return dict(vertices=attribute(verts), colors=None if cols is None else attribute(cols),
                triangles=np.concatenate([corner.reshape(-1, 3), ftris]).astype(np.int32),
                vertex_source=vsource.astype(np.int32), triangle_source=np.concatenate([tsrc, fsource]).astype(np.int32),
                loop_lengths=lengths.astype(np.int32), stats=stats,
                half_edge=bh.astype(np.int32), loop=loop.astype(np.int32), position=position.astype(np.int32))
