"""numpy restatement of MESH.md (the TSDF fusion and marching-cubes spec of libsurfel_hip.so's mesh kernels).  Test-only: the
product never imports it.

Volumes are block-sparse: `coords` [nb,3] block coordinates in table order (the library's slot order) and per-voxel arrays
[nb*4096(, k)], voxel (x, y, z) of a block at index x + 16 y + 256 z.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import gen_mc_table as MC  # noqa: E402

TABLE = MC.table()
NTRI = np.array([len(t) for t in TABLE], np.int64)
MAXT = int(NTRI.max())
EDGE_OFF = np.array([[a & 1, (a >> 1) & 1, (a >> 2) & 1] for a, _, _ in MC.EDGES], np.int64)
EDGE_AXIS = np.array([ax for _, _, ax in MC.EDGES], np.int64)
LOCAL = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)  # i = x+16y+256z


def voxel_coords(coords):
    return (np.asarray(coords, np.int64)[:, None, :] * 16 + LOCAL[None]).reshape(-1, 3)


class Lookup:
    """global voxel -> index into the per-voxel arrays (-1: block not allocated)"""

    def __init__(self, coords):
        coords = np.asarray(coords, np.int64).reshape(-1, 3)
        self.lo = coords.min(0) if len(coords) else np.zeros(3, np.int64)
        shape = (coords.max(0) - self.lo + 1) if len(coords) else np.ones(3, np.int64)
        self.grid = np.full(tuple(shape), -1, np.int64)
        if len(coords):
            self.grid[tuple((coords - self.lo).T)] = np.arange(len(coords))

    def __call__(self, g):
        b = (g >> 4) - self.lo
        ok = np.all((b >= 0) & (b < np.array(self.grid.shape)), axis=1)
        out = np.full(len(g), -1, np.int64)
        s = self.grid[tuple(b[ok].T)]
        loc = g[ok] & 15
        out[ok] = np.where(s >= 0, s * 4096 + loc[:, 0] + 16 * loc[:, 1] + 256 * loc[:, 2], -1)
        return out


# ------------------------------------------------------------------------------------------------ fusion
def touched_blocks(depth, cam, voxel_size, sdf_trunc):
    """Blocks one view touches, in the kernel's fp32 arithmetic (mesh_tsdf.hip pixel_blocks, no contraction): set of (x, y, z)."""
    f32 = np.float32
    cam = np.asarray(cam, f32)
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W]
    d = depth.astype(f32).reshape(-1)
    u, v = u.reshape(-1).astype(f32), v.reshape(-1).astype(f32)
    ok = d > 0
    d, u, v = d[ok], u[ok], v[ok]
    fx, fy, cx, cy = cam[12], cam[13], cam[14], cam[15]
    pc = [(u - cx) * d / fx, (v - cy) * d / fy, d]
    q = [pc[0] - cam[3], pc[1] - cam[7], pc[2] - cam[11]]
    bs = f32(voxel_size) * f32(16)
    tr = f32(sdf_trunc)
    lo, hi = [], []
    for j in range(3):
        x = cam[j] * q[0] + cam[4 + j] * q[1] + cam[8 + j] * q[2]
        lo.append(np.floor((x - tr) / bs).astype(np.int64))
        hi.append(np.floor((x + tr) / bs).astype(np.int64))
    out = set()
    span = max(int((hi[j] - lo[j]).max(initial=0)) for j in range(3)) + 1
    for dz in range(span):
        for dy in range(span):
            for dx in range(span):
                m = (lo[0] + dx <= hi[0]) & (lo[1] + dy <= hi[1]) & (lo[2] + dz <= hi[2])
                out.update(map(tuple, np.stack([lo[0][m] + dx, lo[1][m] + dy, lo[2][m] + dz], 1).tolist()))
    return out


def _pixel_f32(g, cam, voxel_size):
    """(u, v) of mesh_integrate_kernel in fp32: centre = (g + 0.5) * vs, p = R c + t, u = floor(fx p.x / p.z + cx + 0.5)"""
    f32 = np.float32
    cam = np.asarray(cam, f32)
    c = [(g[:, j].astype(f32) + f32(0.5)) * f32(voxel_size) for j in range(3)]
    p = [cam[4 * i] * c[0] + cam[4 * i + 1] * c[1] + cam[4 * i + 2] * c[2] + cam[4 * i + 3] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = np.floor(cam[12] * p[0] / p[2] + cam[14] + f32(0.5)).astype(np.float64)
        v = np.floor(cam[13] * p[1] / p[2] + cam[15] + f32(0.5)).astype(np.float64)
    return u, v


def fuse(views, voxel_size, sdf_trunc, table=None):
    """views: [(depth [H,W] (valid means d > 0; already truncated / masked), rgb8 [H,W,3] uint8, camera block [16])].  fp64 integration
    (MESH.md §Integration) over the fp32 allocation.  table = (origin, dims) in blocks: only blocks inside it exist (None: no bound).
    Returns dict(coords, tsdf, rgb, weight, exempt)."""
    per_view = [touched_blocks(d, c, voxel_size, sdf_trunc) for d, _, c in views]
    if table is not None:
        lo, hi = np.asarray(table[0], np.int64), np.asarray(table[0], np.int64) + np.asarray(table[1], np.int64)
        per_view = [{b for b in blocks if np.all(np.asarray(b) >= lo) and np.all(np.asarray(b) < hi)} for blocks in per_view]
    allb = sorted(set().union(*per_view), key=lambda b: (b[2], b[1], b[0]))      # table order: x fastest
    coords = np.array(allb, np.int64).reshape(-1, 3)
    index = {b: k for k, b in enumerate(allb)}
    n = len(allb) * 4096
    tsdf, w, rgb = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    exempt = np.zeros(n, bool)
    vs, tr = float(np.float32(voxel_size)), float(np.float32(sdf_trunc))
    g_all = voxel_coords(coords)
    for (depth, rgb8, cam), blocks in zip(views, per_view):
        cam = np.asarray(cam, np.float32).astype(np.float64)
        R, t = cam[:12].reshape(3, 4)[:, :3], cam[:12].reshape(3, 4)[:, 3]
        fx, fy, cx, cy = cam[12:16]
        H, W = depth.shape
        sel = np.concatenate([np.arange(index[b] * 4096, index[b] * 4096 + 4096) for b in sorted(blocks, key=lambda b: index[b])]) if blocks else np.zeros(0, np.int64)
        c = (g_all[sel] + 0.5) * vs
        p = c @ R.T + t
        ok = p[:, 2] > 0
        pz = np.where(ok, p[:, 2], 1.0)
        xf, yf = fx * p[:, 0] / pz + cx + 0.5, fy * p[:, 1] / pz + cy + 0.5
        # the pixel each voxel projects to is the kernel's fp32 decision (same operations, no contraction); where it differs from the
        # fp64 one the decision lies within rounding of a half pixel: such voxels are exempt (counted by the caller)
        u, v = _pixel_f32(g_all[sel], cam, voxel_size)
        near = ((u != np.floor(xf)) | (v != np.floor(yf))) & ((np.abs(xf - np.round(xf)) < 1e-4) | (np.abs(yf - np.round(yf)) < 1e-4))
        ok &= (u >= 0) & (v >= 0) & (u < W) & (v < H)
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        d = depth.astype(np.float64)[vi, ui]
        ok &= d > 0      # valid means d > 0: zero, negative and NaN depths are holes, as in touched_blocks
        d = np.where(ok, d, 1.0)
        sdf = (d - p[:, 2]) * np.sqrt(1 + ((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2)
        exempt[sel[near]] = True
        exempt[sel[ok & (np.abs(sdf + tr) < 1e-6)]] = True
        ok &= sdf > -tr
        k = sel[ok]
        tv = np.minimum(1.0, sdf[ok] / tr)
        col = rgb8[vi[ok], ui[ok]].astype(np.float64)
        w0 = w[k]
        tsdf[k] = (tsdf[k] * w0 + tv) / (w0 + 1)
        rgb[k] = (rgb[k] * w0[:, None] + col) / (w0 + 1)[:, None]
        w[k] = w0 + 1
    return dict(coords=coords, tsdf=tsdf, rgb=rgb, weight=w, exempt=exempt)


# ------------------------------------------------------------------------------------------------ marching cubes
def cube_cases(coords, tsdf, weight):
    """(valid [n] bool, case [n] int64) of the cube at every voxel: valid when all 8 corners are allocated with w > 0; bit c of the
    case is set when corner c (x = c & 1, y = c >> 1 & 1, z = c >> 2) has tsdf < 0; 0 where the cube is not valid."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    g = voxel_coords(coords)
    look = Lookup(coords)
    okv = weight > 0
    inside = tsdf < 0
    valid = np.ones(len(g), bool)
    case = np.zeros(len(g), np.int64)
    for c in range(8):
        i = look(g + np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.int64))
        valid &= (i >= 0) & okv[np.maximum(i, 0)]
        case |= np.where((i >= 0) & inside[np.maximum(i, 0)], 1, 0) << c
    return valid, np.where(valid, case, 0)


def marching_cubes(coords, tsdf, weight, rgb, voxel_size):
    """MESH.md §Extraction on a block-sparse volume.  Returns (verts [V,3] fp64, colors [V,3], tris [F,3] int64) in the library's order."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    g = voxel_coords(coords)
    look = Lookup(coords)
    n = len(g)
    okv = weight > 0
    inside = tsdf < 0

    def at(off):
        return look(g + np.asarray(off, np.int64))

    valid, case = cube_cases(coords, tsdf, weight)
    mask = np.zeros((n, 3), bool)
    for a in range(3):
        e = np.eye(3, dtype=np.int64)[a]
        o = at(e)
        cross = okv & (o >= 0) & okv[np.maximum(o, 0)] & (inside != inside[np.maximum(o, 0)])
        a1, a2 = [x for x in range(3) if x != a]
        used = np.zeros(n, bool)
        for q in range(4):
            off = np.zeros(3, np.int64)
            off[a1] -= q & 1
            off[a2] -= q >> 1
            cidx = at(off)
            used |= (cidx >= 0) & valid[np.maximum(cidx, 0)]
        mask[:, a] = cross & used
    vid = np.full((n, 3), -1, np.int64)
    flat = mask.reshape(-1)
    vid.reshape(-1)[flat] = np.arange(int(flat.sum()))
    src = np.repeat(np.arange(n), 3)[flat]
    ax = np.tile(np.arange(3), n)[flat]
    other = np.empty(len(src), np.int64)
    for a in range(3):
        m = ax == a
        other[m] = at(np.eye(3, dtype=np.int64)[a])[src[m]]
    ta, tb = tsdf[src], tsdf[other]
    s = ta / (ta - tb)
    verts = g[src] + 0.5
    verts[np.arange(len(src)), ax] += s
    verts = verts * float(np.float32(voxel_size))
    colors = ((1 - s)[:, None] * rgb[src] + s[:, None] * rgb[other]) / 255.0
    cube = np.nonzero(valid & (NTRI[case] > 0))[0]
    tab = np.array([[e for t in TABLE[c] for e in t] + [0] * (3 * MAXT - 3 * len(TABLE[c])) for c in range(256)], np.int64)
    slots = np.zeros((len(cube), MAXT, 3), np.int64)
    for j in range(3 * MAXT):
        e = tab[case[cube], j]
        owner = look(g[cube] + EDGE_OFF[e])
        slots[:, j // 3, j % 3] = np.where(owner >= 0, vid[np.maximum(owner, 0), EDGE_AXIS[e]], -1)
    tris = slots[np.arange(MAXT)[None, :] < NTRI[case[cube]][:, None]]      # (cube, table slot) order
    return verts, colors, tris.reshape(-1, 3)


def sphere_volume(radius_vox, center_vox, nblocks):
    """An analytic sphere SDF (in voxel units, tsdf = signed distance / 4 clipped to [-1, 1]) on every voxel of nblocks^3 blocks."""
    coords = np.stack(np.meshgrid(*[np.arange(nblocks)] * 3, indexing="ij"), -1).transpose(2, 1, 0, 3).reshape(-1, 3)
    g = voxel_coords(coords) + 0.5
    sdf = np.linalg.norm(g - np.asarray(center_vox, np.float64), axis=1) - radius_vox
    return coords, np.clip(sdf / 4.0, -1, 1), np.ones(len(g)), np.full((len(g), 3), 128.0)


# ------------------------------------------------------------------------------------------------ post-processing (MESH.md §Post-processing)
def clusters(tris, V):
    """(label [F], size [F]) int64.  Two triangles are adjacent when they share an unordered vertex pair {a, b} with both ids in
    [0, V) (whatever the winding; (a, a) counts); label[t] = smallest triangle id of t's connected set, size[r] = triangles of the
    set at its root id r and 0 elsewhere.  An edge with an id outside [0, V) links nothing.  A dictionary of edges and a union-find."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    F = len(tris)
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = {}
    for t, tri in enumerate(tris.tolist()):
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if not (0 <= a < V and 0 <= b < V):
                continue
            o = first.setdefault((min(a, b), max(a, b)), t)
            ra, rb = find(o), find(t)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)      # the smaller id stays root
    label = np.array([find(t) for t in range(F)], np.int64).reshape(F)
    return label, np.bincount(label, minlength=F).astype(np.int64)


def post_threshold(size, k):
    """max(k-th largest cluster size, 50); 50 with fewer than k clusters.  size as clusters() returns it (0 at non-root ids)."""
    counts = sorted((int(s) for s in np.asarray(size).reshape(-1) if s > 0), reverse=True)
    return max(counts[k - 1] if 1 <= k <= len(counts) else 0, 50)


def filter_mesh(verts, cols, tris, label, size, threshold):
    """(verts, cols, tris) after the filter: a triangle is kept when size[label[t]] >= threshold and its ids lie in [0, V); a vertex
    is kept when a kept triangle references it (one that repeats an index too); kept triangles that repeat an index are dropped
    last.  Order is preserved, floats are copied bit for bit, triangle ids are renumbered to the kept vertices."""
    verts, cols = np.asarray(verts), np.asarray(cols)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    label, size = np.asarray(label, np.int64), np.asarray(size, np.int64)
    V = len(verts)
    keep = (size[label] >= threshold) & np.all((tris >= 0) & (tris < V), axis=1)
    vref = np.zeros(V, bool)
    vref[tris[keep].reshape(-1)] = True
    vpos = np.cumsum(vref) - vref
    t = tris[keep]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    return verts[vref], cols[vref], vpos[t].reshape(-1, 3)


# name: (tris, V, label worked out by hand) -- the small cluster cases the CPU tests pin the reference to and the GPU tests rerun
HAND_CLUSTERS = {
    "single": ([(0, 1, 2)], 3, [0]),
    "bow_tie": ([(0, 1, 2), (2, 3, 4)], 5, [0, 1]),                                        # one shared vertex is no edge
    "edge_same_winding": ([(0, 1, 2), (0, 1, 3)], 4, [0, 0]),
    "edge_opposite_winding": ([(0, 1, 2), (1, 0, 3)], 4, [0, 0]),
    "fan_of_5": ([(0, 1, 2), (1, 0, 3), (0, 1, 4), (5, 0, 1), (1, 6, 0)], 7, [0] * 5),      # non-manifold: five on edge 0-1
    "duplicate": ([(0, 1, 2), (0, 1, 2)], 3, [0, 0]),
    "repeated_index": ([(3, 4, 5), (0, 0, 1), (2, 1, 0)], 6, [0, 1, 1]),                   # (a, a, b) has the edge a-b
    # V = 16: (5, 25) has an id out of range and 25 & 15 = 9, so on 4 key bits it would sort between the two (5, 9) edges
    "bad_id_alias": ([(5, 9, 1), (5, 25, 3), (9, 5, 2)], 16, [0, 1, 0]),
}


# ------------------------------------------------------------------------------------------------ mesh checks
def edge_use(tris):
    """{(a, b): count of directed uses}"""
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    keys, counts = np.unique(e, axis=0, return_counts=True)
    return {tuple(k): int(c) for k, c in zip(keys.tolist(), counts)}


def closed_oriented_manifold(tris):
    """every undirected edge used by exactly two triangles, once in each direction"""
    use = edge_use(tris)
    return all(c == 1 and use.get((b, a), 0) == 1 for (a, b), c in use.items())


def euler(verts, tris):
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    return len(verts) - len(np.unique(e, axis=0)) + len(tris)


def face_normals(verts, tris):
    v = np.asarray(verts, np.float64)
    return np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
