"""numpy fp64 restatement of MESH.md §Unbounded (contraction, lattice, fusion, marching cubes, vertex colours of the unbounded mesh
extraction in libsurfel_hip.so).  Test-only: the product never imports it.

Lattices are [M, M, M] arrays indexed [z, y, x], i.e. sample (x, y, z) at flat index x + M (y + M z), the library's layout.  A view
is (P, depth [H, W], rgb [3, H, W] or None) with P the row-vector full_proj_transform [4, 4].
"""
import numpy as np

import mesh_oracle as MO

CLIP = 32.0      # max_range of marching_cubes_with_contraction


def contract(x):
    x = np.asarray(x, np.float64)
    mag = np.linalg.norm(x, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag < 1, x, (2 - 1 / mag) * (x / mag))


def uncontract(y):
    y = np.asarray(y, np.float64)
    mag = np.linalg.norm(y, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag < 1, y, y / (mag * (2 - mag)))


def lattice_size(resolution):
    """M = (N/512) * 511 + 1: the reference's N/512 crops per axis of 512 samples, neighbours sharing their boundary plane."""
    assert resolution % 512 == 0
    return resolution // 512 * 511 + 1


def lattice_step(M, R):
    """the library's step, 2R/(M-1) rounded to fp32 from the fp32 R"""
    R32 = np.float32(R)
    return float(R32), float(np.float32(np.float32(2) * R32 / np.float32(M - 1)))


def lattice_contracted(M, R):
    """contracted positions [M^3, 3] (x, y, z) of the samples in flat order: -R + j * step"""
    R, step = lattice_step(M, R)
    j = np.arange(M, dtype=np.float64)
    z, y, x = np.meshgrid(j, j, j, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1) * step - R


def adaptive_trunc(s, voxel_size):
    """5 voxel_size, divided by 2 - min(|s|, 1.9) where |s| > 1"""
    mag = np.linalg.norm(np.asarray(s, np.float64), axis=-1)
    tr = np.full(mag.shape, 5.0 * float(np.float32(voxel_size)))
    out = mag > 1
    tr[out] /= 2 - np.minimum(mag[out], 1.9)
    return tr


def project(P, p):
    """(ndc_x, ndc_y, w) of world points p [n, 3] under [p, 1] @ P"""
    P = np.asarray(P, np.float32).astype(np.float64)
    q = p @ P[:3] + P[3]
    w = q[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[:, 0] / w, q[:, 1] / w, w


def bilinear(img, nx, ny):
    """grid_sample(img[None, None], ..., mode='bilinear', padding_mode='border', align_corners=True) at ndc (nx, ny), fp64; also the
    largest slope between neighbouring taps of the footprint (value change per pixel).  img [H, W]."""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    px = np.clip((np.nan_to_num(nx) + 1) / 2 * (W - 1), 0, W - 1)
    py = np.clip((np.nan_to_num(ny) + 1) / 2 * (H - 1), 0, H - 1)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = px - x0, py - y0
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    val = (1 - ax) * (1 - ay) * a + ax * (1 - ay) * b + (1 - ax) * ay * c + ax * ay * d
    slope = np.maximum.reduce([np.abs(b - a), np.abs(d - c), np.abs(c - a), np.abs(d - b)])
    return val, slope


def fuse(views, M, R, center, radius, voxel_size, px_err=2e-4, ndc_eps=1e-5):
    """MESH.md §Unbounded fusion in the sum form: tsdf = (-1 + sum clamp(sdf / trunc, -1, 1)) / (1 + n).

    Returns dict(tsdf [M^3], count [M^3], exempt [M^3] bool, bound [M^3]).  A sample is exempt when one of its decisions (ndc inside
    (-1, 1), sdf > -trunc) lies within the fp32 evaluation error of its threshold: ndc_eps in ndc, and for the sdf the depth slope
    times px_err pixels plus 2.5e-7 of |depth| + |w| (more where uncontract amplifies).  bound is the same error carried into the tsdf
    through the unclamped terms: a tsdf sampled across a depth edge is ill-conditioned, and 1e-5 alone does not hold there."""
    s = lattice_contracted(M, R)
    mag = np.linalg.norm(s, axis=1)
    tr = adaptive_trunc(s, voxel_size)
    p = np.asarray(center, np.float64) + float(radius) * uncontract(s)
    amp = 1 + 1 / np.maximum(2 - np.minimum(mag, 1.999), 1e-3)
    total = np.full(len(s), -1.0)
    n = np.zeros(len(s), np.int64)
    exempt = np.zeros(len(s), bool)
    bound = np.zeros(len(s))
    for P, depth, _ in views:
        nx, ny, w = project(P, p)
        vis = (w > 0) & (nx > -1) & (nx < 1) & (ny > -1) & (ny < 1)
        near = (np.abs(w) < 1e-6) | (w > 0) & ((np.abs(np.abs(nx) - 1) < ndc_eps) | (np.abs(np.abs(ny) - 1) < ndc_eps))
        d, slope = bilinear(depth, nx, ny)
        sdf = d - w
        err = slope * px_err + 2.5e-7 * (np.abs(d) + np.abs(w) * amp)
        exempt |= near | (vis & (np.abs(sdf + tr) < err))
        ok = vis & (sdf > -tr)
        total[ok] += np.clip(sdf[ok] / tr[ok], -1, 1)
        n[ok] += 1
        bound[ok] += np.where(np.abs(sdf[ok]) < tr[ok] + err[ok], err[ok] / tr[ok], 0.0)
    return dict(tsdf=(total / (1 + n)).reshape(M, M, M), count=n.reshape(M, M, M), exempt=exempt.reshape(M, M, M),
                bound=(bound / (1 + n)).reshape(M, M, M))


def marching_cubes(tsdf, R, center, radius):
    """MESH.md §Unbounded extraction of a lattice tsdf [M, M, M] ([z, y, x]): every sign-changing lattice edge gets one vertex, owned by
    its lower sample, in (z, y, x, axis) order; triangles in cube order from the case table.  Returns (verts [V, 3] world fp64,
    clipped to +-32, tris [F, 3] int64)."""
    t = np.asarray(tsdf, np.float64)
    M = t.shape[0]
    flat = t.reshape(-1)
    inside = flat < 0
    g = np.arange(M ** 3, dtype=np.int64)
    xyz = np.stack([g % M, (g // M) % M, g // (M * M)], 1)
    stride = np.array([1, M, M * M], np.int64)
    mask = np.zeros((M ** 3, 3), bool)
    for a in range(3):
        ok = xyz[:, a] + 1 < M
        o = np.where(ok, g + stride[a], g)
        mask[:, a] = ok & (inside != inside[o])
    vid = np.full((M ** 3, 3), -1, np.int64)
    vid.reshape(-1)[mask.reshape(-1)] = np.arange(int(mask.sum()))
    src = np.repeat(g, 3)[mask.reshape(-1)]
    ax = np.tile(np.arange(3), M ** 3)[mask.reshape(-1)]
    ta, tb = flat[src], flat[src + stride[ax]]
    q = xyz[src].astype(np.float64)
    q[np.arange(len(src)), ax] += ta / (ta - tb)
    R32, step = lattice_step(M, R)
    verts = np.clip(np.asarray(center, np.float64) + float(radius) * uncontract(q * step - R32), -CLIP, CLIP)
    cube = g[np.all(xyz < M - 1, axis=1)]
    case = np.zeros(len(cube), np.int64)
    for c in range(8):
        case |= inside[cube + (c & 1) + M * ((c >> 1) & 1) + M * M * ((c >> 2) & 1)].astype(np.int64) << c
    keep = MO.NTRI[case] > 0
    cube, case = cube[keep], case[keep]
    tab = np.array([[e for tri in MO.TABLE[c] for e in tri] + [0] * (3 * MO.MAXT - 3 * len(MO.TABLE[c])) for c in range(256)], np.int64)
    slots = np.zeros((len(cube), MO.MAXT, 3), np.int64)
    for j in range(3 * MO.MAXT):
        e = tab[case, j]
        owner = cube + MO.EDGE_OFF[e] @ stride
        slots[:, j // 3, j % 3] = vid[owner, MO.EDGE_AXIS[e]]
    tris = slots[np.arange(MO.MAXT)[None, :] < MO.NTRI[case][:, None]]
    return verts, tris.reshape(-1, 3)


def vertex_colors(verts, views, voxel_size):
    """sum of bilinear rgb / (1 + n) over the views that see a world vertex with depth - w > -5 voxel_size (no contraction)"""
    p = np.asarray(verts, np.float64)
    tr = 5.0 * float(np.float32(voxel_size))
    acc = np.zeros((len(p), 3))
    n = np.zeros(len(p))
    for P, depth, rgb in views:
        nx, ny, w = project(P, p)
        vis = (w > 0) & (nx > -1) & (nx < 1) & (ny > -1) & (ny < 1)
        d, _ = bilinear(depth, nx, ny)
        ok = vis & (d - w > -tr)
        for c in range(3):
            acc[ok, c] += bilinear(rgb[c], nx[ok], ny[ok])[0]
        n[ok] += 1
    return acc / (1 + n)[:, None]
