"""GPU checks of what stands behind fuse_post.ply (csrc/mesh_tsdf.hip, MESH.md): triangle clusters, the filter and its scans bit for
bit against tests/mesh_oracle.py, marching cubes on crafted fields that hold all 256 cube cases, and fusion at the table's border
and on invalid depths.  Integer results must be equal; the float bounds are derived where they are used."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mesh_oracle as O  # noqa: E402

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ seeded builders
def _islands(G, cut_rows):
    """(tris, nverts) of a G x G quad grid, two triangles per quad, without the quads of the rows in cut_rows: every band of rows
    that remains is one island of 2 G triangles per row."""
    tris = []
    for i in (r for r in range(G) if r not in cut_rows):
        for j in range(G):
            a, b, c, d = i * (G + 1) + j, i * (G + 1) + j + 1, (i + 1) * (G + 1) + j, (i + 1) * (G + 1) + j + 1
            tris += [(a, b, c), (b, d, c)]
    return np.array(tris, np.int64), (G + 1) ** 2


def _join(*meshes):
    tris, n = [], 0
    for t, nv in meshes:
        tris.append(t + n)
        n += nv
    return np.concatenate(tris), n


def _shuffled(tris, nverts, seed, V=None):
    """triangle order permuted and vertex ids sent through a random injective map into [0, V) that reaches 0 and V - 1"""
    rng = np.random.default_rng(seed)
    V = nverts if V is None else V
    ids = rng.choice(V, nverts, replace=False).astype(np.int64)
    for k, want in enumerate((0, V - 1)):
        if want not in ids:
            ids[k] = want
    return ids[tris[rng.permutation(len(tris))]], V


CUT = {3, 7, 12, 20, 33}      # G = 40: islands of 3, 3, 4, 7, 12 and 6 rows = 240, 240, 320, 560, 960 and 480 triangles


def _island_mesh(seed=0):
    """The 40 x 40 islands plus a 4 x 4 grid cut into islands of 8 and 16 triangles (below the floor of 50): 2 824 triangles."""
    return _shuffled(*_join(_islands(40, CUT), _islands(4, {1})), seed)


def _strip(n):
    return np.array([(t, t + 1, t + 2) for t in range(n)], np.int64), n + 2


def _confetti():
    """Isolated triangles with runs of edge-connected triangles at consecutive ids: {first id: length}.  Lanes: 62 -> a run inside a
    wave's last two lanes; 127, 191 -> runs that start at lane 63 and cross into the next wave; 255 -> across a workgroup of 256;
    318 -> 64 from lane 62; 448 -> exactly one wave; 1000 -> 130 over three waves; the last run ends at F - 1, followed by the tail
    wave's idle lanes.  F = 20 011 is 43 past a multiple of 64."""
    F = 20011
    runs = {62: 2, 127: 2, 191: 63, 255: 2, 318: 64, 448: 64, 600: 65, 1000: 130, 5000: 63, F - 65: 65}
    tris = np.array([(3 * t, 3 * t + 1, 3 * t + 2) for t in range(F)], np.int64)
    for s, n in runs.items():
        tris[s:s + n] = 3 * s + _strip(n)[0]
    return tris, 3 * F, runs


# ------------------------------------------------------------------------------------------------ clusters
def _gpu_clusters(tris, V):
    import surfel_native as _n
    dev = torch.device(DEV)
    t = torch.from_numpy(np.ascontiguousarray(tris, dtype=np.int32)).to(dev)
    F = int(t.shape[0])
    runs = []
    for _ in range(2):      # hooking order differs from run to run; the result may not
        label = torch.full((F,), -7, dtype=torch.int32, device=dev)
        size = torch.full((F,), -7, dtype=torch.int32, device=dev)
        alloc = _n.TorchAllocator(dev)
        _n.call(dev, "surfel_mesh_clusters", alloc.cb, None, int(V), F, t, label, size)
        runs.append((label.cpu().numpy(), size.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    return runs[0]


def _check_clusters(tris, V):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    label, size = _gpu_clusters(tris, V)
    olabel, osize = O.clusters(tris, V)
    bad = np.nonzero(label != olabel)[0]
    assert np.array_equal(label, olabel), "label differs at %d of %d triangles, first %s: %s, expected %s" % (
        len(bad), len(tris), bad[:5].tolist(), label[bad[:5]].tolist(), olabel[bad[:5]].tolist())
    assert np.array_equal(size, osize)
    assert int(size.sum()) == len(tris)
    return olabel, osize


@pytest.mark.parametrize("name", sorted(O.HAND_CLUSTERS))
def test_clusters_hand_cases(name):
    tris, V, expect = O.HAND_CLUSTERS[name]
    label, _ = _check_clusters(tris, V)
    assert label.tolist() == expect


@pytest.mark.parametrize("F", [2824, 682, 683, 2731])      # 3 F = 2 046, 2 049 and 8 193 edges around the sort's tile sizes
def test_clusters_islands(F):
    tris, V = _island_mesh()
    label, size = _check_clusters(tris[:F], V)
    if F == len(tris):
        assert sorted(size[size > 0].tolist()) == [8, 16, 240, 240, 320, 480, 560, 960]
    else:
        assert (size > 0).sum() >= 8


@pytest.mark.parametrize("order", ["ascending", "reversed", "shuffled"])
def test_clusters_strip(order):
    tris, V = _strip(8192)      # one cluster: hook chains and parent trees as long as the order allows
    if order == "reversed":
        tris = tris[::-1]
    elif order == "shuffled":
        tris = tris[np.random.default_rng(1).permutation(len(tris))]
    label, size = _check_clusters(tris, V)
    assert size[0] == 8192 and not label.any()


def test_clusters_confetti():
    tris, V, runs = _confetti()
    label, size = _check_clusters(tris, V)
    assert len(tris) % 64 != 0
    for s, n in runs.items():
        assert size[s] == n and np.all(label[s:s + n] == s)
    assert (size == 1).sum() == len(tris) - sum(runs.values())


# key bits 8, 9, 16, 17, 17, 24, 25, 25 (ids 0 .. V - 1 and the key V of out-of-range edges): 1, 2, 3 and 4 sort passes of 8 bits, so
# the sorted values end in either buffer of the ping-pong pair
@pytest.mark.parametrize("V", [200, 257, 65535, 65536, 65537, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1])
def test_clusters_pass_count(V):
    tris, V = _shuffled(*_islands(12, {2, 5, 9}), seed=V % 1000, V=V)      # 169 vertices spread over [0, V), 0 and V - 1 among them
    assert tris.min() == 0 and tris.max() == V - 1
    label, size = _check_clusters(tris, V)
    assert sorted(size[size > 0].tolist()) == [48, 48, 48, 72]


def test_clusters_bad_ids():
    tris, V = _island_mesh(seed=3)
    rng = np.random.default_rng(4)
    rows = rng.choice(len(tris), len(tris) // 100, replace=False)
    clean = O.clusters(tris, V)[1]
    for k, r in enumerate(rows):      # one id of the triangle: V + a valid id (aliases into a valid key group on ceil(log2 V) bits) or -1
        tris[r, rng.integers(3)] = V + rng.integers(V) if k % 2 == 0 else -1
    label, size = _check_clusters(tris, V)
    assert int(size.max()) <= int(clean.max())


# ------------------------------------------------------------------------------------------------ filter
def _random_floats(rng, n):
    return rng.normal(size=(n, 3)).astype(np.float32)


def _gpu_filter(verts, cols, tris, label, size, threshold):
    import surfel_native as _n
    dev = torch.device(DEV)
    V, F = len(verts), len(tris)
    dv, dc = torch.from_numpy(verts).to(dev), torch.from_numpy(cols).to(dev)
    dt = torch.from_numpy(np.ascontiguousarray(tris, dtype=np.int32)).to(dev)
    dl = torch.from_numpy(np.ascontiguousarray(label, dtype=np.int32)).to(dev)
    ds = torch.from_numpy(np.ascontiguousarray(size, dtype=np.int32)).to(dev)
    vout = torch.full((V, 3), 7.0, dtype=torch.float32, device=dev)
    cout = torch.full((V, 3), 7.0, dtype=torch.float32, device=dev)
    tout = torch.full((F, 3), -7, dtype=torch.int32, device=dev)
    n = (C.c_int64 * 2)()
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_mesh_filter", alloc.cb, None, V, F, dv, dc, dt, dl, ds, int(threshold), vout, cout, tout, n)
    return (int(n[0]), int(n[1])), vout.cpu().numpy(), cout.cpu().numpy(), tout.cpu().numpy()


def _check_filter(verts, cols, tris, label, size, threshold):
    ev, ec, et = O.filter_mesh(verts, cols, tris, label, size, threshold)
    counts, v, c, t = _gpu_filter(verts, cols, tris, label, size, threshold)
    assert counts == (len(ev), len(et))
    assert v[:counts[0]].tobytes() == ev.tobytes() and c[:counts[0]].tobytes() == ec.tobytes()      # floats bit for bit
    assert np.array_equal(t[:counts[1]], et)
    return ev, et


def _filter_mesh_input():
    """The island mesh with two degenerate triangles hung on the largest island, (a, a, b) on its edge a-b and (a, a, x) on the pair
    {a, a}: x is referenced by that triangle alone.  Six more vertices are referenced by nothing."""
    tris, nv = _join(_islands(40, CUT), _islands(4, {1}))
    a, b, x = 25 * 41 + 10, 25 * 41 + 11, nv
    tris = np.concatenate([tris, [(a, a, b), (x, a, a)]])
    tris, V = _shuffled(tris, nv + 7, seed=7)
    rng = np.random.default_rng(8)
    return _random_floats(rng, V), _random_floats(rng, V), tris


@pytest.fixture(scope="module")
def filter_input():
    verts, cols, tris = _filter_mesh_input()
    label, size = O.clusters(tris, len(verts))
    assert sorted(size[size > 0].tolist()) == [8, 16, 240, 240, 320, 480, 560, 962]
    return verts, cols, tris, label, size


@pytest.mark.parametrize("threshold", [0, 1, 480, 481, 963])      # 480: >= keeps the island of exactly 480; 963: above the largest
def test_filter_thresholds(filter_input, threshold):
    verts, cols, tris, label, size = filter_input
    ev, et = _check_filter(verts, cols, tris, label, size, threshold)
    kept = sum(s for s in (8, 16, 240, 240, 320, 480, 560, 962) if s >= threshold)
    assert len(et) == kept - (2 if threshold <= 962 else 0)           # the two degenerate triangles leave last ...
    assert len(ev) == {0: 1707, 1: 1707, 480: 1149, 481: 862, 963: 0}[threshold]      # ... and x stays: rows + 1 times 41 vertices per island, + x
    assert len(ev) <= len(verts) - 6                                  # the unreferenced vertices never stay


@pytest.mark.parametrize("V", [1, 4095, 4096, 4097, 8193])      # one element, one short of a scan tile, a full tile, one over, two tiles + 1
def test_filter_scan_tile_edges(V):
    for F in (1, 4095, 4096, 4097, 8193):
        rng = np.random.default_rng(1000 * V + F)
        tris = rng.integers(0, V, (F, 3))
        rows = rng.choice(F, F // 100, replace=False)
        tris[rows, rng.integers(0, 3, len(rows))] = np.where(rng.random(len(rows)) < 0.5, -1, V)      # ids out of range: dropped
        label = rng.integers(0, F, F)              # the filter takes label / size as given: an arbitrary keep pattern
        size = rng.integers(0, 4, F)
        _, et = _check_filter(_random_floats(rng, V), _random_floats(rng, V), tris, label, size, 2)
        assert V == 1 or F == 1 or 0 < len(et) < F


def _post_process(verts, cols, tris, k):
    import surfel_mesh
    dev = torch.device(DEV)
    mesh = surfel_mesh.TriangleMesh(torch.from_numpy(verts).to(dev), torch.from_numpy(np.ascontiguousarray(tris, dtype=np.int32)).to(dev),
                                    torch.from_numpy(cols).to(dev))
    return surfel_mesh.post_process_mesh(mesh, k).numpy()


@pytest.mark.parametrize("k,threshold", [(1, 962), (5, 240), (6, 240), (7, 50), (9, 50), (1000, 50)])      # 5 / 6: a tie at the k-th place; 9, 1000: k past the 8 clusters
def test_post_process_mesh(filter_input, k, threshold):
    verts, cols, tris, label, size = filter_input
    assert O.post_threshold(size, k) == threshold
    ev, ec, et = O.filter_mesh(verts, cols, tris, label, size, threshold)
    post = _post_process(verts, cols, tris, k)
    assert post.vertices.tobytes() == ev.tobytes() and post.vertex_colors.tobytes() == ec.tobytes()
    assert np.array_equal(post.triangles, et) and len(et) > 0


def test_post_process_mesh_all_below_floor():
    tris, V = _shuffled(*_islands(6, {1, 3}), seed=2)      # islands of 12, 12 and 24 triangles: all below 50
    rng = np.random.default_rng(3)
    verts, cols = _random_floats(rng, V), _random_floats(rng, V)
    size = O.clusters(tris, V)[1]
    assert sorted(size[size > 0].tolist()) == [12, 12, 24] and O.post_threshold(size, 1) == 50
    post = _post_process(verts, cols, tris, 1)
    assert post.vertices.shape == (0, 3) and post.vertex_colors.shape == (0, 3) and post.triangles.shape == (0, 3)


def test_filter_scan_outer_loop():
    """F = 2^24 + 4097 is 4 098 scan tiles, so the one-workgroup scan of the tile sums takes two trips through its loop (4 096 sums
    per trip); nothing smaller reaches the second trip.  About 0.7 GB on the device, the one large case of this file."""
    import surfel_native as _n
    dev = torch.device(DEV)
    F, V = 2 ** 24 + 4097, 1000
    g = torch.Generator(device=dev).manual_seed(11)
    tris = torch.randint(0, V, (F, 3), dtype=torch.int32, device=dev, generator=g)
    label = torch.arange(F, dtype=torch.int32, device=dev)
    size = torch.randint(0, 2, (F,), dtype=torch.int32, device=dev, generator=g)      # threshold 1: about half kept
    verts = torch.rand((V, 3), dtype=torch.float32, device=dev, generator=g)
    cols = torch.rand((V, 3), dtype=torch.float32, device=dev, generator=g)
    vout, cout = torch.zeros_like(verts), torch.zeros_like(cols)
    tout = torch.full((F, 3), -7, dtype=torch.int32, device=dev)
    n = (C.c_int64 * 2)()
    alloc = _n.TorchAllocator(dev)
    _n.call(dev, "surfel_mesh_filter", alloc.cb, None, V, F, verts, cols, tris, label, size, 1, vout, cout, tout, n)
    t = tris.cpu().numpy()
    keep = size.cpu().numpy() >= 1
    assert np.bincount(t[keep].reshape(-1), minlength=V).all()      # every vertex is referenced, so the vertex map is the identity
    kept = keep & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    expect = t[kept]      # order-preserving compaction
    assert 0.45 * F < len(expect) < 0.55 * F
    assert kept[2 ** 24:].sum() > 1000      # kept triangles in the tiles whose sums the loop's second trip scans
    assert (int(n[0]), int(n[1])) == (V, len(expect))
    assert torch.equal(vout, verts) and torch.equal(cout, cols)
    got = tout[:len(expect)].cpu().numpy()
    assert np.array_equal(got, expect)


# ------------------------------------------------------------------------------------------------ marching cubes on crafted fields
MC_VS, MC_TR = 0.05, 0.2
MC_ORIGIN, MC_DIMS = (-2, -2, -2), (4, 4, 4)


def _plane_view(t, W=24, H=16, f=20.0, d=0.3):
    """A fronto-parallel plane at depth d seen by an axis-aligned camera with extrinsic translation t: (depth, camera block)"""
    cam = np.zeros(16, np.float32)
    cam[[0, 5, 10]] = 1.0
    cam[[3, 7, 11]] = t
    cam[12:] = [f, f, (W - 1) / 2, (H - 1) / 2]
    return np.full((H, W), d, np.float32), cam


def _mc_views():
    # blocks x {-2, -1}, y {-1, 0}, z 0 and blocks x {0, 1}, y {-1, 0}, z -1: both ends of the table's x range (the neighbour blocks
    # -3 and 2 lie outside the table), negative coordinates, and allocated blocks next to unallocated ones inside the table
    return [_plane_view((0.9, 0.0, 0.0)), _plane_view((-0.9, 0.0, 0.6))]


def _mc_blocks():
    b = set().union(*(O.touched_blocks(d, cam, MC_VS, MC_TR) for d, cam in _mc_views()))
    return np.array(sorted(b, key=lambda c: (c[2], c[1], c[0])), np.int64)


def _mc_field(kind, nvox):
    """(tsdf, weight, rgb) float32: 'normal' i.i.d. N(0, 1) with colours in [0, 255]; 'holes' the same with 10 % of the weights 0;
    'zeros' as 'holes' with 5 % of the values 0.0 and 5 % -0.0 (both outside: inside means tsdf < 0)"""
    rng = np.random.default_rng(17)
    tsdf = rng.normal(size=nvox).astype(np.float32)
    rgb = rng.uniform(0, 255, (nvox, 3)).astype(np.float32)
    w = np.ones(nvox, np.float32)
    u = rng.random(nvox)
    z = rng.random(nvox)
    if kind != "normal":
        w[u < 0.1] = 0
    if kind == "zeros":
        tsdf[z < 0.05] = 0.0
        tsdf[(z >= 0.05) & (z < 0.1)] = -0.0
    return tsdf, w, rgb


@pytest.fixture(scope="module")
def mc_volume():
    import surfel_mesh
    dev = torch.device(DEV)
    vol = surfel_mesh.TsdfVolume(MC_VS, MC_TR, MC_ORIGIN, MC_DIMS, 1 << 30, dev)
    for d, cam in _mc_views():
        vol.mark(torch.from_numpy(d).to(dev), torch.from_numpy(cam).to(dev))
    vol.allocate()
    coords = vol.blocks()[0]
    assert np.array_equal(coords, _mc_blocks()) and len(coords) == 8
    assert coords.min() == -2 and coords[:, 0].max() == 1
    return vol, coords


@pytest.mark.parametrize("kind", ["normal", "holes", "zeros"])
def test_marching_cubes_crafted_fields(mc_volume, kind):
    vol, coords = mc_volume
    nvox = len(coords) * 4096
    tsdf, w, rgb = _mc_field(kind, nvox)
    vol._tensor("tsdf_rgb", torch.float32, (nvox, 4)).copy_(torch.from_numpy(np.concatenate([tsdf[:, None], rgb], 1)))
    vol._tensor("weight", torch.float32, (nvox,)).copy_(torch.from_numpy(w))
    valid, case = O.cube_cases(coords, tsdf, w)
    if kind == "normal":      # a condition on the input: every one of the 256 cube cases is there
        assert np.array_equal(np.unique(case[valid]), np.arange(256))
    else:
        assert 0.1 < valid.mean() < 0.6      # holes take most cubes away, not all
    if kind == "zeros":
        assert (tsdf == 0).mean() > 0.09 and np.signbit(tsdf[tsdf == 0]).any() and not np.signbit(tsdf[tsdf == 0]).all()
    verts, cols, tris = O.marching_cubes(coords, tsdf.astype(np.float64), w.astype(np.float64), rgb.astype(np.float64), MC_VS)
    mesh = vol.extract()
    assert len(tris) > 10000
    assert mesh.vertices.shape[0] == len(verts) and mesh.triangles.shape[0] == len(tris)
    assert np.array_equal(mesh.triangles.cpu().numpy(), tris)
    # vertices: coordinates stay inside +-32 voxels, where half an fp32 ulp is 1.9e-6 voxel; s = a / (a - b) has no cancellation
    # (the signs differ), so x + 0.5 + s and the product with the voxel size stay within 1e-5 voxel
    dv = np.max(np.abs(mesh.vertices.cpu().numpy() - verts))
    # colours: inputs <= 255 and four fp32 roundings.  A numpy float32 restatement of the kernel's formula on these fields differs
    # from the fp64 oracle by at most 1.3e-7 on each of the three fields (and its vertices by 2.1e-6 voxel)
    dc = np.max(np.abs(mesh.vertex_colors.cpu().numpy() - cols))
    print("%s: V %d F %d, max vertex error %.3g voxel, max colour error %.3g" % (kind, len(verts), len(tris), dv / MC_VS, dc))
    assert dv < 1e-5 * MC_VS
    assert dc < 1e-5


@pytest.mark.parametrize("origin,dims", [((-1, 0, 0), (1, 1, 1)), ((-8, -8, -8), (16, 16, 16)), ((-8, -120, 0), (17, 241, 1))])
def test_allocate_scan_tile_edges(origin, dims):
    """The allocation scans one flag per table entry: tables of one entry, of one full scan tile (4 096) and of one entry more.  The blocks
    found are the oracle's in table order.  The table of one block also gives the extraction its shortest scan, one tile of voxels."""
    import surfel_mesh
    dev = torch.device(DEV)
    vol = surfel_mesh.TsdfVolume(MC_VS, MC_TR, origin, dims, 1 << 30, dev)
    for d, cam in _mc_views():
        vol.mark(torch.from_numpy(d).to(dev), torch.from_numpy(cam).to(dev))
    vol.allocate()
    want = np.array([b for b in _mc_blocks() if all(o <= x < o + n for x, o, n in zip(b, origin, dims))], np.int64)
    coords = vol.blocks()[0]
    assert len(want) == {1: 1, 4096: 8, 4097: 4}[int(np.prod(dims))] and np.array_equal(coords, want)
    if len(want) == 1:
        tsdf, w, rgb = _mc_field("normal", 4096)
        vol._tensor("tsdf_rgb", torch.float32, (4096, 4)).copy_(torch.from_numpy(np.concatenate([tsdf[:, None], rgb], 1)))
        vol._tensor("weight", torch.float32, (4096,)).copy_(torch.from_numpy(w))
        verts, _, tris = O.marching_cubes(coords, tsdf.astype(np.float64), w.astype(np.float64), rgb.astype(np.float64), MC_VS)
        mesh = vol.extract()
        assert len(tris) > 1000 and mesh.vertices.shape[0] == len(verts) and np.array_equal(mesh.triangles.cpu().numpy(), tris)


# ------------------------------------------------------------------------------------------------ fusion edges
FU_VS, FU_TR, FU_DT = 0.03, 0.12, 10.0
FU_W, FU_H = 64, 48


def _look_at_block(eye, W, H, f):
    """camera block of a camera at `eye` that looks at the origin"""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([np.concatenate([R, (-R @ eye)[:, None]], 1).reshape(-1), [f, f, (W - 1) / 2, (H - 1) / 2]]).astype(np.float32)


def _sphere_views(radius=0.55):
    """Six views of a sphere at the origin, one from near each of +-x, +-y, +-z; 0 (invalid) off the sphere.  The sphere's caps lie
    past +-0.48, the faces of a table of 2 x 2 x 2 blocks of 16 voxels of 0.03 around the origin.  The cameras stand well off the
    axes: seen along an axis, rows of voxel centres project onto pixel borders and the oracle exempts more than test_fusion_parity's
    cap of 1e-3 allows; with these views it exempts 3e-5 of the voxels of the small table and 2e-5 of the large one."""
    rng = np.random.default_rng(21)
    views = []
    for eye in ((2.1, 0.57, 0.31), (-2.1, 0.43, -0.37), (0.47, 2.1, 0.53), (-0.39, -2.1, 0.41), (0.53, -0.33, 2.1), (0.29, 0.61, -2.1)):
        cam = _look_at_block(eye, FU_W, FU_H, 88.0)
        R = cam[:12].reshape(3, 4)[:, :3].astype(np.float64)
        v, u = np.mgrid[0:FU_H, 0:FU_W].astype(np.float64)
        dw = np.stack([(u - cam[14]) / cam[12], (v - cam[15]) / cam[13], np.ones_like(u)], -1) @ R      # world direction of the z = 1 ray
        o = np.asarray(eye, np.float64)
        b, a, c = dw @ o, (dw * dw).sum(-1), o @ o - radius ** 2
        disc = b * b - a * c
        d = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, 0.0).astype(np.float32)
        views.append((d, rng.random((3, FU_H, FU_W)).astype(np.float32), cam))
    return views


def _fuse_explicit(views, origin, dims):
    """prepare_view, mark, allocate and integrate into an explicit table; returns (volume, [(prepared depth, rgb8, cam)])"""
    import surfel_mesh
    dev = torch.device(DEV)
    vol = surfel_mesh.TsdfVolume(FU_VS, FU_TR, origin, dims, 1 << 30, dev)
    prep = []
    for d, rgb, cam in views:
        dd, rgba = surfel_mesh.prepare_view(torch.from_numpy(d).to(dev)[None], torch.from_numpy(rgb).to(dev), None, FU_DT)
        prep.append((dd, rgba, torch.from_numpy(cam).to(dev)))
        vol.mark(dd, prep[-1][2])
    vol.allocate()
    for dd, rgba, cam in prep:
        vol.integrate(dd, rgba, cam)
    return vol, [(p[0].cpu().numpy(), (np.clip(rgb, 0, 1) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0), cam)
                 for p, (_, rgb, cam) in zip(prep, views)]


def _check_fusion(vol, ora, min_voxels):
    """test_fusion_parity's comparison: its tolerances and its exemption rule"""
    coords, trgb, wgt = vol.blocks()
    assert np.array_equal(coords, ora["coords"])
    t = trgb.cpu().numpy().reshape(-1, 4).astype(np.float64)
    w = wgt.cpu().numpy().reshape(-1)
    ex = ora["exempt"]
    print("exempt voxels: %d of %d" % (ex.sum(), ex.size))
    assert ex.mean() < 1e-3
    ok = ~ex
    bad = np.nonzero(ok & (w != ora["weight"]))[0]
    assert np.array_equal(w[ok], ora["weight"][ok]), "weight differs at %d voxels, first %s: %s, expected %s" % (
        len(bad), bad[:4].tolist(), w[bad[:4]].tolist(), ora["weight"][bad[:4]].tolist())
    m = ok & (w > 0)
    assert m.sum() > min_voxels
    assert np.max(np.abs(t[m, 0] - ora["tsdf"][m])) < 1e-5
    assert np.max(np.abs(t[m, 1:] - ora["rgb"][m])) < 1e-3


def test_fusion_table_smaller_than_scene():
    origin, dims = (-1, -1, -1), (2, 2, 2)
    views = _sphere_views()
    vol, oviews = _fuse_explicit(views, origin, dims)
    touched = set().union(*(O.touched_blocks(d, cam, FU_VS, FU_TR) for d, _, cam in oviews))
    lo, hi = np.array(sorted(touched)).min(0), np.array(sorted(touched)).max(0)
    assert np.all(lo < -1) and np.all(hi > 0)      # the observed points leave the table on each of its six sides ...
    ora = O.fuse(oviews, FU_VS, FU_TR, table=(origin, dims))
    assert len(ora["coords"]) == 8                 # ... and every block of the table is touched
    _check_fusion(vol, ora, 10000)


def test_fusion_invalid_depths_are_holes():
    views = _sphere_views()
    d = views[0][0].copy()
    hole = d.copy()
    patches = [(np.nan, 0.0), (np.inf, 0.0), (-np.inf, -np.inf), (-1e-9, -1e-9), (-1.0, -1.0)]      # (raw depth, what prepare_view leaves)
    prepared = d.copy()
    for k, (x, y) in enumerate(patches):
        rows, colsl = slice(16 + 3 * k, 19 + 3 * k), slice(20, 44)      # bands across the sphere's image
        assert np.all(d[rows, colsl] > 0)
        d[rows, colsl], prepared[rows, colsl], hole[rows, colsl] = x, y, 0.0
    vol, oviews = _fuse_explicit([(d,) + views[0][1:]] + views[1:], (-2, -2, -2), (4, 4, 4))
    assert oviews[0][0].tobytes() == prepared.tobytes()      # NaN and +inf are not <= depth_trunc: 0; the rest passes as it is
    ora = O.fuse([(hole,) + oviews[0][1:]] + oviews[1:], FU_VS, FU_TR)      # every such pixel acts as a hole
    _check_fusion(vol, ora, 20000)
