"""CPU checks of the TSDF mesh extraction: the generated case table, the numpy oracle (tests/mesh_oracle.py) against closed forms,
the bounding sphere, PLY / cameras.json round trips and the library surface of include/surfel_mesh.h."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import gen_mc_table as MC  # noqa: E402
import mesh_oracle as O  # noqa: E402


# ------------------------------------------------------------------------------------------------ case table
def test_table_header_is_generated():
    assert open(MC.HEADER).read() == MC.render_header()


def _face_of_segment(e1, e2):
    """faces (index into MC.FACES) that hold both edges"""
    out = []
    for k, (cyc, _) in enumerate(MC.FACES):
        fe = {MC.edge_of(cyc[i], cyc[(i + 1) % 4]) for i in range(4)}
        if e1 in fe and e2 in fe:
            out.append(k)
    return out


@pytest.mark.parametrize("case", range(256))
def test_table_boundary_is_face_pairing(case):
    tris = MC.triangles(case)
    directed = {}
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            directed[(a, b)] = directed.get((a, b), 0) + 1
    # boundary = directed edges without their reverse (interior fan diagonals cancel)
    boundary = sorted(k for k, c in directed.items() for _ in range(c) if directed.get((k[1], k[0]), 0) == 0)
    expected = sorted(s for cyc, n in MC.FACES for s in MC.face_segments(case, cyc, n))
    assert boundary == expected
    for a, b in boundary:
        assert len(_face_of_segment(a, b)) == 1


@pytest.mark.parametrize("case", range(1, 255))
def test_table_normals_follow_sign_gradient(case):
    inside = np.array([(case >> c) & 1 for c in range(8)], bool)
    pos = np.array([MC.corner_pos(c) for c in range(8)])
    grad_dir = pos[~inside].mean(0) - pos[inside].mean(0)      # toward increasing tsdf
    total = np.zeros(3)
    for t in MC.triangles(case):
        p = [MC.edge_mid(e) for e in t]
        total += np.cross(p[1] - p[0], p[2] - p[0])
    if np.linalg.norm(grad_dir) > 1e-9:
        assert np.dot(total, grad_dir) > 0, case


# ------------------------------------------------------------------------------------------------ oracle marching cubes
def test_oracle_sphere_closed_manifold():
    r, c = 13.3, np.array([24.2, 23.7, 24.9])
    coords, tsdf, w, rgb = O.sphere_volume(r, c, 3)
    verts, cols, tris = O.marching_cubes(coords, tsdf, w, rgb, 1.0)
    assert len(tris) > 500
    assert O.closed_oriented_manifold(tris)
    assert O.euler(verts, tris) == 2
    assert np.all(np.bincount(tris.reshape(-1), minlength=len(verts)) > 0)      # no unreferenced vertex
    # vertices on the interpolated zero crossing: the tsdf is linear along the grid axes only approximately, so compare against the
    # crossing of the linear interpolant itself (the grid values at both ends of the vertex's edge)
    g = verts - 0.5
    lo = np.floor(g + 1e-9)
    frac = g - lo
    ax = np.argmax(frac, axis=1)
    a = lo.astype(np.int64)
    b = a.copy(); b[np.arange(len(a)), ax] += 1
    sd = lambda p: (np.linalg.norm(p + 0.5 - c, axis=1) - r) / 4.0
    ta, tb = sd(a), sd(b)
    s = ta / (ta - tb)
    assert np.max(np.abs(s - frac[np.arange(len(a)), ax])) < 1e-3
    n = O.face_normals(verts, tris)
    centroid = verts[tris].mean(1)
    area = np.linalg.norm(n, axis=1) > 1e-9      # (fans over collinear crossings leave zero-area triangles)
    assert area.mean() > 0.99 and np.all(np.einsum("ij,ij->i", n, centroid - c)[area] > 0)
    assert np.allclose(cols, 128.0 / 255.0)


def test_oracle_tsdf_fronto_parallel_plane():
    W, H, vs, tr = 64, 48, 0.05, 0.25
    fx = fy = 50.0
    cam = np.zeros(16, np.float32)
    cam[[0, 5, 10]] = 1.0
    cam[12:] = [fx, fy, (W - 1) / 2, (H - 1) / 2]
    depth = np.full((H, W), 2.0, np.float32)
    rgb8 = np.full((H, W, 3), 200, np.uint8)
    vol = O.fuse([(depth, rgb8, cam)], vs, tr)
    g = O.voxel_coords(vol["coords"])
    c = (g + 0.5) * np.float32(vs)
    m = vol["weight"] > 0
    assert m.sum() > 1000
    u = np.floor(fx * c[:, 0] / c[:, 2] + (W - 1) / 2 + 0.5)
    v = np.floor(fy * c[:, 1] / c[:, 2] + (H - 1) / 2 + 0.5)
    stretch = np.sqrt(1 + ((u - (W - 1) / 2) / fx) ** 2 + ((v - (H - 1) / 2) / fy) ** 2)
    sdf = (2.0 - c[:, 2]) * stretch
    t = np.minimum(1.0, sdf / np.float32(tr))
    expect = (c[:, 2] > 0) & (u >= 0) & (v >= 0) & (u < W) & (v < H) & (sdf > -np.float32(tr))
    ok = ~vol["exempt"]
    assert np.array_equal(m[ok], expect[ok])
    assert np.allclose(vol["tsdf"][m & ok], t[m & ok], atol=1e-12)
    assert np.allclose(vol["rgb"][m], 200.0)


# ------------------------------------------------------------------------------------------------ post-processing references
@pytest.mark.parametrize("name", sorted(O.HAND_CLUSTERS))
def test_oracle_clusters_hand_cases(name):
    tris, V, expect = O.HAND_CLUSTERS[name]
    label, size = O.clusters(tris, V)
    assert label.tolist() == expect
    assert size.tolist() == [expect.count(t) for t in range(len(tris))]      # the count at root ids, 0 elsewhere


def test_oracle_clusters_counts():
    n = {name: len(set(expect)) for name, (_, _, expect) in O.HAND_CLUSTERS.items()}
    assert n == dict(single=1, bow_tie=2, edge_same_winding=1, edge_opposite_winding=1, fan_of_5=1, duplicate=1, repeated_index=2,
                     bad_id_alias=2)
    # an edge with an id out of range changes nothing for the others: -1, V and V + id alike
    base = [(0, 1, 2), (2, 1, 3), (4, 5, 6)]
    for bad in (-1, 7, 7 + 1, 2 ** 31 - 1):
        label, size = O.clusters(base + [(1, 2, bad), (bad, 5, 4), (bad, bad, bad)], 7)
        assert label.tolist() == [0, 0, 2, 0, 2, 5] and size.tolist() == [3, 0, 2, 0, 0, 1]
    label, size = O.clusters(np.zeros((0, 3), np.int64), 4)
    assert label.shape == (0,) and size.shape == (0,)


def _six_triangle_mesh():
    """10 vertices, 6 triangles.  Cluster A: T0, T1 (edge 1-2), T3 = (1, 1, 3) (edge 1-3 of T1) and T5 = (7, 1, 1) (the pair {1, 1} of
    T3); cluster B: T2, T4 (edge 4-5).  Vertex 7 is referenced by the degenerate T5 alone, vertex 9 by nothing."""
    tris = np.array([(0, 1, 2), (2, 1, 3), (4, 5, 6), (1, 1, 3), (5, 4, 8), (7, 1, 1)], np.int64)
    rng = np.random.default_rng(5)
    verts = rng.integers(0, 2 ** 32, (10, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bit pattern, NaNs too
    cols = rng.integers(0, 2 ** 32, (10, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return verts, cols, tris


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32).tolist()


def test_oracle_filter_mesh_six_triangles():
    verts, cols, tris = _six_triangle_mesh()
    label, size = O.clusters(tris, len(verts))
    assert label.tolist() == [0, 0, 2, 0, 2, 0] and size.tolist() == [4, 0, 2, 0, 0, 0]
    # threshold 3: B (2 triangles) goes with its vertices 4, 5, 6, 8; 7 stays through T5; 9 is unreferenced; T3 and T5 leave last
    v, c, t = O.filter_mesh(verts, cols, tris, label, size, 3)
    assert _bits(v) == _bits(verts[[0, 1, 2, 3, 7]]) and _bits(c) == _bits(cols[[0, 1, 2, 3, 7]])
    assert v.dtype == np.float32 and t.tolist() == [[0, 1, 2], [2, 1, 3]]
    # threshold 2: >= keeps B at exactly its size; only vertex 9 goes
    v, c, t = O.filter_mesh(verts, cols, tris, label, size, 2)
    assert _bits(v) == _bits(verts[:9]) and _bits(c) == _bits(cols[:9])
    assert t.tolist() == [[0, 1, 2], [2, 1, 3], [4, 5, 6], [5, 4, 8]]
    v, c, t = O.filter_mesh(verts, cols, tris, label, size, 5)
    assert v.shape == (0, 3) and c.shape == (0, 3) and t.shape == (0, 3)
    # T1 with an id out of range: it is dropped whatever its cluster, its edge 2-1 still links it to T0, its other edges link nothing,
    # so T3 and T5 form a cluster of their own; vertex 3 now survives through the degenerate T3 alone
    tris[1] = (2, 1, 10)
    label, size = O.clusters(tris, len(verts))
    assert label.tolist() == [0, 0, 2, 3, 2, 3] and size.tolist() == [2, 0, 2, 2, 0, 0]
    v, c, t = O.filter_mesh(verts, cols, tris, label, size, 2)
    assert _bits(v) == _bits(verts[:9]) and t.tolist() == [[0, 1, 2], [4, 5, 6], [5, 4, 8]]


def test_oracle_post_threshold():
    size = np.array([300, 0, 0, 120, 120, 0, 120, 60, 0, 7])      # clusters of 300, 120, 120, 120, 60, 7
    assert [O.post_threshold(size, k) for k in (1, 2, 3, 4, 5)] == [300, 120, 120, 120, 60]      # ties at the k-th place
    assert O.post_threshold(size, 6) == 50                       # the 6th largest is 7: the floor of 50 holds
    assert O.post_threshold(size, 7) == 50 and O.post_threshold(size, 1000) == 50      # fewer than k clusters
    assert O.post_threshold(np.array([49, 0, 12, 3]), 1) == 50   # all clusters below 50
    assert O.post_threshold(np.zeros(0, np.int64), 1) == 50


def test_oracle_fuse_invalid_depths_are_holes():
    W, H, vs, tr = 32, 24, 0.05, 0.25
    cam = np.zeros(16, np.float32)
    cam[[0, 5, 10]] = 1.0
    cam[12:] = [25.0, 25.0, (W - 1) / 2, (H - 1) / 2]
    depth = np.full((H, W), 2.0, np.float32)
    rgb8 = np.full((H, W, 3), 200, np.uint8)
    bad = depth.copy()
    hole = depth.copy()
    for k, x in enumerate((np.nan, -np.inf, -1e-9, -1.0, 0.0)):
        bad[4:8, 4 * k + 2:4 * k + 5] = x
        hole[4:8, 4 * k + 2:4 * k + 5] = 0.0
    a, b = O.fuse([(bad, rgb8, cam)], vs, tr), O.fuse([(hole, rgb8, cam)], vs, tr)
    assert np.array_equal(a["coords"], b["coords"]) and np.array_equal(a["weight"], b["weight"])
    assert np.array_equal(a["tsdf"], b["tsdf"]) and np.isfinite(a["tsdf"]).all()
    assert (a["weight"] > 0).sum() > 1000


# ------------------------------------------------------------------------------------------------ bounding sphere
def test_bounding_sphere_orbit():
    sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
    torch = pytest.importorskip("torch")  # noqa: F841
    import surfel_mesh
    rng = np.random.default_rng(3)
    c2ws = []
    for _ in range(12):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        eye = 3.5 * d
        z = -d
        x = np.cross([0.0, 1.0, 0.3], z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        m = np.eye(4); m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
        c2ws.append(m)
    center, radius = surfel_mesh.bounding_sphere(np.array(c2ws))
    assert np.max(np.abs(center)) < 1e-9 and abs(radius - 3.5) < 1e-9


# ------------------------------------------------------------------------------------------------ I/O
def test_triangle_mesh_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
    import surfel_io
    rng = np.random.default_rng(0)
    mesh = type("M", (), {})()
    mesh.vertices = rng.normal(size=(50, 3)).astype(np.float32)
    mesh.vertex_colors = (rng.integers(0, 256, (50, 3)) / 255.0).astype(np.float32)
    mesh.triangles = rng.integers(0, 50, (80, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    surfel_io.write_triangle_mesh(p, mesh)
    v, t, c = surfel_io.read_triangle_mesh(p)
    assert np.array_equal(v, mesh.vertices) and np.array_equal(t, mesh.triangles)
    assert np.allclose(c, mesh.vertex_colors, atol=0.5 / 255)
    assert open(p, "rb").read(400).count(b"property list uchar int vertex_indices") == 1


def test_cameras_json_round_trip(tmp_path):
    torch = pytest.importorskip("torch")  # noqa: F841
    sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
    import surfel_io
    fix = json.load(open(os.path.join(REPO, "tests", "golden", "ref_cameras.json")))
    cams = surfel_io.read_cameras_json(os.path.join(REPO, "tests", "golden", "ref_cameras.json"), device="cpu")
    meta = json.load(open(os.path.join(REPO, "tests", "golden", "ref_cameras_source.json")))
    assert len(cams) == len(fix) == len(meta)
    for cam, m in zip(cams, meta):
        assert np.allclose(cam.R, np.array(m["R"]), atol=1e-12)
        assert np.allclose(cam.T, np.array(m["T"]), atol=1e-12)
        assert abs(cam.FoVx - m["FoVx"]) < 1e-12 and abs(cam.FoVy - m["FoVy"]) < 1e-12
        assert (cam.image_width, cam.image_height) == (m["width"], m["height"])


# ------------------------------------------------------------------------------------------------ library surface
def _lib():
    return os.path.join(REPO, "2d-gaussian-splatting_amd", "lib", "libsurfel_hip.so")


def test_mesh_header_exported():
    sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", "surfel_mesh.h")).read(), re.M)
    assert len(decl) == 11
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.MESH_EXPORTS) == sorted(decl)


def test_mesh_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("mesh_tsdf.hip"))
    names = [k for k in ks if "mesh_" in k or "scan_" in k or "uf_" in k or "edge_" in k or "filter_" in k]
    assert len(names) >= 15, names
    for k in names:
        assert int(ks[k][1].get("private_segment_fixed_size", 0)) == 0, k


def test_scan_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("device_scan.hip"))
    for want in ("scan_sums_kernel", "scan_top_kernel", "scan_apply_kernel"):
        names = [k for k in ks if want in k]
        assert len(names) == 1, (want, list(ks))
        assert ks[names[0]][1]["private_segment_fixed_size"] == 0, want
