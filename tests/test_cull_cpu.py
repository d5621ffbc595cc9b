"""CPU checks of the view culling (CULL.md): the point-mask oracle and the trajectory reader against what the reference's own
cull_mesh.py computed (tests/golden/ref_tnt_cull.npz, minted by tests/golden/make_golden_tnt_cull.py), the conditions the scene has to
meet so that the caps of the GPU tests cannot hide a failure, the compaction tail against a literal restatement, the host-side readers
and the library surface (header, exports, signatures, kernel resources)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cull_oracle as O
import cull_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_cull.h"


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_tnt_cull.npz"))
    assert json.loads(str(z["scene"])) == json.loads(S.fingerprint()), "the fixture was minted from another scene: run make_golden_tnt_cull.py"
    return z


# ------------------------------------------------------------------------------------------------ the oracle against the reference
def test_point_mask_oracle_reproduces_reference(golden):
    """The reference's own Mesher.point_masks on the fixture's depth images: the mask exactly, and the counts on every vertex that has no
    undecided pair (torch's CPU grid_sample and matmul may order their fp32 sums differently)."""
    v = S.mesh()[0]
    ref = O.scene_reference(S.FIXTURE_SIZE)
    assert np.array_equal(golden["depth"], ref["d64"].astype(np.float32))
    r = O.point_masks(v, golden["depth"], ref["w2c"], ref["intr"], 0.005, 20)
    assert np.array_equal(r["mask"], golden["mask"])
    clear = ~r["undecided_pairs"].any(0)
    print("fixture: %d of %d vertices kept, %d vertices with an undecided pair" % (golden["mask"].sum(), len(v), (~clear).sum()))
    assert np.array_equal(r["counts"][clear], golden["counts"][clear]) and clear.mean() > 0.9
    assert np.array_equal(golden["mask"], golden["counts"] >= 20) and 0.1 < 1 - golden["mask"].mean() < 0.9


def test_json_reader_reproduces_reference(golden, tmp_path):
    sys.path.insert(0, PKG)
    import surfel_cull as P
    path = str(tmp_path / "transforms.json")
    with open(path, "w") as f:
        json.dump(S.transforms_json(), f)
    got = P.read_trajectory(path)
    assert got.shape == golden["traj"].shape == (S.TRAJ["frames"], 4, 4) and got.dtype == np.float32
    assert np.max(np.abs(got - golden["traj"])) <= 1e-6
    assert abs(np.abs(got[:, :3, 3]).max() - 1.0) < 1e-6 and np.array_equal(got[:, 3], np.tile([0, 0, 0, 1], (len(got), 1)))


# ------------------------------------------------------------------------------------------------ conditions on the oracle alone
@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_scene_conditions(size):
    """What keeps the caps of the GPU tests from hiding a failure.  The covered share is asked of every ordinary view and of the mean
    over all views: the arc's last camera sees only the triangle that fills its screen (100 %), the camera that looks away sees nothing."""
    ref = O.scene_reference(size)
    und, d64 = ref["und"], ref["d64"]
    share = und.mean((1, 2))
    print("%s: undecided pixels per image: max %d = %.4f %%; fp32 twin deviation %.3g" % (size, und.sum((1, 2)).max(), 100 * share.max(), ref["deviation"]))
    assert share.max() <= 1e-3
    cover = (d64 > 0).mean((1, 2))
    n = S.SCENE["views"]
    assert ((cover[:n - 1] > 0.25) & (cover[:n - 1] < 0.75)).all() and 0.25 < cover.mean() < 0.75, cover
    assert cover[n - 1] == 1.0 and cover[n] == 0.0
    # the last camera's two triangles: the one that crosses the eye plane is in front of the filler on part of the screen
    nearest = O.depth_image(ref["verts"], ref["tris"], ref["w2c"][n - 1], ref["intr"], ref["H"], ref["W"], S.SCENE["znear"], S.SCENE["zfar"])[1]
    first = len(ref["tris"]) - 8
    assert set(np.unique(nearest)) == {first, first + 1} and 0.02 < (nearest == first).mean() < 0.9
    for mv in S.MIN_VIEWS:
        m = ref["masks"][mv]
        culled = 1 - m["mask"].mean()
        print("%s, min_views %d: culled %.3f, %d undecided vertices, %d undecided pairs" % (size, mv, culled, m["undecided"].sum(), m["undecided_pairs"].sum()))
        assert 0.1 < culled < 0.9
        if size == S.FIXTURE_SIZE:      # the size the vertex tests run at
            assert m["undecided"].mean() <= 1e-3
    small, large = O.size_classes(ref["verts"], ref["tris"], ref["w2c"], ref["intr"], ref["H"], ref["W"], S.SCENE["znear"], S.SCENE["zfar"])
    print("%s: %d small and %d large (view, triangle) pairs" % (size, small, large))
    assert small > 1000 and large > 100
    assert 0 < ref["deviation"] < 1e-2


def test_special_triangles_change_nothing():
    a, b = O.scene_reference(S.FIXTURE_SIZE), O.scene_reference(S.FIXTURE_SIZE, special=False)
    assert len(a["tris"]) == len(b["tris"]) + 5 and np.array_equal(a["d64"], b["d64"])


def test_anchor_is_a_plane():
    """the closed form of the anchor quad against the oracle (the GPU test compares the kernel with the closed form alone)"""
    v, t, n, d = S.quad_anchor()
    H, W = S.SIZES["large"][:2]
    k = S.intrinsics("large")
    got = O.depth_image(v, t, np.eye(4, dtype=np.float32), k, H, W, 0.01, 20.0)[0]
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    want = d / (n[0] * (xs - np.float32(k[2])) / np.float32(k[0]) + n[1] * (ys - np.float32(k[3])) / np.float32(k[1]) + n[2])
    assert np.max(np.abs(got - want) / want) < 1e-6      # (the quad's corners are fp32: it is a plane only up to their rounding)


# ------------------------------------------------------------------------------------------------ the compaction tail
def test_compaction_against_a_literal_restatement():
    v, t, c = S.mesh()
    rng = np.random.default_rng(5)
    for p in (0.0, 0.5, 0.9, 1.0):
        keep = rng.uniform(size=len(v)) < p
        nv, nt, nc = O.compact(v, t, keep, c)
        tt = t[((t >= 0) & (t < len(v))).all(1)]
        tk = tt[keep[tt].all(1)]
        used = np.zeros(len(v), bool)
        used[tk.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        assert np.array_equal(nv, v[used], equal_nan=True) and np.array_equal(nt, remap[tk]) and np.array_equal(nc, c[used])
        assert len(nt) == 0 or (nt.max() == len(nv) - 1 and nt.min() == 0)
    assert len(O.compact(v, t, np.ones(len(v), bool))[1]) == len(t) - 2      # only the two triangles with a bad index go


# ------------------------------------------------------------------------------------------------ readers
def test_readers(tmp_path):
    sys.path.insert(0, PKG)
    import torch
    import surfel_cull as P
    c = S.cameras()
    np.save(str(tmp_path / "a.npy"), c)
    np.save(str(tmp_path / "b.npy"), c[:, :3].astype(np.float64))
    a, b = P.read_trajectory(str(tmp_path / "a.npy")), P.read_trajectory(str(tmp_path / "b.npy"))
    assert a.shape == b.shape == (len(c), 4, 4) and a.dtype == b.dtype == np.float32 and np.array_equal(a, c)
    assert np.array_equal(b[:, :3], c[:, :3]) and np.array_equal(b[:, 3], np.tile([0, 0, 0, 1], (len(c), 1)))
    with pytest.raises(ValueError):
        P.read_trajectory(str(tmp_path / "a.log"))
    np.save(str(tmp_path / "bad.npy"), np.zeros((4, 5, 5)))
    with pytest.raises(ValueError):
        P.read_trajectory(str(tmp_path / "bad.npy"))
    # the exactly-opposite branch, where the reference draws random noise
    with pytest.raises(ValueError, match="opposite"):
        P.rotation_between([0.0, 0.0, -1.0], [0.0, 0.0, 1.0])
    down = np.tile(np.diag([1.0, -1.0, -1.0, 1.0]), (3, 1, 1))      # poses whose up column is (0, -1, 0) turned so that the mean up is -z
    down[:, :3, :3] = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]])
    with pytest.raises(ValueError, match="opposite"):
        P.orient_and_center(down)
    r = P.rotation_between([0.0, 1.0, 0.0], [0.0, 0.0, 1.0])
    assert torch.allclose(r @ torch.tensor([0.0, 1.0, 0.0]), torch.tensor([0.0, 0.0, 1.0]), atol=1e-6)
    # conventions: "opengl" on flipped poses is "opencv" on the poses themselves
    assert torch.equal(P.world_to_camera(S.cameras_opengl(), "opengl"), P.world_to_camera(c, "opencv"))
    assert np.array_equal(P.world_to_camera(c, "opencv").numpy(), O.world_to_camera(c))
    with pytest.raises(ValueError):
        P.world_to_camera(c, "blender")
    # cameras.json
    entry = {"id": 0, "img_name": "x", "width": 67, "height": 45, "position": [1.0, 2.0, 3.0], "rotation": np.eye(3).tolist(), "fx": 60.0, "fy": 61.0}
    (tmp_path / "m").mkdir()
    with open(str(tmp_path / "m" / "cameras.json"), "w") as f:
        json.dump([entry], f)
    (c2w, k, h, w), = P.read_model_cameras(str(tmp_path / "m"))
    assert (h, w, k) == (45, 67, (60.0, 61.0, 33.0, 22.0)) and c2w[:3, 3].tolist() == [1.0, 2.0, 3.0]
    assert (P.EPS, P.MIN_VIEWS, P.ZNEAR, P.ZFAR, P.TNT_H, P.TNT_W) == (0.005, 20, 0.01, 20.0, 1080, 1920)


# ------------------------------------------------------------------------------------------------ library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_cull_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", HEADER)).read(), re.M)
    assert len(decl) == 2
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.CULL_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    others = [name for h, group in surfel_native.SIGNATURES.items() if h != HEADER for name in group]
    assert not set(decl) & set(others)
    lib = surfel_native.load()
    for name in surfel_native.CULL_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_cull", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "mesh_cull.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["mesh_cull.hip"] and any(h.endswith(HEADER) for h in mod.HEADERS)
    import surfel_cull as P
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    assert int(re.search(r"#define SURFEL_CULL_SMALL_PIXELS (\d+)", hdr).group(1)) == P.SMALL_PIXELS == O.SMALL_PIXELS


def test_cull_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_cull.h."""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 2
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES[HEADER])
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is returns[ret], (name, ret, fn.restype)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            else:
                assert ctype.endswith("*"), where
                assert at in (n.DevPtr, n.Stream, C.c_void_p) or issubclass(at, C._Pointer), where
                host = pname in ("stage_ms", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_cull_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("mesh_cull.hip"))
    names = [k for k in ks if "cull_" in k]
    assert len(names) == 4, names
    for k in names:
        md = ks[k][1]
        print("%s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (isa_count.demangle(k).split("(")[0], md.get("next_free_vgpr", 0), md.get("next_free_sgpr", 0),
                                                                   md.get("group_segment_fixed_size", 0), md.get("private_segment_fixed_size", 0)))
        assert int(md.get("private_segment_fixed_size", 0)) == 0, k
        assert md.get("next_free_vgpr", 0) <= 64 and md.get("group_segment_fixed_size", 0) == 0, k


def test_cull_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    sys.path.insert(0, PKG)
    import surfel_cull as P
    from surfel_mesh import TriangleMesh
    p = torch.zeros((8, 3))
    mesh = TriangleMesh(p, torch.zeros((1, 3), dtype=torch.int32), p)
    w2c, k = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), (60.0, 60.0, 33.0, 22.0)
    for call in (lambda: P.mesh_depth(mesh, w2c, k, 45, 67), lambda: P.view_counts(p, torch.zeros((2, 45, 67)), w2c, k),
                 lambda: P.cull_mesh_views(mesh, w2c, k, 45, 67), lambda: P.cull_mesh_cameras(mesh, [(w2c[0], k, 45, 67)])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "tensors must live on a HIP device" in str(e.value)


def test_cull_arguments_are_checked_before_a_device_is_touched():
    import ctypes as C
    import surfel_native as n
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    p = C.c_void_p(256)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # znear = 0
        n.call(None, "surfel_cull_mesh_depth", cb, None, 3, 1, p, p, 1, p, p, 1, 45, 67, 0.0, 20.0, -1, p, None)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # intrinsics for 2 of 3 views
        n.call(None, "surfel_cull_mesh_depth", cb, None, 3, 1, p, p, 3, p, p, 2, 45, 67, 0.01, 20.0, -1, p, None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*SURFEL_CULL_MAX_VIEWS"):
        n.call(None, "surfel_cull_mesh_depth", cb, None, 3, 1, p, p, 65536, p, p, 1, 4, 4, 0.01, 20.0, -1, p, None)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # a one-pixel-wide image has no bilinear sample
        n.call(None, "surfel_cull_visibility", 3, p, 1, p, p, 1, 45, 1, p, 0.005, p)
    assert n.call(None, "surfel_cull_visibility", 0, None, 1, p, p, 1, 45, 67, p, 0.005, None) == 0
    assert not taken
