"""CPU checks of the mesh viewer (MESHVIEW.md): the conditions the scene has to meet so that the caps of the GPU tests cannot hide a
failure, the float32 restatement of the shading against the float64 oracle, the vertex-normal sums, the supersampling grid, and the
library surface (header, exports, signatures, kernel resources, command lines, the viewer's menu)."""
import json
import os
import re
import socket
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import cull_oracle as O
import cull_scenes as S
import meshview_oracle as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_meshview.h"
ZN, ZF = S.SCENE["znear"], S.SCENE["zfar"]
# The restatement against the float64 oracle on decided pixels: the largest deviation measured on this scene is 1 level (below), and any
# reordering of the same float32 operations can flip one quantisation step more.
BAR_LEVELS = 1 + 1
# (size, ssaa, views): all views with one sample per pixel; with four samples, views in which both classes and the filler are live
CASES = (("small", 1, None), ("large", 1, None), ("small", 2, (0, 11, 23)), ("large", 2, (5, 23)))


# ------------------------------------------------------------------------------------------------ 1: the oracle alone
@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_scene_conditions(size):
    """At most 0.5 % undecided pixels per image with the close-pair rule added; coverage and class counts are those of CULL.md §Pinning."""
    r = M.scene_reference(size)
    share = r["pixel_und"].mean((1, 2))
    w = int(share.argmax())
    print("%s: worst image %d: %d undecided pixels = %.4f %%; over all views %d by close pairs, %d by cull_oracle's own rules" %
          (size, w, r["pixel_und"][w].sum(), 100 * share[w], r["close"].sum(), r["own"].sum()))
    assert share.max() <= M.CAP
    assert r["close"].sum() > 0 and r["own"].sum() > 0
    cover = (r["tri64"] >= 0).mean((1, 2))
    n = S.SCENE["views"]
    assert ((cover[:n - 1] > 0.25) & (cover[:n - 1] < 0.75)).all() and cover[n - 1] == 1.0 and cover[n] == 0.0
    assert np.array_equal(r["tri64"] >= 0, O.scene_reference(size)["d64"] > 0)
    small, large = O.size_classes(r["verts"], r["tris"], r["w2c"], r["intr"], r["H"], r["W"], ZN, ZF)
    assert (small, large) == {"small": (41240, 2034), "large": (37074, 6200)}[size]
    # more than one triangle wins pixels in every ordinary view, and the special triangles of the arc's last camera both do
    assert all(len(np.unique(r["tri64"][i])) > 50 for i in range(n - 1))
    first = len(r["tris"]) - 8
    assert set(np.unique(r["tri64"][n - 1])) == {first, first + 1}


def test_keys_pack_and_unpack():
    r = M.scene_reference("small")
    key = M.pack(r["depth32"], r["tri32"])
    d, t = M.unpack(key)
    assert np.array_equal(d, r["depth32"]) and np.array_equal(t, r["tri32"]) and key.dtype == np.uint64
    assert (key[r["tri32"] < 0] == M.EMPTY).all() and int(M.EMPTY) == 0x7f800000ffffffff
    # the integer order of the keys is (depth, then index)
    a, b, c = M.pack(np.float32([1.0, 1.0, 1.5]), np.array([7, 3, 0]))
    assert b < a < c < M.EMPTY
    d2, t2 = M.unpack(key.view(np.int64))      # (the device tensor is int64)
    assert np.array_equal(d2, d) and np.array_equal(t2, t)


# ------------------------------------------------------------------------------------------------ 2: restatement against the fp64 oracle
@pytest.mark.parametrize("size,ssaa,views", CASES)
def test_restatement_matches_the_fp64_oracle(size, ssaa, views):
    """Per mode, smooth and flat: on decided pixels the float32 restatement (on the float32 twin's keys) is within BAR_LEVELS of the float64
    oracle (on the float64 twin's nearest triangles).  Measured on this scene: the largest deviation is 1 level, on at most 0.012 % of the
    decided pixels of a case, and no pixel deviates by more.  Pixels above the bar count under the 0.5 % cap with the undecided ones."""
    r = M.scene_reference(size, ssaa, views)
    H, W = r["H"], r["W"]
    assert r["pixel_und"].mean((1, 2)).max() <= M.CAP
    for mode in ("shaded", "normal", "color"):
        for smooth in (True, False):
            hist = np.zeros(256, np.int64)
            for i in range(len(r["views"])):
                k32 = M.pack(r["depth32"][i], r["tri32"][i])
                k64 = M.pack(np.where(r["tri64"][i] >= 0, 1.0, 0.0), r["tri64"][i])
                a = M.shade(k32, r["verts"], r["tris"], r["colors"], r["normals32"] if smooth else None, r["w2c"][i], r["sample_intr"], H, W, ssaa, mode)[0]
                b = M.shade(k64, r["verts"], r["tris"], r["colors"], r["normals64"] if smooth else None, r["w2c"][i], r["sample_intr"], H, W, ssaa, mode,
                            T=np.float64)[0]
                assert a.shape == b.shape == (H, W, 3) and a.dtype == b.dtype == np.uint8
                dev = np.abs(a.astype(int) - b.astype(int)).max(-1)
                ok = ~r["pixel_und"][i]
                hist += np.bincount(dev[ok], minlength=256)
                over = (dev > BAR_LEVELS) & ok
                assert (over | r["pixel_und"][i]).mean() <= M.CAP, (mode, smooth, i, int(over.sum()))
                if i == 0:
                    assert (a[r["tri32"][i].reshape(H, ssaa, W, ssaa).max((1, 3)) < 0] == 255).all()      # nothing hit: the background
            top = int(np.nonzero(hist)[0].max())
            print("%s x%d %s %s: largest deviation %d level(s); %.4f %% of %d decided pixels at 1 level, %.4f %% above" %
                  (size, ssaa, mode, "smooth" if smooth else "flat", top, 100 * hist[1] / hist.sum(), hist.sum(), 100 * hist[2:].sum() / hist.sum()))
            assert top <= BAR_LEVELS - 1, "the measured maximum behind BAR_LEVELS no longer holds: measure again and restate it"


def test_modes_are_distinct_and_grey_ignores_colours():
    r = M.scene_reference("small")
    i = 7
    key = M.pack(r["depth32"][i], r["tri32"][i])
    args = (r["w2c"][i], r["sample_intr"], r["H"], r["W"], 1)
    frames = {m: M.shade(key, r["verts"], r["tris"], r["colors"], r["normals32"], *args, m)[0] for m in M.MODES}
    assert not np.array_equal(frames["shaded"], frames["color"]) and not np.array_equal(frames["normal"], frames["color"])
    grey = M.shade(key, r["verts"], r["tris"], None, r["normals32"], *args, "color")[0]
    hit = r["tri32"][i] >= 0
    assert (grey[hit] == int(np.float32(0.8) * np.float32(255))).all() and (grey[~hit] == 255).all()
    flat = M.shade(key, r["verts"], r["tris"], r["colors"], None, *args, "normal")[0]
    assert not np.array_equal(flat, frames["normal"])
    # the normal frame faces the camera: n_cam . ray <= 0 wherever something is hit
    n_world = (M.shade(key, r["verts"], r["tris"], r["colors"], None, *args, "normal")[1] - 0.5) / 0.5
    n_cam = n_world @ r["w2c"][i][:3, :3].T
    fx, fy, cx, cy = r["sample_intr"]
    xs, ys = np.meshgrid(np.arange(r["W"]), np.arange(r["H"]))
    ray = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs, float)], -1)
    assert ((n_cam * ray).sum(-1)[hit] <= 1e-5).all() and np.allclose(np.linalg.norm(n_world[hit], axis=-1), 1, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 3: vertex normals
def _fan(valence=5000):
    """a cone of `valence` triangles around vertex 0, the rim bumpy so that the face normals differ"""
    a = 2 * np.pi * np.arange(valence) / valence
    rim = np.stack([np.cos(a), np.sin(a), 0.3 + 0.05 * np.sin(7 * a)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(np.float32)
    k = np.arange(valence)
    return v, np.stack([np.zeros(valence, int), 1 + k, 1 + (k + 1) % valence], 1).astype(np.int32)


def _normal_case(v, t):
    acc = M.normal_sums(v, t)
    # the same sums in plain Python integers, triangle after triangle
    tt, q = M.face_quanta(v, t)
    want = [[0, 0, 0] for _ in range(len(v))]
    for tri, qq in zip(tt.tolist(), q.tolist()):
        for i in tri:
            for k in range(3):
                want[i][k] += qq[k]
    assert acc.dtype == np.int64 and acc.tolist() == want
    n32, n64 = M.normals_from_sums(acc), M.vertex_normals64(v, t)
    # The bound.  A face's quantum is off by at most 0.5 per component from rounding and by 2^20 times the float32 error of its unit
    # normal: the differences p1 - p0 and the products round to 2^-24 relative each, which the cancellation of the cross product
    # amplifies by |a| |b| / |fn| = 1 / sin(angle); 8 such roundings cover the cross product, the length and the division.  A vertex's
    # sum S of k faces is therefore off by at most sum(eps_f); normalising moves a unit vector by at most twice the relative error of S,
    # and the float32 conversion, length and division add 4 x 2^-24.
    v64 = v.astype(np.float64)
    ok = ((t >= 0) & (t < len(v))).all(1)
    a, b = v64[t[ok][:, 1]] - v64[t[ok][:, 0]], v64[t[ok][:, 2]] - v64[t[ok][:, 0]]
    with np.errstate(all="ignore"):
        sin = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        eps_f = np.sqrt(3) * (0.5 / M.SCALE + 8 * 2.0 ** -24 / sin)
    eps_f = np.where(np.isfinite(eps_f), eps_f, 2.0)      # (a face one side skips and the other keeps moves the sum by at most a unit vector)
    err_sum = np.zeros(len(v))
    for k in range(3):
        np.add.at(err_sum, t[ok][:, k], eps_f)
    u = np.zeros((len(v), 3))
    tu, uu = M._unit_face_normals(v, t, np.float64)
    for k in range(3):
        np.add.at(u, tu[:, k], uu)
    length = np.linalg.norm(u, axis=1)
    with np.errstate(all="ignore"):
        bound = 2 * err_sum / length + 4 * 2.0 ** -24
    live = length > 1e-3
    err = np.abs(n32.astype(np.float64) - n64).max(1)
    assert (err[live] <= bound[live]).all(), float((err[live] - bound[live]).max())
    return acc, n32, err[live].max(), np.median(bound[live])


def test_vertex_normal_sums_and_bound():
    v, t, _ = S.mesh()
    acc, n32, err, med = _normal_case(v, t)
    print("scene: largest deviation of the fixed-point normals from float64 averaging %.3g (median bound %.3g)" % (err, med))
    assert med < 2e-5 and err < 1e-4      # (the bound is not vacuous where it matters)
    assert np.isfinite(n32).all() and (acc[-1] == 0).all() and (n32[-1] == 0).all()      # the NaN vertex: nothing adds up, (0, 0, 0)
    used = np.zeros(len(v), bool)
    used[M.face_quanta(v, t)[0].reshape(-1)] = True
    assert np.allclose(np.linalg.norm(n32[used], axis=1), 1, atol=1e-6)
    # a fan: valence 5 000, the sum of one component passes 2^32
    fv, ft = _fan()
    acc, n32, err, med = _normal_case(fv, ft)
    print("fan: |sum| at the hub %s, deviation %.3g (median bound %.3g)" % (acc[0].tolist(), err, med))
    assert int(acc[0, 2]) > 1 << 32 and n32[0, 2] > 0.99
    # order-free: a permutation of the triangles gives the same sums
    p = np.random.default_rng(1).permutation(len(ft))
    assert np.array_equal(M.normal_sums(fv, ft[p]), acc)


# ------------------------------------------------------------------------------------------------ 4: the supersampling grid
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_scaled_intrinsics_sample_the_stated_positions(s):
    """sample s x + k of the sample grid looks along the ray of the pixel coordinate x + (k + 0.5) / s - 0.5, exactly"""
    sys.path.insert(0, PKG)
    import surfel_meshview as P
    for size in sorted(S.SIZES):
        k = S.intrinsics(size)
        got = P.scaled_intrinsics(k, s)
        assert got.shape == (1, 4) and got.dtype == np.float64
        assert np.array_equal(got.astype(np.float32), M.scaled_intrinsics(k, s))
        fx, fy, cx, cy = (Fraction(float(x)) for x in k)
        fxs, fys, cxs, cys = (Fraction(float(x)) for x in got[0])
        for x in (0, 1, 17, S.SIZES[size][1] - 1):
            for j in range(s):
                pos = Fraction(x) + (Fraction(j) + Fraction(1, 2)) / s - Fraction(1, 2)
                assert abs((Fraction(s * x + j) - cxs) / fxs - (pos - cx) / fx) < Fraction(1, 10 ** 12)
                assert abs((Fraction(s * x + j) - cys) / fys - (pos - cy) / fy) < Fraction(1, 10 ** 12)
    assert np.array_equal(P.scaled_intrinsics(S.intrinsics("small"), 1)[0], np.asarray(S.intrinsics("small"), np.float64))


# ------------------------------------------------------------------------------------------------ 5, 6: the library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_meshview_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("mesh_view.hip"))
    names = [k for k in ks if "meshview_" in k or "cull_" in k]
    assert len(names) == 6, names      # clear, face normals, vertex normals, shade, and the two class kernels with the 64-bit key
    for k in names:
        md = ks[k][1]
        print("%s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (isa_count.demangle(k).split("(")[0], md.get("next_free_vgpr", 0), md.get("next_free_sgpr", 0),
                                                                   md.get("group_segment_fixed_size", 0), md.get("private_segment_fixed_size", 0)))
        assert int(md.get("private_segment_fixed_size", 0)) == 0, k
        assert md.get("next_free_vgpr", 0) <= 128 and md.get("group_segment_fixed_size", 0) == 0, k


def test_meshview_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", hdr, re.M)
    assert len(decl) == 3
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.MESHVIEW_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    others = [name for h, group in surfel_native.SIGNATURES.items() if h != HEADER for name in group]
    assert not set(decl) & set(others)
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_meshview", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "mesh_view.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["mesh_view.hip"] and "-ffp-contract=off" in mod.EXTRA["mesh_cull.hip"]
    assert any(h.endswith(HEADER) for h in mod.HEADERS) and "mesh_raster.h" in mod.HEADERS
    import surfel_meshview as P
    assert int(re.search(r"#define SURFEL_MESHVIEW_EMPTY (0x[0-9a-f]+)ull", hdr).group(1), 16) == P.EMPTY_KEY == int(M.EMPTY)
    assert int(re.search(r"#define SURFEL_MESHVIEW_NORMAL_SCALE (\d+)", hdr).group(1)) == P.NORMAL_SCALE == M.SCALE
    assert int(re.search(r"#define SURFEL_MESHVIEW_MAX_SSAA (\d+)", hdr).group(1)) == P.MAX_SSAA
    for name, value in P._KERNEL_MODE.items():
        assert int(re.search(r"#define SURFEL_MESHVIEW_%s (\d+)" % name.upper(), hdr).group(1)) == value == M.MODES[name]
    # one set-up and one pixel test: both files take them from the shared header
    for src in ("mesh_cull.hip", "mesh_view.hip"):
        text = open(os.path.join(PKG, "csrc", src)).read()
        assert '#include "mesh_raster.h"' in text and "cull_setup(" not in text.replace("cull_setup(t0", "") and "bool cull_setup" not in text
    assert open(os.path.join(PKG, "csrc", "mesh_raster.h")).read().count("bool cull_setup(") == 1


def test_meshview_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_meshview.h."""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 3
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
                host = pname in ("stage_ms", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_meshview_arguments_are_checked_before_a_device_is_touched():
    import ctypes as C
    import surfel_native as n
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    p = C.c_void_p(256)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):      # znear = 0
        n.call(None, "surfel_meshview_visibility", cb, None, 3, 1, p, p, 1, p, p, 1, 45, 67, 0.0, 20.0, -1, p, None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*do not fit the key"):
        n.call(None, "surfel_meshview_visibility", cb, None, 3, (1 << 32) - 1, p, p, 1, p, p, 1, 45, 67, 0.01, 20.0, -1, p, None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*SURFEL_CULL_MAX_VIEWS"):
        n.call(None, "surfel_meshview_visibility", cb, None, 3, 1, p, p, 65536, p, p, 1, 4, 4, 0.01, 20.0, -1, p, None)
    for ssaa, mode in ((0, 0), (5, 0), (1, 3), (1, -1)):
        with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
            n.call(None, "surfel_meshview_shade", 3, 1, p, p, None, None, 1, p, p, 1, 45, 67, ssaa, p, mode, 1.0, 1.0, 1.0, p)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
        n.call(None, "surfel_meshview_vertex_normals", 3, 1, p, p, None, p)
    assert n.call(None, "surfel_meshview_vertex_normals", 0, 0, None, None, None, None) == 0
    assert n.call(None, "surfel_meshview_shade", 3, 1, p, p, None, None, 0, None, None, 1, 45, 67, 2, None, 0, 1.0, 1.0, 1.0, None) == 0
    assert not taken


def test_meshview_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    sys.path.insert(0, PKG)
    import surfel_meshview as P
    from surfel_mesh import TriangleMesh
    p = torch.zeros((8, 3))
    mesh = TriangleMesh(p, torch.zeros((1, 3), dtype=torch.int32), p)
    w2c, k = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), (60.0, 60.0, 33.0, 22.0)
    for call in (lambda: P.visibility(mesh, w2c, k, 45, 67), lambda: P.vertex_normals(mesh), lambda: P.unpack(torch.zeros((1, 4, 4), dtype=torch.int64)),
                 lambda: P.render_mesh(mesh, (w2c, k, 45, 67)), lambda: P.shade(mesh, torch.zeros((2, 45, 67), dtype=torch.int64), w2c, k, 45, 67)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "tensors must live on a HIP device" in str(e.value)
    with pytest.raises(ValueError):
        P.render_mesh(mesh, (w2c, k, 45, 67), mode="wireframe")


# ------------------------------------------------------------------------------------------------ 7: command lines and the viewer's menu
def test_command_lines_parse():
    sys.path.insert(0, PKG)
    import surfel_mesh
    import surfel_meshview as P
    import surfel_view as SV
    a = P.build_parser().parse_args(["--ply-path", "m.ply", "-m", "model", "--views", "train", "--mesh_modes", "shaded", "depth", "--mesh_ssaa", "3"])
    assert (a.ply_path, a.model_path, a.views, a.mesh_modes, a.mesh_ssaa, a.traj_path) == ("m.ply", "model", "train", ["shaded", "depth"], 3, None)
    a = P.build_parser().parse_args(["--ply-path", "m.ply", "--traj-path", "t.npy"])
    assert (a.views, a.mesh_modes, a.mesh_ssaa, a.video, a.video_only) == ("path", ["shaded", "normal"], 2, False, False)
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(["--ply-path", "m.ply", "-m", "x", "--mesh_modes", "wireframe"])
    with pytest.raises(SystemExit):
        P.main(["--ply-path", "m.ply"])      # neither -m nor --traj-path (refused before the mesh is read)
    a = surfel_mesh.build_parser().parse_args(["-m", "model", "--render_path", "--render_mesh", "--mesh_modes", "shaded", "normal", "color", "depth",
                                               "--mesh_ssaa", "2", "--skip_mesh"])
    assert a.render_mesh and a.mesh_modes == ["shaded", "normal", "color", "depth"] and a.mesh_ssaa == 2
    a = surfel_mesh.build_parser().parse_args(["-m", "model"])
    assert not a.render_mesh and a.mesh_modes == ["shaded", "normal"] and a.mesh_ssaa == 2
    assert SV.build_parser().parse_args(["-m", "model"]).mesh is None
    assert SV.build_parser().parse_args(["-m", "model", "--mesh", "m.ply"]).mesh == "m.ply"
    assert P.MODES == ("shaded", "normal", "color", "depth")


def _items_sent(**kw):
    sys.path.insert(0, PKG)
    import surfel_view as SV
    a, b = socket.socketpair()
    try:
        b.settimeout(5.0)
        v = SV.Viewer.attached(a, **kw)
        n = int.from_bytes(b.recv(4), "little")
        body = b""
        while len(body) < n:
            body += b.recv(n - len(body))
        return v, n.to_bytes(4, "little") + body
    finally:
        a.close()
        b.close()


def test_the_menu_without_a_mesh_is_unchanged():
    import surfel_view as SV
    want = json.dumps(["RGB", "Alpha", "Normal", "Depth", "Edge", "Curvature"]).encode("utf-8")
    v, sent = _items_sent()
    assert SV.RENDER_ITEMS == ["RGB", "Alpha", "Normal", "Depth", "Edge", "Curvature"] and v.items == SV.RENDER_ITEMS
    assert sent == len(want).to_bytes(4, "little") + want
    assert all(v._mesh_mode(m) is None for m in (0, 5, 6, 7, "Mesh", "RGB"))
    v, sent = _items_sent(mesh=object())
    assert v.items == SV.RENDER_ITEMS + ["Mesh", "Mesh Normal"] and json.loads(sent[4:].decode()) == v.items
    assert [v._mesh_mode(m) for m in (0, 5, 6, 7, 8, "mesh", "Mesh Normal", "RGB")] == [None, None, "shaded", "normal", None, "shaded", "normal", None]
    assert SV.RENDER_ITEMS == ["RGB", "Alpha", "Normal", "Depth", "Edge", "Curvature"]      # (the module's list is not appended to)
