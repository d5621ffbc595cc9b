"""CPU checks of the mesh smoothing (SMOOTH.md): the numpy restatement (tests/smooth_oracle.py) against counts known in closed form and
against a per-vertex loop that shares nothing with it, the filter's effect on a noisy sphere, the boundary modes, the argument checks
that run before any device is touched, and the library surface (header, exports, signatures, the size limit)."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import simplify_scenes as S
import smooth_oracle as O
import smooth_scenes as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_smooth.h"


@pytest.fixture(scope="module")
def adjacencies():
    return {name: O.adjacency(v, t) for name, (v, t) in M.meshes().items()}


def _degrees(adj):
    return np.diff(adj["offsets"])


# ------------------------------------------------------------------------------------------------ 1: the adjacency's counts
def test_closed_form_counts(adjacencies):
    cube = adjacencies["cube"]
    assert len(cube["offsets"]) == 9603 and cube["stats"]["directed_edges"] == 57600 and bool((cube["multiplicity"] == 2).all())
    assert collections.Counter(_degrees(cube).tolist()) == {4: 6, 6: 9596}
    assert cube["stats"] == dict(kept=19200, dropped=0, directed_edges=57600, border_edges=0, nonmanifold_edges=0, boundary_vertices=0,
                                 isolated_vertices=0, max_degree=6) and not cube["flags"].any()
    sphere = adjacencies["sphere"]
    assert sphere["stats"]["directed_edges"] == 57120 and bool((sphere["multiplicity"] == 2).all()) and not sphere["flags"].any()
    assert sphere["stats"]["max_degree"] == 140 and _degrees(sphere)[0] == _degrees(sphere)[-1] == 140
    plates = adjacencies["plates"]
    assert plates["stats"]["directed_edges"] == 6400 and int((plates["multiplicity"] == 1).sum()) == 512
    assert plates["stats"]["border_edges"] == 256 and plates["stats"]["boundary_vertices"] == 256 == int((plates["flags"] & O.FLAG_BOUNDARY).astype(bool).sum())
    clustered = adjacencies["clustered"]
    v, t = M.clustered_plates()
    assert v.shape == (578, 3) and t.shape == (1536, 3)
    undirected = collections.Counter((clustered["multiplicity"][clustered["neighbors"] > np.repeat(np.arange(578), _degrees(clustered))]).tolist())
    assert undirected == {1: 64, 2: 800, 4: 736} and clustered["stats"]["directed_edges"] == 3200      # the figure of SIMPLIFY.md
    assert clustered["stats"]["border_edges"] == 64 and clustered["stats"]["nonmanifold_edges"] == 736
    special = adjacencies["special"]
    assert special["stats"]["kept"] == 19201 and special["stats"]["dropped"] == 4 and special["stats"]["isolated_vertices"] == 1
    assert special["flags"][-1] == O.FLAG_ISOLATED and special["stats"]["directed_edges"] == 57600 + 2      # the zero-area triangle's long edge
    fan = adjacencies["fan"]
    assert _degrees(fan)[0] == M.FAN_RIM == fan["stats"]["max_degree"] and fan["stats"]["border_edges"] == M.FAN_RIM - 1 + 2
    assert fan["stats"]["boundary_vertices"] == M.FAN_RIM + 1
    umb = adjacencies["umbrellas"]
    assert [int(_degrees(umb)[h]) for h in M.umbrellas()[2]] == list(M.UMBRELLA_DEGREES)
    for name, V in (("no-vertex", 0), ("no-triangle", 300), ("all-dropped", 4)):
        a = adjacencies[name]
        assert a["offsets"].tolist() == [0] * (V + 1) and len(a["neighbors"]) == 0 and a["flags"].tolist() == [O.FLAG_ISOLATED] * V
        assert a["stats"]["isolated_vertices"] == V and a["stats"]["directed_edges"] == a["stats"]["max_degree"] == 0
    assert adjacencies["all-dropped"]["stats"]["dropped"] == 4 and adjacencies["all-dropped"]["stats"]["kept"] == 0


@pytest.mark.parametrize("name", ["clustered", "special", "umbrellas"])
def test_adjacency_equals_a_dictionary_count(adjacencies, name):
    """every kept triangle's three edges counted in a dictionary: the same rows, multiplicities and flags"""
    v, t = M.meshes()[name]
    V = len(v)
    count = collections.Counter()
    for a, b, c in t.tolist():
        if min(a, b, c) < 0 or max(a, b, c) >= V or len({a, b, c}) < 3 or not np.isfinite(v[[a, b, c]]).all():
            continue
        for x, y in ((a, b), (b, c), (c, a)):
            count[(x, y)] += 1
            count[(y, x)] += 1
    adj = adjacencies[name]
    pairs = sorted(count)
    assert [p[1] for p in pairs] == adj["neighbors"].tolist() and [count[p] for p in pairs] == adj["multiplicity"].tolist()
    rows = collections.Counter(p[0] for p in pairs)
    assert [rows[i] for i in range(V)] == _degrees(adj).tolist()
    for i in range(V):
        m = [count[p] for p in pairs if p[0] == i] if V < 700 else None
        if m is not None:
            assert adj["flags"][i] == (O.FLAG_BOUNDARY * (1 in m)) | (O.FLAG_NONMANIFOLD * any(x > 2 for x in m)) | (O.FLAG_ISOLATED * (not m))


# ------------------------------------------------------------------------------------------------ 2: a step
@pytest.mark.parametrize("boundary", O.BOUNDARY)
def test_step_equals_a_per_vertex_loop(adjacencies, boundary):
    """rule 4 written as a loop over the vertices with Python floats (IEEE doubles, one rounding per operation), on the clustered plates
    (border and non-manifold edges) and the closed fans (rows up to 513 entries)"""
    for name in ("clustered", "umbrellas"):
        v, _ = M.meshes()[name]
        adj = adjacencies[name]
        got = O.step(v, O.plan(adj, boundary), -0.53)
        off, nbr, mult, flags = adj["offsets"], adj["neighbors"], adj["multiplicity"], adj["flags"]
        want = v.copy()
        for i in range(len(v)):
            row = list(range(off[i], off[i + 1]))
            on_border = bool(flags[i] & O.FLAG_BOUNDARY)
            if boundary == "curve" and on_border:
                row = [e for e in row if mult[e] == 1]
            if not row or (boundary == "fixed" and on_border):
                continue
            for c in range(3):
                s = 0.0
                for e in row:
                    s += float(v[nbr[e], c])
                x = float(v[i, c])
                want[i, c] = np.float32(x + -0.53 * (s / float(len(row)) - x))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, boundary)
        assert (got != v).any()


def test_taubin_keeps_the_sphere_and_laplacian_shrinks_it(adjacencies):
    v, t, _ = M.noisy_sphere()
    adj = adjacencies["sphere"]
    std0, mean0 = M.radial_stats(v)
    std_t, mean_t = M.radial_stats(O.smooth(v, adj, 10, "taubin"))
    std_l, mean_l = M.radial_stats(O.smooth(v, adj, 10, "laplacian"))
    print("radial std / mean radius: input %.5f %.5f, taubin %.5f %.5f, laplacian %.5f %.5f" % (std0, mean0, std_t, mean_t, std_l, mean_l))
    assert abs(std0 - 0.01005) < 5e-5 and abs(mean0 - 1.00014) < 5e-5
    assert std_t < 0.5 * std0 and abs(mean_t - mean0) < 0.001 and mean0 - mean_l > 0.004
    assert np.array_equal(O.smooth(v, adj, 0).view(np.uint32), v.view(np.uint32))      # N = 0: the input's bits


def test_boundary_modes_on_the_plates(adjacencies):
    v, t = M.noisy_plates()
    adj = adjacencies["plates"]
    on_border = (adj["flags"] & O.FLAG_BOUNDARY).astype(bool)
    free, fixed, curve = (O.smooth(v, adj, 3, "taubin", boundary=b) for b in O.BOUNDARY)
    assert np.array_equal(fixed[on_border].view(np.uint32), v[on_border].view(np.uint32)) and (fixed[~on_border] != v[~on_border]).any()
    assert (free[on_border] != v[on_border]).any() and (curve[on_border] != free[on_border]).any()
    # one step: a plate's straight border stays in its line under `curve` (its neighbours along the border share its x), not under `free`
    left = on_border & (v[:, 0] == 0.0) & (v[:, 1] > 0.0) & (v[:, 1] < 1.0)
    curve1, free1 = (O.smooth(v, adj, 1, "laplacian", boundary=b) for b in ("curve", "free"))
    assert left.sum() == 4 * 15 and np.array_equal(curve1[left, 0], v[left, 0]) and (free1[left, 0] > 0).all()
    assert (curve1[left, 2] != v[left, 2]).any()
    # the NaN vertex of the special cube passes through with its payload, and pulls nobody
    sv, st = S.special_cube()
    sv = sv.copy()
    sv.view(np.uint32)[-1, 0] = 0x7FC12345
    out = O.smooth(sv, O.adjacency(sv, st), 2, "laplacian")
    assert out.view(np.uint32)[-1].tolist() == sv.view(np.uint32)[-1].tolist() and np.isfinite(out[:-1]).all()


# ------------------------------------------------------------------------------------------------ 3: arguments, before any device
def test_bad_arguments_raise_value_errors_without_a_device():
    sys.path.insert(0, PKG)
    import torch
    import surfel_smooth as P
    from surfel_mesh import TriangleMesh
    mesh = TriangleMesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), None)      # host tensors: a device would be refused later
    bad = [dict(lam=0.0), dict(lam=1.5), dict(lam=float("nan")), dict(mu=-0.5), dict(mu=0.3), dict(mu=float("nan")), dict(mu=-0.4, lam=0.4),
           dict(iterations=-1), dict(iterations=1.5), dict(method="cotangent"), dict(boundary="pinned"), dict(colors=True)]
    for kw in bad:
        with pytest.raises(ValueError, match="surfel_smooth"):
            P.smooth_mesh(mesh, **kw)
        if "colors" not in kw:
            with pytest.raises(ValueError):
                O.factors(**dict(dict(iterations=1), **kw))
    with pytest.raises(RuntimeError, match="HIP device"):      # good arguments reach the device check
        P.smooth_mesh(mesh, lam=1.0, mu=-1.01)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.smooth_mesh(mesh, method="laplacian", mu=5.0, iterations=0)      # (mu is taubin's)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.mesh_adjacency(mesh)
    assert P.check_arguments(2, "taubin", 0.5, -0.53, "free") == [0.5, -0.53, 0.5, -0.53] == O.factors(2)
    assert P.check_arguments(3, "laplacian", 0.25, 0.0, "curve") == [0.25] * 3 and P.check_arguments(0, "taubin", 0.5, -0.53, "fixed") == []
    assert P.METHODS == O.METHODS and P.BOUNDARY == O.BOUNDARY and P.COUNTS == O.COUNTS
    assert (P.FLAG_BOUNDARY, P.FLAG_NONMANIFOLD, P.FLAG_ISOLATED) == (O.FLAG_BOUNDARY, O.FLAG_NONMANIFOLD, O.FLAG_ISOLATED)
    import surfel_mesh
    args = surfel_mesh.build_parser().parse_args(["-m", "x"])      # without the flags the mesh CLI smooths nothing
    assert args.smooth_iterations is None and args.smooth_method == "taubin" and args.smooth_boundary == "free"
    with pytest.raises(SystemExit, match="smooth_iterations"):
        surfel_mesh.main(["-m", "x", "--smooth_iterations", "-2"])
    with pytest.raises(SystemExit):
        P.main(["--ply-path", "x.ply", "--method", "cotangent"])
    with pytest.raises(ValueError, match="lam"):
        P.main(["--ply-path", "x.ply", "--lam", "0"])      # (before the file is opened)


# ------------------------------------------------------------------------------------------------ 4: the library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_smooth_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", hdr, re.M)
    assert decl == ["surfel_smooth_adjacency", "surfel_smooth_steps"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.SMOOTH_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    others = [name for h, group in surfel_native.SIGNATURES.items() if h != HEADER for name in group]
    assert not set(decl) & set(others)
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_smooth", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "mesh_smooth.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["mesh_smooth.hip"] and any(h.endswith(HEADER) for h in mod.HEADERS)
    import surfel_smooth as P
    assert int(re.search(r"#define SURFEL_SMOOTH_COUNTS (\d+)", hdr).group(1)) == len(P.COUNTS)
    for k, name in enumerate(("FREE", "FIXED", "CURVE")):
        assert int(re.search(r"#define SURFEL_SMOOTH_%s (\d+)" % name, hdr).group(1)) == k == P.BOUNDARY.index(name.lower())
    for name, bit in (("BOUNDARY", P.FLAG_BOUNDARY), ("NONMANIFOLD", P.FLAG_NONMANIFOLD), ("ISOLATED", P.FLAG_ISOLATED)):
        assert int(re.search(r"#define SURFEL_SMOOTH_%s (\d+)" % name, hdr).group(1)) == bit


def test_smooth_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_smooth.h."""
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
                host = pname in ("counts", "factors", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_the_size_limit_is_refused_before_any_device_call():
    """V = 2^31, or six times F = 2^31 and more: SURFEL_E_LIMIT with no allocation and no count written (the entries compare the sizes
    before their first device call, so no device is needed); the pointers are never followed"""
    import ctypes as C
    import surfel_native as n
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    counts = (C.c_int64 * 8)(*([-7] * 8))
    fake = C.c_void_p(256)
    f_max = (2 ** 31 - 1) // 6
    for V, F in ((2 ** 31, 10), (10, f_max + 1), (2 ** 40, 2 ** 40)):
        with pytest.raises(n.LimitError, match=r"surfel_smooth_adjacency failed \(-4\): .*2\^31"):
            n.call(None, "surfel_smooth_adjacency", cb, None, V, F, fake, fake, fake, fake, fake, fake, counts)
    assert 6 * f_max < 2 ** 31 <= 6 * (f_max + 1)
    with pytest.raises(n.LimitError, match=r"surfel_smooth_steps failed \(-4\): .*2\^31"):
        n.call(None, "surfel_smooth_steps", 2 ** 31, fake, fake, fake, fake, 0, 1, (C.c_double * 1)(0.5), fake, fake, fake)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
        n.call(None, "surfel_smooth_steps", 10, fake, fake, fake, fake, 3, 1, (C.c_double * 1)(0.5), fake, fake, fake)      # no such mode
    with pytest.raises(RuntimeError, match=r"\(-1\): .*not finite"):
        n.call(None, "surfel_smooth_steps", 10, fake, fake, fake, fake, 0, 1, (C.c_double * 1)(float("inf")), fake, fake, fake)
    assert not taken and list(counts) == [-7] * 8
