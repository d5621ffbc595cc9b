"""CPU checks of the mesh repair (REPAIR.md): the numpy restatement (tests/repair_oracle.py) against properties that share nothing with
its formulation — a plain Python edge count, a union-find over every vertex's triangles, the border count, the provenance of every
triangle, Euler's formula on the filled sphere, the closed cube bit for bit — on every fixture and cap; then the argument checks that
run before any device is touched and the library surface (header, exports, signatures, the size limit)."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import repair_oracle as O
import repair_scenes as R
import simplify_scenes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_repair.h"
CASES = R.cases()
RUNS = [(name, cap) for name in sorted(CASES) for cap in CASES[name][3]]
_OUT = {}


def result(name, cap):
    """the restatement's result of a fixture under a cap, computed once and never written"""
    if (name, cap) not in _OUT:
        v, t, c, _ = CASES[name]
        _OUT[name, cap] = O.repair(v, t, c, cap)
    return _OUT[name, cap]


def _edge_count(tris):
    """directed edge -> the number of triangles that have it, by a plain loop"""
    count = collections.Counter()
    for a, b, c in tris.tolist():
        count[a, b] += 1
        count[b, c] += 1
        count[c, a] += 1
    return count


def _fans(tris):
    """vertex -> the number of components of its incident triangles, two of them joined when they share an edge at that vertex"""
    parent = list(range(len(tris)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    at = collections.defaultdict(list)      # (vertex, other end of an edge at it) -> triangles
    for i, (a, b, c) in enumerate(tris.tolist()):
        for u, p, q in ((a, b, c), (b, c, a), (c, a, b)):
            at[u, p].append(i)
            at[u, q].append(i)
    touching = collections.defaultdict(list)
    for (u, _), ts in at.items():
        touching[u].append(ts)
    out = {}
    for u, groups in touching.items():
        # a union-find of this vertex's own: the same two triangles may share an edge at u and lie in different fans of another vertex
        mine = sorted({i for g in groups for i in g})
        for i in mine:
            parent[i] = i
        for g in groups:
            for i in g[1:]:
                parent[find(i)] = find(g[0])
        out[u] = len({find(i) for i in mine})
    return out


@pytest.mark.parametrize("name,cap", RUNS)
def test_output_is_manifold_with_one_fan_per_vertex(name, cap):
    out = result(name, cap)
    tris = out["triangles"]
    assert tris.dtype == np.int32 and out["vertices"].dtype == np.float32
    assert len(out["vertices"]) == len(out["vertex_source"]) and len(tris) == len(out["triangle_source"])
    if len(tris):
        assert tris.min() >= 0 and tris.max() < len(out["vertices"])
    count = _edge_count(tris)
    assert all(n == 1 for n in count.values())                                   # no directed edge twice: two triangles are opposite
    border = sum(1 for (a, b) in count if (b, a) not in count)
    stats = out["stats"]
    lengths = out["loop_lengths"]
    assert border == stats["border_edges_after"] == int(lengths[lengths > cap].sum())
    assert stats["border_edges"] == int(lengths.sum()) and stats["loops"] == len(lengths) and (lengths >= 3).all()
    assert stats["longest_loop"] == (int(lengths.max()) if len(lengths) else 0)
    assert stats["filled_loops"] == int((lengths <= cap).sum())
    assert stats["label_rounds"] <= int(np.ceil(np.log2(max(stats["longest_loop"], 2)))) + 1
    fans = _fans(tris)
    assert all(n == 1 for n in fans.values()), [u for u, n in fans.items() if n != 1][:5]
    assert list(out["stats"]) == list(O.COUNTS)


@pytest.mark.parametrize("name,cap", RUNS)
def test_every_triangle_is_an_input_triangle_or_fills_its_loop(name, cap):
    v, t, c, _ = CASES[name]
    out = result(name, cap)
    tris, tsrc, vsrc, stats = out["triangles"].astype(np.int64), out["triangle_source"], out["vertex_source"], out["stats"]
    V = len(v)
    S_, C_ = stats["split_vertices"], stats["fill_vertices"]
    assert len(vsrc) == V + S_ + C_ and np.array_equal(vsrc[:V], np.arange(V)) and (vsrc[V + S_:] == -1).all()
    assert ((vsrc[V:V + S_] >= 0) & (vsrc[V:V + S_] < V)).all()
    old = tsrc >= 0
    Fs = int(old.sum())
    assert old[:Fs].all() and Fs == stats["kept"] - stats["cut_triangles"] and (np.diff(tsrc[:Fs]) > 0).all()      # survivors first, in order
    assert np.array_equal(vsrc[tris[:Fs]], np.asarray(t, np.int64)[tsrc[:Fs]])
    assert len(tris) - Fs == stats["fill_triangles"]
    bits, obits = np.asarray(v, np.float32).view(np.uint32), out["vertices"].view(np.uint32)
    assert np.array_equal(obits[:V], bits) and np.array_equal(obits[V:V + S_], bits[vsrc[V:V + S_]])
    if c is not None:
        cb, ob = np.asarray(c, np.float32).view(np.uint32), out["colors"].view(np.uint32)
        assert np.array_equal(ob[:V], cb) and np.array_equal(ob[V:V + S_], cb[vsrc[V:V + S_]])
    else:
        assert out["colors"] is None
    # fill triangles: loop by loop in loop order, each loop's triangles name it; a fan's apex is a centroid, the mean of its rim
    loops = -1 - tsrc[Fs:]
    assert (np.diff(loops) >= 0).all() and set(loops.tolist()) == set(np.nonzero(out["loop_lengths"] <= cap)[0].tolist())
    for l in sorted(set(loops.tolist())):
        mine = tris[Fs:][loops == l]
        L = int(out["loop_lengths"][l])
        assert len(mine) == (1 if L == 3 else L)
        if L > 3:
            apex = mine[:, 2]
            assert (apex == apex[0]).all() and vsrc[apex[0]] == -1 and (vsrc[mine[:, :2]] >= 0).all()
            rim = out["vertices"][mine[:, 1]].astype(np.float64)
            assert np.allclose(out["vertices"][apex[0]], rim.mean(0), rtol=0, atol=1e-6 * (1 + np.abs(rim).max()))
            assert sorted(mine[:, 0].tolist()) == sorted(mine[:, 1].tolist())      # the rim is closed
        else:
            assert (vsrc[mine] >= 0).all()


def test_filled_sphere_is_a_sphere():
    for name, cap in (("punched", 200), ("relabelled", 200)):
        out = result(name, cap)
        tris = out["triangles"]
        assert out["stats"]["border_edges_after"] == 0 and out["stats"]["filled_loops"] == out["stats"]["loops"] == 5
        edges = {(min(a, b), max(a, b)) for t in tris.tolist() for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
        assert len(np.unique(tris)) - len(edges) + len(tris) == 2
        assert sorted(out["loop_lengths"].tolist()) == R.punched_sphere()[3]
        assert out["stats"]["split_vertices"] == 1 and out["stats"]["cut_triangles"] == 0
        assert out["stats"]["fill_vertices"] == 4 and out["stats"]["fill_triangles"] == 1 + 4 + 6 + 6 + 140
    # the cap on both sides of the loop of four; ids that do not follow the geometry give the same loops
    assert result("punched", 3)["stats"]["filled_loops"] == 1 and result("punched", 4)["stats"]["filled_loops"] == 2
    assert result("punched", 0)["stats"]["filled_loops"] == 0 and result("punched", 32)["stats"]["filled_loops"] == 4
    assert result("relabelled", 5)["stats"]["filled_loops"] == 2 and result("relabelled", 6)["stats"]["filled_loops"] == 4


def test_closed_cube_comes_back_bit_for_bit():
    v, t = S.cube()
    out = result("cube", 32)
    assert np.array_equal(out["vertices"].view(np.uint32), v.view(np.uint32)) and np.array_equal(out["triangles"], t)
    assert np.array_equal(out["triangle_source"], np.arange(len(t))) and np.array_equal(out["vertex_source"], np.arange(len(v)))
    assert out["stats"] == dict(dict.fromkeys(O.COUNTS, 0), kept=len(t))
    special = result("special", 32)      # rule 1 drops four; the zero-area triangle puts a third triangle on two edges of the cube
    assert special["stats"]["kept"] == 19201 and special["stats"]["dropped"] == 4 and special["stats"]["nonmanifold_edges"] == 2


def test_known_counts():
    pillow = result("one-triangle", 3)
    assert pillow["triangles"].tolist() == [[0, 1, 2], [0, 2, 1]] and pillow["triangle_source"].tolist() == [0, -1]
    assert pillow["stats"]["border_edges_after"] == 0 and result("one-triangle", 0)["stats"]["border_edges_after"] == 3
    for name, V in (("no-vertex", 0), ("no-triangle", 300), ("all-dropped", 4)):
        out = result(name, 32)
        assert out["triangles"].shape == (0, 3) and out["vertices"].shape == (V, 3) and out["stats"]["kept"] == 0 and out["stats"]["loops"] == 0
    flipped = result("flipped", 6)["stats"]      # the flipped triangle and its three neighbours; the hole has six edges
    assert (flipped["misoriented_edges"], flipped["nonmanifold_edges"], flipped["cut_triangles"]) == (3, 0, 4)
    assert (flipped["loops"], flipped["longest_loop"], flipped["filled_loops"], flipped["border_edges_after"]) == (1, 6, 1, 0)
    assert result("flipped", 5)["stats"]["border_edges_after"] == 6
    dup = result("duplicated", 32)["stats"]
    assert (dup["nonmanifold_edges"], dup["misoriented_edges"], dup["cut_triangles"], dup["longest_loop"], dup["filled_loops"]) == (3, 0, 5, 6, 1)
    bow = result("bow-tie", 32)["stats"]
    assert (bow["split_vertices"], bow["loops"], bow["cut_triangles"]) == (1, 2, 0) and bow["filled_loops"] == 2
    clustered = result("clustered", 32)["stats"]
    assert clustered["nonmanifold_edges"] == 736 and clustered["cut_triangles"] > 0      # the count of SMOOTH.md's adjacency
    plates = result("plates", 32)["stats"]
    assert (plates["loops"], plates["longest_loop"], plates["filled_loops"], plates["border_edges"]) == (4, 64, 0, 256)
    assert result("plates", 63)["stats"]["filled_loops"] == 0 and result("plates", 64)["stats"]["filled_loops"] == 4
    fan = result("fan", 6000)["stats"]
    assert (fan["loops"], fan["longest_loop"], fan["fill_triangles"], fan["label_rounds"]) == (1, 5001, 5001, 14)
    assert result("fan", 32)["stats"]["filled_loops"] == 0
    umb = result("umbrellas", 32)
    assert sorted(umb["loop_lengths"].tolist()) == sorted((3, 31, 32, 33, 64, 255, 256, 257, 513)) and umb["stats"]["filled_loops"] == 3
    assert umb["stats"]["split_vertices"] == 0 and result("umbrellas", 600)["stats"]["border_edges_after"] == 0


def test_loops_are_ordered_by_their_smallest_half_edge():
    out = result("punched", 0)
    he, loop, pos, tris = out["half_edge"], out["loop"], out["position"], out["triangles"]
    assert (np.diff(he) > 0).all()
    starts = [int(he[(loop == l) & (pos == 0)][0]) for l in range(out["stats"]["loops"])]
    assert starts == sorted(starts) and all(starts[l] == he[loop == l].min() for l in range(len(starts)))
    src, dst = tris.reshape(-1)[he], tris[he // 3, (he % 3 + 1) % 3]
    for l in range(len(starts)):
        order = np.argsort(pos[loop == l])
        assert np.array_equal(np.sort(pos[loop == l]), np.arange(out["loop_lengths"][l]))
        s, d = src[loop == l][order], dst[loop == l][order]
        assert np.array_equal(d, np.roll(s, -1))      # each half-edge ends where the next position starts


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments_are_checked_before_the_device():
    sys.path.insert(0, PKG)
    import torch
    import surfel_repair as P
    from surfel_mesh import TriangleMesh
    mesh = TriangleMesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), None)      # host tensors: a device would be refused later
    for bad in (-1, 1.5, True, False, float("nan"), float("inf"), "3", None, np.bool_(True)):
        with pytest.raises(ValueError, match="surfel_repair: max_hole_edges"):
            P.repair_mesh(mesh, max_hole_edges=bad)
        with pytest.raises(ValueError):
            O.check_cap(bad)
    for good in (0, 32, 4.0, np.int64(7)):
        assert P.check_arguments(good) == int(good) == O.check_cap(good)
        with pytest.raises(RuntimeError, match="HIP device"):
            P.repair_mesh(mesh, max_hole_edges=good)
    with pytest.raises(RuntimeError, match="HIP device"):
        P.border_loops(mesh)
    assert P.COUNTS == O.COUNTS
    import surfel_mesh
    args = surfel_mesh.build_parser().parse_args(["-m", "x"])      # without the flags the mesh CLI repairs nothing
    assert args.repair is False and args.repair_max_hole == 32
    with pytest.raises(SystemExit, match="repair_max_hole"):
        surfel_mesh.main(["-m", "x", "--repair", "--repair_max_hole", "-2"])
    with pytest.raises(ValueError, match="max_hole_edges"):
        P.main(["--ply-path", "x.ply", "--max_hole_edges", "-1"])      # (before the file is opened)


# ------------------------------------------------------------------------------------------------ the library surface
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


def test_repair_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", hdr, re.M)
    assert decl == ["surfel_repair_analyze", "surfel_repair_emit", "surfel_repair_loops"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.REPAIR_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    others = [name for h, group in surfel_native.SIGNATURES.items() if h != HEADER for name in group]
    assert not set(decl) & set(others)
    spec = __import__("importlib.util").util.spec_from_file_location("surfel_build_repair", os.path.join(PKG, "build.py"))
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "mesh_repair.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["mesh_repair.hip"] and any(h.endswith(HEADER) for h in mod.HEADERS)
    import surfel_repair as P
    assert int(re.search(r"#define SURFEL_REPAIR_COUNTS (\d+)", hdr).group(1)) == len(P.COUNTS)
    assert int(re.search(r"#define SURFEL_REPAIR_STAGES (\d+)", hdr).group(1)) == len(P.STAGES)
    # the plan's fields, in the header's order and of the header's kinds
    body = re.search(r"typedef struct surfel_repair_plan \{(.*?)\} surfel_repair_plan;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int64_t|u?int32_t\*)\s+([\w\s,]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    import ctypes as C
    assert [(n, C.c_int64 if c == "int64_t" else C.c_void_p) for n, c in fields] == list(surfel_native.RepairPlan._fields_)


def test_repair_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_repair.h."""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN}
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 3
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES[HEADER])
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert ret == "int" and fn.restype is C.c_int
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            else:
                assert ctype.endswith("*"), where
                assert at in (n.DevPtr, n.Stream, C.c_void_p) or issubclass(at, C._Pointer), where
                host = pname in ("plan", "counts", "stage_ms", "user")      # the HOST pointers of this header
                assert (at is n.DevPtr) == (not host and pname != "stream"), where
                if pname == "plan":
                    assert at is C.POINTER(n.RepairPlan), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_the_size_limit_is_refused_before_any_device_call():
    """3 F = 2^31 and more, or V + 3 F: SURFEL_E_LIMIT with no allocation and no count written (the entry compares the sizes before its
    first device call, so no device is needed); the pointers are never followed"""
    import ctypes as C
    import surfel_native as n
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    counts = (C.c_int64 * 14)(*([-7] * 14))
    plan = n.RepairPlan()
    fake = C.c_void_p(256)
    f_max = (2 ** 31 - 1) // 3
    for V, F in ((10, f_max + 1), (2 ** 31, 0), (2 ** 31 - 3 * 1000, 1000), (2 ** 40, 2 ** 40)):
        with pytest.raises(n.LimitError, match=r"surfel_repair_analyze failed \(-4\): .*2\^31"):
            n.call(None, "surfel_repair_analyze", cb, None, V, F, fake, fake, 32, C.byref(plan), counts, None)
    assert 3 * f_max < 2 ** 31 <= 3 * (f_max + 1)
    assert not taken and list(counts) == [-7] * 14
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
        n.call(None, "surfel_repair_analyze", cb, None, 10, 10, fake, fake, -1, C.byref(plan), counts, None)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
        n.call(None, "surfel_repair_emit", None, fake, None, fake, None, fake, fake, fake, fake)
