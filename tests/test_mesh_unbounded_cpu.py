"""CPU checks of the unbounded mesh extraction (MESH.md §Unbounded): the oracle's contraction, lattice, truncation and bilinear
convention against closed forms and the reference's formulas, and the library surface of include/surfel_mesh_unbounded.h."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import mesh_oracle as MO  # noqa: E402
import mesh_unbounded_oracle as U  # noqa: E402


def _pkg():
    sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))


def test_contraction_round_trip():
    rng = np.random.default_rng(0)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([rng.uniform(0.0, 0.999, 1000), rng.uniform(1.001, 40.0, 1000)])
    x = d * r[:, None]
    y = U.contract(x)
    mag = np.linalg.norm(y, axis=1)
    assert np.allclose(y[:1000], x[:1000], rtol=0, atol=0)                 # identity inside the unit ball
    assert np.all(mag[1000:] > 1) and np.all(mag[1000:] < 2)
    assert np.allclose(mag[1000:], 2 - 1 / r[1000:], rtol=1e-12)
    assert np.allclose(U.uncontract(y), x, rtol=1e-10, atol=1e-12)
    torch = pytest.importorskip("torch")
    _pkg()
    import surfel_mesh
    xt = torch.from_numpy(x)
    assert torch.allclose(surfel_mesh.uncontract(surfel_mesh.contract(xt)), xt, rtol=1e-10, atol=1e-12)
    assert torch.allclose(surfel_mesh.contract(xt), torch.from_numpy(y), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("N,M", [(512, 512), (1024, 1023), (2048, 2045)])
def test_lattice_size(N, M):
    assert U.lattice_size(N) == M
    torch = pytest.importorskip("torch")  # noqa: F841
    _pkg()
    import surfel_mesh
    assert surfel_mesh.lattice_size(N) == M


def test_lattice_is_the_union_of_the_reference_crops():
    """mcube_utils.py:31-52: N/512 crops per axis, 512 linspace samples each, endpoints included; the distinct samples are the
    uniform lattice -R + j * 2R/(M-1) to within a few ulps"""
    R, N = 1.37, 1536
    cuts = np.linspace(-R, R, N // 512 + 1)
    crop = np.concatenate([np.linspace(cuts[i], cuts[i + 1], 512) for i in range(N // 512)])
    M = U.lattice_size(N)
    lat = -R + np.arange(M) * (2 * R / (M - 1))
    distinct = np.unique(np.round(crop, 9))
    assert len(distinct) == M
    assert np.max(np.abs(distinct - lat)) < 1e-9
    R32, step = U.lattice_step(M, R)             # the library's fp32 R and step
    s = np.arange(M) * step - R32
    assert np.max(np.abs(s - lat)) < 4 * np.finfo(np.float32).eps * R * M


def test_adaptive_truncation():
    vs = 0.01
    s = np.array([[0.5, 0, 0], [0, 1.0, 0], [0, 0, 1.5], [1.95, 0, 0], [0, -1.2, 0]])
    tr = U.adaptive_trunc(s, vs)
    v = float(np.float32(vs))
    assert np.allclose(tr, [5 * v, 5 * v, 5 * v / 0.5, 5 * v / 0.1, 5 * v / 0.8], rtol=1e-12)


def test_bilinear_align_corners_by_hand():
    img = np.array([[1.0, 2.0, 4.0], [10.0, 20.0, 40.0]])      # H = 2, W = 3
    # ndc (0.25, -0.5): px = 1.25 / 2 * 2 = 1.25, py = 0.5 / 2 * 1 = 0.25
    v, slope = U.bilinear(img, np.array([0.25]), np.array([-0.5]))
    top, bottom = 2.0 + 0.25 * (4.0 - 2.0), 20.0 + 0.25 * (40.0 - 20.0)
    assert abs(v[0] - (0.75 * top + 0.25 * bottom)) < 1e-12 and abs(v[0] - 8.125) < 1e-12
    assert slope[0] == 36.0      # |40 - 4|, the largest step between neighbouring taps
    v, _ = U.bilinear(img, np.array([-1.0, 1.0, 1.0]), np.array([-1.0, -1.0, 1.0]))      # corners land on pixel centres
    assert np.allclose(v, [1.0, 4.0, 40.0])
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = np.random.default_rng(1)
    big = rng.normal(size=(7, 11))
    nx, ny = rng.uniform(-1, 1, 500), rng.uniform(-1, 1, 500)
    g = torch.from_numpy(np.stack([nx, ny], -1))[None, None]
    ref = F.grid_sample(torch.from_numpy(big)[None, None], g, mode="bilinear", padding_mode="border", align_corners=True).reshape(-1).numpy()
    assert np.allclose(U.bilinear(big, nx, ny)[0], ref, rtol=0, atol=1e-12)


def test_oracle_lattice_sphere_is_closed():
    M, R = 41, 1.0
    s = U.lattice_contracted(M, R)
    tsdf = np.clip((np.linalg.norm(s - [0.03, -0.02, 0.05], axis=1) - 0.6) / 0.1, -1, 1).reshape(M, M, M)
    verts, tris = U.marching_cubes(tsdf, R, [0.0, 0.0, 0.0], 1.0)
    assert len(tris) > 500
    assert MO.closed_oriented_manifold(tris)
    assert MO.euler(verts, tris) == 2
    assert np.all(np.bincount(tris.reshape(-1), minlength=len(verts)) > 0)
    n = MO.face_normals(verts, tris)
    big = np.linalg.norm(n, axis=1) > 1e-12
    assert np.mean(np.einsum("ij,ij->i", n, verts[tris].mean(1) - [0.03, -0.02, 0.05])[big] > 0) > 0.99      # toward increasing tsdf


def _lib():
    return os.path.join(REPO, "2d-gaussian-splatting_amd", "lib", "libsurfel_hip.so")


def test_unbounded_header_exported():
    _pkg()
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", "surfel_mesh_unbounded.h")).read(), re.M)
    assert len(decl) == 6
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.UNBOUNDED_EXPORTS) == sorted(decl)
    assert not set(decl) & set(surfel_native.EXPORTS + surfel_native.MESH_EXPORTS)
    import ctypes
    assert ctypes.sizeof(surfel_native.UnboundedView) == 64
    assert ctypes.sizeof(surfel_native.UnboundedVolume) == 112


def test_unbounded_budget_checked_on_the_host():
    """surfel_unbounded_bytes and the limit of surfel_unbounded_init need no device: nothing is allocated when the budget is short"""
    _pkg()
    import ctypes
    import surfel_native
    lib = surfel_native.load()
    v = surfel_native.UnboundedVolume()
    v.M, v.R, v.radius, v.voxel_size = 1023, 1.5, 2.0, 0.004
    need = lib.surfel_unbounded_bytes(ctypes.byref(v))
    assert need > 4 * 1023 ** 3 and need < 4 * 1023 ** 3 + (1 << 30)      # lattice + about 0.8 GB of slab scratch
    v.budget_bytes = need - 1
    calls = []
    cb = surfel_native.ALLOC_FN(lambda user, n: calls.append(n) or None)
    assert lib.surfel_unbounded_init(ctypes.byref(v), cb, None, None) == -4
    assert calls == [] and not v.tsdf
    v.M = 1
    assert lib.surfel_unbounded_bytes(ctypes.byref(v)) == -1


def test_unbounded_kernels_no_scratch():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    ks = isa_count.kernels(isa_count.assemble("mesh_unbounded.hip"))
    names = [k for k in ks if "unb_" in k]
    assert len(names) == 5, names
    for k in names:
        assert int(ks[k][1].get("private_segment_fixed_size", 0)) == 0, k
