"""CPU tests: the C-ABI library loads (no GPU needed for dlopen) and exports every symbol include/*.h declare;
the Python boundary mirrors the reference's names and error behaviour without touching a device."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    syms = set()
    for hdr in ("surfel_hip.h", "surfel_debug.h", "surfel_train.h"):
        src = open(os.path.join(REPO, "include", hdr)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        syms |= set(re.findall(r"\b(surfel_[a-z0-9_]+)\s*\(", src))
    return sorted(syms - {"surfel_alloc_fn"})


def test_library_exports_every_declared_symbol():
    import ctypes
    import surfel_native
    assert os.path.exists(surfel_native.LIB_PATH), "run python 2d-gaussian-splatting_amd/build.py"
    lib = surfel_native.load()
    syms = _declared_symbols()
    assert len(syms) >= 9
    for s in syms:
        assert hasattr(lib, s), s
        assert ctypes.cast(getattr(lib, s), ctypes.c_void_p).value
    assert sorted(surfel_native.EXPORTS) == syms
    assert lib.surfel_abi_version() == 1


def test_python_surface_names_and_argument_checks():
    import inspect
    import torch
    import diff_surfel_rasterization as d
    assert d.GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
                                                       "viewmatrix", "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    sig = inspect.signature(d.GaussianRasterizer.forward)
    assert list(sig.parameters) == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                                    "cov3D_precomp"]
    rs = d.GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    r = d.GaussianRasterizer(rs)
    x = torch.zeros(2, 3)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=x, means2D=x, opacities=x[:, :1], shs=None, colors_precomp=None, scales=x[:, :2], rotations=torch.zeros(2, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=x, means2D=x, opacities=x[:, :1], shs=None, colors_precomp=x, scales=x[:, :2], rotations=None)
    # CPU tensors are refused loudly — there is no fallback path
    with pytest.raises(RuntimeError, match="HIP device"):
        r(means3D=x, means2D=x, opacities=x[:, :1], shs=None, colors_precomp=x, scales=x[:, :2], rotations=torch.zeros(2, 4))
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="HIP device"):
        distCUDA2(x)


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "2d-gaussian-splatting_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt, f


def test_allocator_frees_by_refcount():
    """The allocator callback must not sit in a reference cycle: its buffers have to die with the last reference,
    not at the next cyclic-GC pass (at 10 M surfels a cycle grew the device footprint by ~13 GB per step)."""
    import ctypes as C
    import gc
    import weakref
    import torch
    import surfel_native as n
    gc.disable()
    try:
        a = n.TorchAllocator("cpu")
        p = a.cb(None, 4096)
        assert p and a.last().numel() == 4096
        w_alloc, w_buf = weakref.ref(a), weakref.ref(a.last())
        del a
        assert w_alloc() is None and w_buf() is None, "TorchAllocator is kept alive by a reference cycle"
    finally:
        gc.enable()


def test_train_header_symbols_are_exported():
    """every function include/surfel_train.h declares is exported by the library"""
    import re
    import surfel_native as n
    lib = n.load()
    hdr = open(os.path.join(REPO, "include", "surfel_train.h")).read()
    names = set(re.findall(r"\bint\s+(surfel_\w+)\s*\(", hdr))
    assert len(names) == 15
    for name in names:
        assert hasattr(lib, name), name
        assert name in n.EXPORTS


def test_ply_roundtrip_and_reference_layout(tmp_path):
    """point_cloud.ply as scene/gaussian_model.py:176-207 lays it out: 61 float properties, binary little endian."""
    import numpy as np
    import surfel_io
    names = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)] + \
        ["opacity", "scale_0", "scale_1"] + ["rot_%d" % i for i in range(4)]
    assert len(names) == 61
    rng = np.random.default_rng(0)
    cols = rng.normal(size=(37, 61)).astype(np.float32)
    p = str(tmp_path / "pc.ply")
    surfel_io.write_ply(p, names, cols)
    raw = open(p, "rb").read()
    head = raw[:raw.index(b"end_header\n") + 11].decode()
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n")
    assert len(raw) == len(head) + 37 * 61 * 4
    back = surfel_io.read_ply(p)
    assert list(back) == names
    for i, n_ in enumerate(names):
        assert np.array_equal(back[n_], cols[:, i])
    # ascii variant (what MeshLab / CloudCompare may re-save)
    with open(p, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment x\nelement vertex 2\nproperty float x\nproperty double y\nend_header\n1 2\n3 4\n")
    b2 = surfel_io.read_ply(p)
    assert b2["x"].tolist() == [1.0, 3.0] and b2["y"].tolist() == [2.0, 4.0]


def test_scratch_sizes_are_bucketed():
    """surfel_native.bucket_bytes: large scratch requests are rounded up to a multiple of 1/16..1/8 of their size, so the R-sized
    buffers of consecutive frames (sizes a few per cent apart) land in the same cached block instead of forcing a fresh hipMalloc at
    every new maximum (measured at 10 M surfels: 290 ms per new maximum and +9.6 GB reserved each time)."""
    import surfel_native as n
    assert n.bucket_bytes(0) == 1 and n.bucket_bytes(1000) == 1000 and n.bucket_bytes((1 << 26) - 1) == (1 << 26) - 1
    prev = 0
    for size in [1 << 26, (1 << 26) + 1, 100_000_000, 129_137_928 * 80, 129_770_365 * 80, 10 ** 11]:
        b = n.bucket_bytes(size)
        assert size <= b <= size * 1.125 + 1 and b >= prev
        assert n.bucket_bytes(b) == b          # a bucket maps to itself
        prev = b
    # the creeping maxima of the C5 bench (instances x 80 B) share one bucket
    assert len({n.bucket_bytes(r * 80) for r in (129_137_928, 129_394_610, 129_434_296, 129_655_849, 129_770_365)}) == 1


def test_surfel_options_environment_hook():
    """SURFEL_OPTIONS="name=value,..." is applied through surfel_set_option when the library is loaded (how an unmodified caller
    such as bench.py is A/B-tested); an unknown option name fails loudly."""
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); import surfel_native as n; n.load(); print('loaded')" % os.path.join(REPO, "2d-gaussian-splatting_amd")
    ok = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SURFEL_OPTIONS="bwd_variant=1, tile_stream=0,cull=1"), capture_output=True, text=True)
    assert ok.returncode == 0 and "loaded" in ok.stdout, ok.stderr[-2000:]
    bad = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SURFEL_OPTIONS="no_such_option=1"), capture_output=True, text=True)
    assert bad.returncode != 0 and "no_such_option" in bad.stderr


def test_image_layout_mirror_matches_the_library():
    """diff_surfel_rasterization.image_layout (what the white-box GPU tests and scripts/tile_lists.py read the image buffer with) against
    ImgState::carve itself."""
    import ctypes
    import surfel_native
    import diff_surfel_rasterization as dsr
    lib = surfel_native.load()
    out = (ctypes.c_int64 * 6)()
    for W, H in [(1, 1), (16, 16), (72, 56), (800, 800), (800, 600), (1600, 1060), (1920, 1080), (3840, 2160), (1023, 1025)]:
        assert lib.surfel_debug_image_layout(W, H, out) == 0
        gx, gy, final_T, n_contrib, tile_map = dsr.image_layout(W, H)
        assert (out[1], out[2], out[3]) == (final_T, n_contrib, tile_map), (W, H, list(out))
        tiles = gx * gy
        assert tile_map < out[0] < tile_map + 4 * 32 * (tiles // 8 + 64) + 256
    assert lib.surfel_debug_image_layout(0, 4, out) < 0


HEADERS = ("surfel_hip.h", "surfel_debug.h", "surfel_train.h", "surfel_mesh.h", "surfel_mesh_unbounded.h", "surfel_eval.h")


def _prototypes(hdr):
    """[(name, return type, [(parameter type, parameter name)])] of every function a header declares (comments stripped; the headers
    are plain C), and the number of `surfel_xxx(` occurrences outside comments and typedefs, which must be the same number."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", hdr)).read(), flags=re.S)
    src = re.sub(r"^\s*(#|typedef\s[^{;]*;).*$", "", src, flags=re.M)
    protos = []
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(surfel_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        plist = []
        for p in (x.strip() for x in params.split(",")):
            if p != "void":
                m = re.fullmatch(r"(.*?)(\w+)", p, flags=re.S)
                plist.append((re.sub(r"\bconst\b|\s+", "", m.group(1)), m.group(2)))
        protos.append((name, re.sub(r"\s+", "", ret), plist))
    return protos, len(re.findall(r"\bsurfel_[a-z0-9_]+\s*\(", src))


def test_every_signature_matches_its_header():
    """surfel_native.SIGNATURES against all six headers: return type, arity and the kind of every parameter of every function.  No
    function is skipped: a header that gains, loses or retypes a parameter fails here."""
    import ctypes as C
    import surfel_native as n
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "surfel_alloc_fn": n.ALLOC_FN,
               "surfel_hook_fn": n.HOOK_FN}
    structs = {"surfel_tsdf_volume*": n.TsdfVolume, "surfel_unbounded_volume*": n.UnboundedVolume, "surfel_eval_grid*": n.EvalGrid}
    returns = {"int": C.c_int, "int64_t": C.c_int64, "constchar*": C.c_char_p}
    parsed = checked = 0
    for hdr in HEADERS:
        protos, mentions = _prototypes(hdr)
        assert len(protos) == mentions, (hdr, len(protos), mentions)
        assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES[hdr]), hdr
        parsed += len(protos)
        for name, ret, params in protos:
            fn = getattr(lib, name)
            assert fn.restype is returns[ret], (name, ret, fn.restype)
            assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
            for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
                where = (name, k, ctype, pname, at)
                if ctype in scalars:
                    assert at is scalars[ctype], where
                elif ctype in structs:
                    assert at is C.POINTER(structs[ctype]), where
                elif ctype == "char*":
                    assert at is C.c_char_p, where
                else:
                    assert ctype.endswith("*"), where
                    assert at in (n.DevPtr, n.Stream, C.c_void_p) or issubclass(at, C._Pointer), where
                # the stream is the last parameter, and call() appends it exactly there
                assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
            checked += 1
    assert checked == parsed and parsed >= 62
    assert parsed == len(n.EXPORTS + n.MESH_EXPORTS + n.UNBOUNDED_EXPORTS + n.EVAL_EXPORTS)


def test_call_maps_error_codes_without_a_device():
    """surfel_native.call: a negative return code raises with the code and the library's own message; SURFEL_E_LIMIT is LimitError (the
    one class the mesh and evaluation modules export as MeshLimitError).  All four calls fail before the library touches a device."""
    import ctypes as C
    import torch
    import surfel_eval
    import surfel_mesh
    import surfel_native as n
    assert surfel_mesh.MeshLimitError is surfel_eval.MeshLimitError is n.LimitError and issubclass(n.LimitError, RuntimeError)
    out = (C.c_int64 * 4)()
    assert n.call(None, "surfel_debug_image_layout", 16, 16, out) == 0
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments") as e:
        n.call(None, "surfel_debug_image_layout", 0, 4, out)
    assert not isinstance(e.value, (n.LimitError, n.CapacityOverflow))
    with pytest.raises(RuntimeError, match=r"surfel_set_option failed \(-1\): .*unknown option"):
        n.call(None, "surfel_set_option", b"no_such_option", 1)
    v = n.TsdfVolume()
    v.dims[:] = [1, 1, 1]
    v.voxel_size, v.sdf_trunc, v.budget_bytes = 0.01, 0.05, 0
    taken = []
    cb = n.ALLOC_FN(lambda user, nbytes: taken.append(nbytes) or None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*budget"):
        n.call(None, "surfel_tsdf_init", v, cb, None)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*budget"):
        n.call(None, "surfel_eval_sample_count", cb, None, 1000, 0, C.c_void_p(256), None, 0.2, 11999, None)
    assert not taken
    # a host tensor never reaches a device-pointer parameter
    with pytest.raises(RuntimeError, match="HIP device"):
        n.call(None, "surfel_debug_set_blend_stats", torch.zeros(8, dtype=torch.int64))
    with pytest.raises(C.ArgumentError, match="HIP device"):      # the same refusal for a caller that goes to the library directly
        n.load().surfel_activate(1, torch.zeros(58), torch.zeros(7), None)


def test_allocator_view_finds_a_held_buffer_by_its_address():
    import torch
    import surfel_native as n
    a = n.TorchAllocator("cpu")
    p0, p1 = a.cb(None, 64), a.cb(None, 4096)
    v = a.view(p1, torch.float32, (4, 8))
    assert v.shape == (4, 8) and v.dtype == torch.float32 and v.data_ptr() == p1 and a.view(p0, torch.uint8, (64,)).data_ptr() == p0
    with pytest.raises(KeyError):
        a.view(p1 + 4, torch.float32, (1,))
