"""CPU checks of the JPEG decoder (JPEGDEC.md): the numpy restatement (tests/jpegdec_oracle.py) against Pillow on every fixture, the
round counts the default cap rests on, the host parser's scope, and the C ABI of include/surfel_jpegdec.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpegdec_oracle as JO
import jpegdec_scenes as JS
import surfel_jpegdec as JD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", JS.NAMES + ["own-encoder"])
def test_oracle_equals_pillow(name):
    data = JS.own_encoder() if name == "own-encoder" else JS.jpeg(name)
    want = JS.pillow(data)
    results = {}
    for bits in (128, 1024, 77):
        got, info = JO.decode(data, bits)
        assert info["status"] == "ok" and info["blocks"] == JD.parse(data).nblocks, (name, bits, info)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (name, bits)
        results[bits] = info
    # the fixtures reach their fixed point within half the default cap (JPEGDEC.md "Rounds")
    assert results[128]["rounds"] <= JD.MAX_ROUNDS_DEFAULT // 2 and results[1024]["rounds"] <= JD.MAX_ROUNDS_DEFAULT // 2, (name, results)
    assert results[128]["subsequences"] >= results[1024]["subsequences"]


def test_fixtures_are_what_their_names_say():
    d = {name: JD.parse(JS.jpeg(name)) for name in JS.NAMES}
    assert all(v is not None for v in d.values())
    assert (d["rgb-40x56-420-q90"].hs, d["rgb-40x56-420-q90"].vs, d["rgb-40x56-420-q90"].width, d["rgb-40x56-420-q90"].height) == (2, 2, 40, 56)
    assert (d["rgb-40x56-422-q90"].hs, d["rgb-40x56-422-q90"].vs) == (2, 1) and (d["rgb-40x56-444-q90"].hs, d["rgb-40x56-444-q90"].vs) == (1, 1)
    assert d["gray-40x56"].ncomp == 1 and d["rgb-4x17-420"].width == 4
    assert d["rgb-48x48-420-rows"].restart_interval == 3 and d["rgb-48x48-420-rows"].nintervals == 3
    assert d["rgb-48x48-420-blocks3"].restart_interval == 3
    assert d["rgb-40x56-420-blocks2"].restart_interval == 2 and d["rgb-40x56-420-blocks2"].mcux == 3      # intervals straddle the MCU rows
    assert d["noise-64x64-q100"].restart_interval == 1 and JS.jpeg("noise-64x64-q100").count(b"\xff\x00") >= 50      # stuffed zeros
    assert d["rgb-40x56-420-q30"].bits != d["rgb-40x56-420-q30-opt"].bits                                          # optimised tables
    for name in JS.NAMES:      # the entropy-coded segment starts behind the SOS header, found here by a plain search
        data = JS.jpeg(name)
        sos = data.index(b"\xff\xda")
        assert data.count(b"\xff\xda") == 1 and d[name].ecs_offset == sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"), name
        assert d[name].ecs_bytes == len(data) - d[name].ecs_offset and data[d[name].ecs_offset - 3:d[name].ecs_offset] == b"\x00\x3f\x00"
        sof = data.index(b"\xff\xc0")
        assert [data[sof + 10 + 3 * c + 2] for c in range(d[name].ncomp)] == list(d[name].tq), name
        assert [data[sos + 5 + 2 * c + 1] for c in range(d[name].ncomp)] == [16 * a + b for a, b in zip(d[name].td, d[name].ta)], name
    own = JD.parse(JS.own_encoder())
    assert own.restart_interval == own.mcux and own.nintervals == own.mcuy
    # the synchronisation fixture: no restart markers, many blind subsequences, several rounds
    sync = JO.decode(JS.jpeg(JS.SYNC), 128)[1]
    assert d[JS.SYNC].restart_interval == 0 and sync["rounds"] >= 2 and sync["subsequences"] >= 50, sync


def test_oracle_reports_not_converged_and_damaged():
    pixels, info = JO.decode(JS.jpeg(JS.SYNC), 128, max_rounds=1)
    assert pixels is None and info["status"] == "not converged" and info["rounds"] == 1
    pixels, info = JO.decode(JS.truncated(), 128)
    assert pixels is None and info["status"] == "damaged" and 0 < info["blocks"] < JD.parse(JS.jpeg(JS.SYNC)).nblocks
    # a stream that ends inside its last block, or behind it without EOI, is damaged: Pillow raises "image file is truncated" for
    # every one of these files, and with the marker kept it warns of a premature end
    for name in JS.CUT_NAMES:
        for k in range(4):
            for keep_eoi in (False, True):
                if k == 0 and keep_eoi:
                    continue
                cut = JS.cut_before_eoi(name, k, keep_eoi)
                assert JD.parse(cut) is not None
                for bits in (128, 1024):
                    pixels, info = JO.decode(cut, bits)
                    assert pixels is None and info["status"] == "damaged", (name, k, keep_eoi, bits, info)
            with pytest.raises(OSError, match="truncated"):
                JS.pillow(JS.cut_before_eoi(name, k))
    data = JS.jpeg("rgb-48x48-420-rows")
    cut = data.replace(b"\xff\xd1", b"\x00\x00", 1)      # one restart marker gone
    assert JD.parse(cut) is not None and JO.decode(cut, 128)[1] == {"status": "damaged", "rounds": 0, "subsequences": 0, "blocks": 0}


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_refuses_what_the_device_does_not_decode():
    base = JS.jpeg("rgb-40x56-420-q90")
    assert JD.parse(base) is not None
    assert JD.parse(JS.progressive()) is None and JO.decode(JS.progressive())[1]["status"] == "not supported"
    assert JD.parse(JS.cmyk()) is None
    assert JD.parse(JS.with_segment(base, 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01")) is None
    assert JD.parse(JS.with_segment(base, 0xEE, b"Other\x00")) is not None
    sof = base.index(b"\xff\xc0")
    assert base[sof + 4] == 8
    assert JD.parse(base[:sof + 4] + b"\x0c" + base[sof + 5:]) is None                      # 12-bit precision (synthetic)
    assert JD.parse(base[:sof + 9] + b"\x04" + base[sof + 10:]) is None                     # component id 4
    assert JD.parse(base[:sof + 10] + b"\x41" + base[sof + 11:]) is None                    # luma sampling 4x1
    assert JD.parse(base[:sof + 1] + b"\xc9" + base[sof + 2:]) is None                      # arithmetic coding
    eoi = base.rindex(b"\xff\xd9")
    assert JD.parse(base[:eoi] + b"\xff\xda" + base[eoi + 2:]) is None                      # a second scan
    assert JD.parse(base[2:]) is None and JD.parse(b"") is None and JD.parse(base[:sof]) is None
    assert JD.parse(base[:eoi]) is not None      # no EOI: taken, and reported as damaged by the device (Pillow raises for it too)


def test_segments_are_walked_by_their_lengths():
    """an EXIF thumbnail is a whole JPEG file inside APP1: its SOI, tables, SOS and EOI are skipped"""
    base = JS.jpeg("rgb-40x56-420-q90")
    thumb = JS.jpeg("rgb-8x8-420")
    data = JS.with_segment(JS.with_segment(base, 0xE1, b"Exif\x00\x00" + thumb), 0xFE, b"a comment \xff\xd9")
    d, b = JD.parse(data), JD.parse(base)
    assert d is not None and (d.width, d.height) == (40, 56)
    assert len(data) == len(base) + len(thumb) + 10 + 16 and d.ecs_offset == b.ecs_offset + len(data) - len(base) and d.ecs_bytes == b.ecs_bytes
    assert d.qt == b.qt and d.bits == b.bits and d.huffval == b.huffval
    assert np.array_equal(JO.decode(data)[0], JS.pixels("rgb-40x56-420-q90"))


def test_descriptor_mirrors_the_c_structure():
    import surfel_native as n
    assert C.sizeof(n.JpegDecDesc) == 1656 and n.JpegDecDesc.ecs_offset.offset == 24 and n.JpegDecDesc.qt.offset == 52
    d = JD.parse(JS.jpeg("rgb-40x56-422-q30"))
    assert (d.c.width, d.c.height, d.c.ncomp, d.c.hs, d.c.vs) == (40, 56, 3, 2, 1) and list(d.c.tq)[:3] == [0, 1, 1]
    assert list(d.c.qt[0]) == d.qt[0] and list(d.c.bits[2]) == d.bits[2] and list(d.c.huffval[2])[:len(d.huffval[2])] == d.huffval[2]
    assert (d.mcux, d.mcuy, d.bpm, d.nblocks) == (3, 7, 4, 84)


def test_scratch_bytes_and_argument_checks_need_no_device():
    import surfel_native as n
    d = JD.parse(JS.jpeg("rgb-40x56-420-q90"))
    small, large = JD.scratch_bytes(d, 1024), JD.scratch_bytes(d, 128)
    assert 0 < small < large and small % 16 == 0 and large % 16 == 0
    with pytest.raises(RuntimeError, match=r"\(-1\): jpegdec_scratch_bytes: bad arguments"):
        JD.scratch_bytes(d, 16)
    bad = JD.parse(JS.jpeg("rgb-40x56-420-q90"))
    bad.c.hs = 4
    with pytest.raises(RuntimeError, match=r"\(-1\): jpegdec_scratch_bytes: bad descriptor"):
        JD.scratch_bytes(bad)
    bad.c.hs, bad.c.width = 2, 40000
    with pytest.raises(n.LimitError, match="limits"):
        JD.scratch_bytes(bad)


# ------------------------------------------------------------------------------------------------ the C ABI
def _prototypes(hdr):
    """tests/test_abi_cpu.py's: [(name, return type, [(parameter type, parameter name)])] of every function a header declares, and the
    number of `surfel_xxx(` occurrences outside comments and typedefs, which must be the same number"""
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


def test_header_symbols_are_exported_and_signatures_match():
    import surfel_native as n
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    structs = {"surfel_jpegdec_desc*": n.JpegDecDesc}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    protos, mentions = _prototypes("surfel_jpegdec.h")
    assert len(protos) == mentions == 2
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_jpegdec.h"]) == sorted(n.JPEGDEC_EXPORTS)
    for name, ret, params in protos:
        assert C.cast(getattr(lib, name), C.c_void_p).value, name
        fn = getattr(lib, name)
        assert fn.restype is returns[ret], (name, ret, fn.restype)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            elif ctype in structs:
                assert at is C.POINTER(structs[ctype]), where
            else:
                assert ctype.endswith("*"), where
                assert at in (n.DevPtr, n.Stream, C.c_void_p) or issubclass(at, C._Pointer), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_kernels_do_not_spill():
    """the Huffman and IDCT kernels keep their state in registers: no scratch (JPEGDEC.md "Kernel resources")"""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(REPO, "2d-gaussian-splatting_amd", "csrc", "scene_jpeg.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    found = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            found[name] = int(m.group(1))
    kernels = {k: v for k, v in found.items() if "jpegdec_" in k}
    assert len(kernels) >= 12 and any("huffman" in k for k in kernels) and any("idct" in k for k in kernels), found
    assert all(v == 0 for v in kernels.values()), kernels
