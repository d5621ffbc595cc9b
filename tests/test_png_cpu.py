"""CPU tests of the PNG encoder (PNG.md): the numpy restatement (tests/png_oracle.py) against Pillow's decoder and zlib — pixels, inflate,
Adler-32, CRC-32, the chunk structure field by field — the code construction (complete, within 15 / 7 bits, the limit in fact hit), the
size against zlib's Z_RLE and Pillow's default, the capacity bound, and the library's surface without a device."""
import ctypes as C
import functools
import io
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_oracle as PO
import png_scenes as PS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured with this restatement: (IDAT payload, zlib Z_RLE level 6 over the same filtered bytes as one stream, file, Pillow's default file)
MEASURED = {
    "gray-1x1": (20, 10, 77, 67),
    "rgb-1x1": (22, 12, 79, 69),
    "noise-17x33": (1751, 1711, 1808, 1768),
    "const-5x300": (34, 34, 91, 90),
    "runs-1x1824": (34, 34, 91, 95),
    "gradients-60x96": (2139, 2139, 2196, 1804),
    "fibonacci-1x28656": (23510, 23638, 23567, 17085),
    "stripes-33x700": (17617, 17557, 17674, 9445),
    "disc-40x40": (1203, 1203, 1260, 849),
    "ragged-7x13": (52, 53, 109, 111),
    "white-9x31": (35, 35, 92, 83),
    "noise-gray-64x64": (4200, 4171, 4257, 4228),
}


@functools.lru_cache(maxsize=None)
def analysed(name):
    return PO.analyse(PS.scene(name))


def _pillow(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[:, :, None] if a.ndim == 2 else a


def _chunks(data):
    out, p = [], 8
    while p < len(data):
        n, kind = struct.unpack(">I4s", data[p:p + 8])
        out.append((kind, data[p + 8:p + 8 + n], struct.unpack(">I", data[p + 8 + n:p + 12 + n])[0]))
        p += 12 + n
    assert p == len(data)
    return out


# ------------------------------------------------------------------------------------------------ 1. the file
@pytest.mark.parametrize("name", PS.NAMES)
def test_oracle_file_decodes_to_the_input(name):
    img, a = PS.scene(name), analysed(name)
    H, W, Cn = img.shape
    data = a["file"]
    assert np.array_equal(_pillow(data), img)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    chunks = _chunks(data)
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    for kind, payload, crc in chunks:
        assert crc == zlib.crc32(kind + payload), kind
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 0 if Cn == 1 else 2, 0, 0, 0) and chunks[2][1] == b""
    idat = chunks[1][1]
    assert idat == a["idat"] and data.index(b"IDAT") + 4 + 2 == PO.FRONT
    assert idat[:2] == b"\x78\x01" and (idat[0] * 256 + idat[1]) % 31 == 0
    stream = a["stream"].tobytes()
    assert len(stream) == H * (1 + W * Cn)
    assert zlib.decompress(idat) == stream
    assert struct.unpack(">I", idat[-4:])[0] == zlib.adler32(stream) == PO.adler32(a["stream"])
    assert PO.crc32(b"IDAT" + idat) == zlib.crc32(b"IDAT" + idat)
    assert len(a["stripes"]) == len(PO.stripe_lengths(H, W, Cn))
    # every row's filter is the one with the smallest sum of |residual| among Pillow-decodable candidates: the stream's first bytes
    assert np.array_equal(a["stream"][:, 0], a["filters"]) and a["filters"].max() <= 4


def test_stripes_are_independent_and_byte_aligned():
    """every stripe's bytes inflate on their own (raw deflate) to exactly its rows; all but the last end with the empty stored block"""
    img, a = PS.scene("stripes-33x700"), analysed("stripes-33x700")
    lens = PO.stripe_lengths(*img.shape)
    assert lens == [16 * 2101, 16 * 2101, 2101]
    flat, off = a["stream"].reshape(-1), 0
    for k, L in enumerate(lens):
        data, _ = PO.stripe_block(flat[off:off + L], k == len(lens) - 1)
        d = zlib.decompressobj(-15)
        assert d.decompress(data) == flat[off:off + L].tobytes() and d.eof == (k == len(lens) - 1) and d.unused_data == b""
        assert k == len(lens) - 1 or data[-4:] == b"\x00\x00\xff\xff"
        off += L


def test_tokens_of_the_run_scene():
    """runs of exactly 2, 3, 4, 258, 259, 260, 261, 517: a literal, then matches in greedy chunks of 258, a remainder below 3 as literals"""
    a = analysed("runs-1x1824")
    assert list(a["filters"]) == [1]      # Sub: the runs become one differing byte and zeros
    row = PS.scene("runs-1x1824").reshape(-1)
    tok = PO.tokens(row)
    got, p = [], 0
    for k in PS.RUNS:
        got.append([int(t) for t in tok[p:p + k] if t >= 0])
        p += k
    v = [int(row[sum(PS.RUNS[:i])]) for i in range(len(PS.RUNS))]
    assert got == [[v[0], v[0]], [v[1], v[1], v[1]], [v[2], 256 + 3], [v[3], 256 + 257], [v[4], 256 + 258], [v[5], 256 + 258, v[5]],
                   [v[6], 256 + 258, v[6], v[6]], [v[7], 256 + 258, 256 + 258]]


def test_every_filter_wins_a_row_of_the_gradients():
    assert sorted(set(analysed("gradients-60x96")["filters"].tolist())) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ 2. codes
@pytest.mark.parametrize("name", PS.NAMES)
def test_codes_are_complete_and_within_their_limits(name):
    for info in analysed(name)["stripes"]:
        ll, cl = info["ll_len"], info["cl_len"]
        assert int((ll > 0).sum()) >= 2 and ll.max() <= 15 and PO.kraft(ll, 15) == 1 << 15
        assert int((cl > 0).sum()) >= 2 and cl.max() <= 7 and PO.kraft(cl, 7) == 1 << 7
        assert np.array_equal(ll > 0, info["hist"] > 0) and ll[256] > 0
        assert info["matches"] == bool(info["hist"][257:].any())


def test_the_length_limit_is_hit_on_the_fibonacci_scene():
    (info,) = analysed("fibonacci-1x28656")["stripes"]
    assert info["ll_hit"], "the scene no longer needs more than 15 bits without the limit"
    assert info["ll_len"].max() == 15
    # the construction on its own: Fibonacci counts, 30 symbols -> 29 bits without a limit
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for limit in (7, 15):
        lengths, hit = PO.code_lengths(np.array(fib[:25] if limit == 15 else fib[:12]), limit)
        assert hit and lengths.max() == limit and PO.kraft(lengths, limit) == 1 << limit
    lengths, hit = PO.code_lengths(np.array([5, 0, 0, 7]), 15)
    assert not hit and list(lengths) == [1, 0, 0, 1]
    codes = PO.canonical_codes(np.array([3, 3, 3, 3, 3, 2, 4, 4]))      # RFC 1951 3.2.2's example, bit-reversed
    assert [int(c) for c in codes] == [0b010, 0b110, 0b001, 0b101, 0b011, 0b00, 0b0111, 0b1111]


def test_code_length_run_lengths():
    assert PO.rle_lengths([0] * 140 + [5] * 8 + [0, 0] + [3]) == [(18, 7, 127), (0, 0, 0), (0, 0, 0), (5, 0, 0), (16, 2, 3), (5, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0)]
    assert PO.rle_lengths([0] * 10 + [7, 7, 7]) == [(17, 3, 7), (7, 0, 0), (7, 0, 0), (7, 0, 0)]


# ------------------------------------------------------------------------------------------------ 3. size
@pytest.mark.parametrize("name", PS.NAMES)
def test_size_against_zlib_rle_and_pillow(name):
    """the bar is the ratio measured with this restatement plus 0.02 (PNG.md: the device is byte-equal to the restatement)"""
    from PIL import Image
    img, a = PS.scene(name), analysed(name)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    rle = co.compress(a["stream"].tobytes()) + co.flush()
    f = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(f, "PNG")
    pil = f.getvalue()
    m = MEASURED[name]
    print("%s: IDAT %d, Z_RLE %d (%.3f), file %d, Pillow %d (%.3f)" % (name, len(a["idat"]), len(rle), len(a["idat"]) / len(rle), len(a["file"]), len(pil),
                                                                     len(a["file"]) / len(pil)))
    assert len(a["idat"]) / len(rle) <= m[0] / m[1] + 0.02
    assert len(a["file"]) / len(pil) <= m[2] / m[3] + 0.02


def test_capacity_bound_holds_on_every_scene():
    import surfel_native as n
    extra = [np.full((40, 900, 3), 255, np.uint8), np.random.default_rng(4).integers(0, 256, size=(70, 500, 3), dtype=np.uint8)]
    for img in [PS.scene(name) for name in PS.NAMES] + extra:
        H, W, Cn = img.shape
        cap = PO.capacity(H, W, Cn)
        assert cap == n.call(None, "surfel_png_capacity", H, W, Cn)
        assert cap >= len(PO.encode(img)), (H, W, Cn)
        assert n.call(None, "surfel_png_scratch_bytes", H, W, Cn) % 16 == 0
    assert PO.stripe_capacity(1) == (15 + 2140 + 31) // 32 * 4 and 17 + 19 * 3 + 287 * 7 + 15 + 42 == PO.STRIPE_EXTRA_BITS


# ------------------------------------------------------------------------------------------------ 4. ABI, arguments, resources
def test_png_header_signatures_and_exports():
    """include/surfel_png.h <-> SIGNATURES["surfel_png.h"] <-> PNG_EXPORTS <-> the library's exports, both ways"""
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_png.h")
    assert len(protos) == mentions == 3
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_png.h"]) == sorted(n.PNG_EXPORTS)
    scalars = {"int": C.c_int, "int64_t": C.c_int64}
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert C.cast(fn, C.c_void_p).value and fn.restype is scalars[ret], name
        assert len(fn.argtypes) == len(params), name
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            else:
                assert ctype.endswith("*") and at is (n.Stream if pname == "stream" else n.DevPtr), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
    out = subprocess.run(["nm", "-D", "--defined-only", n.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(surfel_png_\w+)\b", out))) == sorted(p[0] for p in protos)
    hdr = open(os.path.join(REPO, "include", "surfel_png.h")).read()
    for macro, value in (("FRONT_BYTES", PO.FRONT), ("STRIPE_BYTES", PO.STRIPE_BYTES), ("STRIPE_EXTRA_BITS", PO.STRIPE_EXTRA_BITS)):
        assert int(re.search(r"#define SURFEL_PNG_%s (\d+)" % macro, hdr).group(1)) == value, macro
    assert "#define SURFEL_PNG_MAX_ROW (1 << 20)" in hdr and "#define SURFEL_PNG_MAX_STREAM (1 << 30)" in hdr
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_png_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "frame_png.hip" in mod.SOURCES and "frame_png.hip" not in mod.EXTRA and any(h.endswith("surfel_png.h") for h in mod.HEADERS)


def test_png_entries_check_their_arguments_without_a_device():
    import surfel_native as n
    p = C.c_void_p(4096)
    cap, scr = n.call(None, "surfel_png_capacity", 17, 33, 3), n.call(None, "surfel_png_scratch_bytes", 17, 33, 3)

    def enc(H=17, W=33, Cn=3, pix=p, dst=p, capacity=cap, size=p, scratch=p, scratch_bytes=scr):
        return n.call(None, "surfel_png_encode", H, W, Cn, pix, dst, capacity, size, scratch, scratch_bytes)

    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(Cn=2), dict(Cn=4), dict(Cn=0), dict(pix=None), dict(dst=None), dict(size=None), dict(scratch=None),
               dict(size=C.c_void_p(4100)), dict(scratch=C.c_void_p(4100))):
        with pytest.raises(RuntimeError, match=r"\(-1\): png_encode: bad arguments"):
            enc(**kw)
    with pytest.raises(RuntimeError, match=r"\(-1\): png_encode: capacity"):
        enc(capacity=cap - 1)
    with pytest.raises(RuntimeError, match=r"\(-1\): png_encode: scratch"):
        enc(scratch_bytes=scr - 1)
    for kw in (dict(W=(1 << 20) // 3 + 1), dict(W=1 << 20, Cn=1), dict(H=1 << 20, W=1 << 10, Cn=1)):
        with pytest.raises(n.LimitError, match="limits"):
            enc(**kw)
    for name in ("surfel_png_capacity", "surfel_png_scratch_bytes"):
        with pytest.raises(RuntimeError, match=r"\(-1\): png_\w+: bad arguments"):
            n.call(None, name, 0, 5, 3)
        with pytest.raises(RuntimeError, match=r"\(-1\): png_\w+: bad arguments"):
            n.call(None, name, 5, 5, 2)
        with pytest.raises(n.LimitError, match="limits"):
            n.call(None, name, 1 << 15, 1 << 15, 1)
    assert n.call(None, "surfel_png_capacity", 1024, (1 << 20) - 1, 1) == 43 + 1024 * PO.stripe_capacity(1 << 20) + 20      # the largest frame


def test_python_layer_refuses_what_it_cannot_encode(tmp_path):
    import torch
    import surfel_mesh
    import surfel_path as SP
    import surfel_png as SG
    with pytest.raises(RuntimeError, match="HIP device"):
        SG.encode_png(torch.zeros((4, 4, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        SG.png_bytes(np.zeros((4, 4, 3), np.uint8))
    assert SG.capacity(17, 33, 3) == PO.capacity(17, 33, 3) and SG.scratch_bytes(17, 33, 3) > 17 * 100 * 3
    with pytest.raises(ValueError, match="pillow"):
        SP.FrameWriter(png="libpng")
    args = surfel_mesh.build_parser().parse_args(["-m", "x"])
    assert args.png == "pillow" and surfel_mesh.path_png_args(args) == {}      # render_path and export_image are called as they always were
    args = surfel_mesh.build_parser().parse_args(["-m", "x", "--png", "device"])
    assert surfel_mesh.path_png_args(args) == dict(png="device")
    with pytest.raises(SystemExit):
        surfel_mesh.build_parser().parse_args(["-m", "x", "--png", "gpu"])


def test_frame_writer_keeps_host_frames_on_pillow(tmp_path):
    """png="device" changes nothing for host tensors and TIFFs: the same bytes as the default writer (no device is touched)"""
    import torch
    import surfel_path as SP
    frames = [torch.from_numpy(np.array(PS.scene(name))) for name in ("noise-17x33", "disc-40x40", "ragged-7x13")]
    depth = torch.linspace(0, 3, 35).reshape(5, 7)
    for mode in ("pillow", "device"):
        os.makedirs(str(tmp_path / mode))
        with SP.FrameWriter(workers=2, ring=2, png=mode) as fw:
            for k, f in enumerate(frames):
                fw.submit(str(tmp_path / mode / ("%d.png" % k)), f)
            fw.submit(str(tmp_path / mode / "d.tiff"), depth)
        assert fw.frames == 4
    for f in sorted(os.listdir(str(tmp_path / "pillow"))):
        assert open(str(tmp_path / "pillow" / f), "rb").read() == open(str(tmp_path / "device" / f), "rb").read(), f


def test_png_kernels_do_not_spill():
    """registers, LDS and scratch of the seven launches, from the assembly's own kernel descriptors: nothing in private memory"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("surfel_build_for_png_resources", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + ["-S", "--cuda-device-only", os.path.join(B.CSRC, "frame_png.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    seen = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", text, re.S):
        md = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, m.group(2)).group(1)) for k in ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size")}
        seen[re.search(r"png_\w+?_kernel", m.group(1)).group(0)] = md
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md["next_free_vgpr"] <= 128 and md["group_segment_fixed_size"] <= 16 * 1024, (m.group(1), md)      # 1024 threads: 4 waves / SIMD
    assert sorted(seen) == ["png_codes_kernel", "png_compact_kernel", "png_emit_kernel", "png_filter_kernel", "png_finish_kernel", "png_layout_kernel",
                            "png_token_kernel"]
