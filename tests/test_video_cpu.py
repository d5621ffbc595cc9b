"""CPU tests of the trajectory videos (VIDEO.md): the numpy restatement of the JPEG encoder (tests/video_oracle.py) against libjpeg
(what it decodes, how well, how large), against an fp64 transform, the generated tables, the C ABI and its argument checks, the AVI
writer through an independent reader, and the CLI's flags.  Nothing here touches a device."""
import ctypes as C
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import video_oracle as VO
import video_scenes as VS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def oracle(name, quality):
    stats = {}
    return VO.encode(VS.scene(name), quality, stats), stats


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _libjpeg(img, quality):
    """the same image through libjpeg with the same tables: 4:2:0, the typical Huffman tables"""
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", quality=quality, subsampling=2, optimize=False)
    return f.getvalue()


def _mse(a, b):
    return float(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean())


# ------------------------------------------------------------------------------------------------ 1. what the scenes exercise
def test_scene_set_covers_every_size_and_content():
    assert sorted({(H, W) for _, _, H, W in VS.SCENES}) == sorted(VS.SIZES)
    assert {c for _, c, _, _ in VS.SCENES} == set(VS.CONTENTS)
    for name in VS.NAMES:
        a, b = VS.scene(name), VS.scene(name)
        assert a.dtype == np.uint8 and np.array_equal(a, b)      # seeded


def test_symbol_stream_coverage():
    """asserted, not hoped for: ZRL, EOB and a block without one, DC category 11 and AC category 10, a stuffed 0xFF, RST7 then RST0"""
    st = [oracle(name, q)[1] for name in VS.NAMES for q in VS.QUALITIES]
    assert sum(s["zrl"] for s in st) > 0
    assert sum(s["eob"] for s in st) > 0 and sum(s["no_eob"] for s in st) > 0
    at100 = [oracle(name, 100)[1] for name in VS.NAMES]
    assert max(s["dc_cat"] for s in at100) == 11 and max(s["ac_cat"] for s in at100) == 10
    assert sum(s["stuffed"] for s in st) > 0
    ten_rows = oracle("noise-150x218", 95)
    assert ten_rows[1]["rst"] == [0, 1, 2, 3, 4, 5, 6, 7, 0] and b"\xff\xd7" in ten_rows[0] and b"\xff\xd0" in ten_rows[0]
    assert oracle("highfreq-272x16", 95)[1]["rst"] == [k % 8 for k in range(16)]      # wraps twice
    assert all(oracle(name, 75)[1]["zrl"] > 0 for name in VS.NAMES if name.startswith("highfreq"))      # runs longer than 15


def test_stuffing_leaves_no_bare_marker_in_the_entropy_data():
    for name in VS.NAMES:
        data, st = oracle(name, 100)
        body = data[629:-2]
        k, rst = 0, []
        while True:
            k = body.find(b"\xff", k)
            if k < 0:
                break
            nxt = body[k + 1]
            assert nxt == 0 or 0xD0 <= nxt <= 0xD7, (name, k, nxt)
            if nxt:
                rst.append(nxt - 0xD0)
            k += 2
        assert rst == st["rst"], name


# ------------------------------------------------------------------------------------------------ 2. libjpeg reads it
@pytest.mark.parametrize("name", VS.NAMES)
def test_pillow_decodes_every_oracle_file(name):
    img = VS.scene(name)
    for q in VS.QUALITIES:
        data = oracle(name, q)[0]
        assert data[:2] == b"\xff\xd8" and data[6:11] == b"JFIF\0" and data[-2:] == b"\xff\xd9"
        im = _decode(data)
        assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
        assert np.asarray(im).shape == img.shape


@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
def test_quantisation_tables_are_libjpegs(quality):
    img = VS.scene("smooth-37x51")
    ours, theirs = _decode(VO.encode(img, quality)), _decode(_libjpeg(img, quality))
    assert {k: list(v) for k, v in ours.quantization.items()} == {k: list(v) for k, v in theirs.quantization.items()}
    assert sorted(ours.quantization) == [0, 1]


def test_header_layout():
    data = oracle("edges-17x33", 95)[0]
    import gen_jpeg_tables as GT
    seg = GT.segments(data)
    assert [m for m, _ in seg] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert sum(len(p) + 4 for _, p in seg) + 2 == 629
    assert seg[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert seg[3][1] == bytes([8, 0, 17, 0, 33, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [p[0] for _, p in seg[4:8]] == [0x00, 0x10, 0x01, 0x11]
    assert seg[8][1] == bytes([0, 3])      # one MCU row of ceil(33 / 16)


# ------------------------------------------------------------------------------------------------ 3. against libjpeg and fp64
@pytest.mark.parametrize("name", VS.NAMES)
def test_error_and_size_against_libjpeg(name):
    img = VS.scene(name)
    for q in (95, 75):
        ours, theirs = oracle(name, q)[0], _libjpeg(img, q)
        e_ours, e_theirs = _mse(_decode(ours), img), _mse(_decode(theirs), img)
        print("%s q%d: mse %.4f / %.4f, bytes %d / %d = %.4f" % (name, q, e_ours, e_theirs, len(ours), len(theirs), len(ours) / len(theirs)))
        assert e_ours <= max(e_theirs * 1.023, 0.05 if name.startswith("flat") else 0.0), (name, q, e_ours, e_theirs)      # (the floor: the flat scene only)
        assert len(ours) <= 1.10 * len(theirs) + 64, (name, q, len(ours), len(theirs))
        if img.shape[:2] == (150, 218):
            assert len(ours) <= 1.05 * len(theirs), (name, q, len(ours), len(theirs))


@pytest.mark.parametrize("name", VS.NAMES)
def test_fp32_coefficients_against_fp64(name):
    img = VS.scene(name)
    for q in VS.QUALITIES:
        a, b = VO.coefficients(img, q), VO.coefficients(img, q, exact=True)
        d = np.abs(a - b)
        print("%s q%d: %d of %d differ" % (name, q, int((d != 0).sum()), d.size))
        assert d.max() <= 1 and int((d != 0).sum()) <= 0.001 * d.size, (name, q, int(d.max()), int((d != 0).sum()), d.size)


def test_capacity_bound_holds_on_every_scene():
    import surfel_native as n
    for name, _, H, W in VS.SCENES:
        cap = n.call(None, "surfel_jpeg_capacity", H, W)
        assert cap == VO.capacity(H, W) and cap >= len(oracle(name, 100)[0]), name
        assert n.call(None, "surfel_jpeg_scratch_bytes", H, W) % 16 == 0


# ------------------------------------------------------------------------------------------------ 4. tables, ABI, arguments
def test_generated_tables_are_current():
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "gen_jpeg_tables.py"), "--check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    import gen_jpeg_tables as GT
    zz = GT.zigzag()
    assert sorted(zz) == list(range(64)) and list(zz[:6]) == [0, 1, 8, 16, 9, 2] and zz[63] == 63
    A, (B, K) = GT.dct_matrix(), GT.dct_factors()
    assert np.allclose(A @ A.T, np.eye(8), atol=1e-12)      # orthonormal
    assert B.dtype == K.dtype == np.float32 and np.all(B[0] == 1.0) and K[0, 0] == 0.125
    assert np.allclose(np.sqrt(np.diag(K).astype(np.float64))[:, None] * B, A, atol=1e-7)      # A = diag(c / 2) B, K[v][u] = c(v) c(u) / 4
    assert np.allclose(K, np.outer(np.sqrt(np.diag(K)), np.sqrt(np.diag(K))), atol=1e-7)
    for (tc, th), (bits, vals) in GT.huffman_spec().items():
        code, length = GT.huffman_codes(bits, vals)
        assert len(vals) == (12 if tc == 0 else 162) and int((length > 0).sum()) == len(vals)
        assert sum(2.0 ** -int(ln) for ln in length if ln) < 1.0      # a prefix code with the all-ones word left out
    assert VO.scaled_tables(50).tolist() == GT.quant_base().tolist() and np.all(VO.scaled_tables(100) == 1)


def test_jpeg_header_signatures_and_exports():
    """include/surfel_jpeg.h <-> SIGNATURES["surfel_jpeg.h"] <-> JPEG_EXPORTS <-> the library's exports, both ways"""
    import re
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_jpeg.h")
    assert len(protos) == mentions == 3
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_jpeg.h"]) == sorted(n.JPEG_EXPORTS)
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
    assert [p[1] for p in dict((p[0], p[2]) for p in protos)["surfel_jpeg_encode"]][-1] == "stream"
    out = subprocess.run(["nm", "-D", "--defined-only", n.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(surfel_jpeg_\w+)\b", out))) == sorted(p[0] for p in protos)
    hdr = open(os.path.join(REPO, "include", "surfel_jpeg.h")).read()
    assert int(re.search(r"#define SURFEL_JPEG_HEADER_BYTES (\d+)", hdr).group(1)) == len(VO.header(16, 16, 95))
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_video_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "frame_jpeg.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["frame_jpeg.hip"]
    assert any(h.endswith("surfel_jpeg.h") for h in mod.HEADERS) and "jpeg_tables.h" in mod.HEADERS


def test_jpeg_entries_check_their_arguments_without_a_device():
    import surfel_native as n
    p = C.c_void_p(4096)
    cap, scr = n.call(None, "surfel_jpeg_capacity", 17, 33), n.call(None, "surfel_jpeg_scratch_bytes", 17, 33)

    def enc(H=17, W=33, rgb=p, quality=95, dst=p, capacity=cap, size=p, scratch=p, scratch_bytes=scr):
        return n.call(None, "surfel_jpeg_encode", H, W, rgb, quality, dst, capacity, size, scratch, scratch_bytes)

    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(quality=0), dict(quality=101), dict(rgb=None), dict(dst=None), dict(size=None),
               dict(scratch=None), dict(size=C.c_void_p(4100)), dict(scratch=C.c_void_p(4100))):
        with pytest.raises(RuntimeError, match=r"\(-1\): jpeg_encode: bad arguments"):
            enc(**kw)
    with pytest.raises(RuntimeError, match=r"\(-1\): jpeg_encode: capacity"):
        enc(capacity=cap - 1)
    with pytest.raises(RuntimeError, match=r"\(-1\): jpeg_encode: scratch"):
        enc(scratch_bytes=scr - 1)
    with pytest.raises(n.LimitError, match="65535"):
        enc(W=65536)
    for name in ("surfel_jpeg_capacity", "surfel_jpeg_scratch_bytes"):
        with pytest.raises(RuntimeError, match=r"\(-1\): jpeg_\w+: bad arguments"):
            n.call(None, name, 0, 5)
        with pytest.raises(n.LimitError, match="65535"):
            n.call(None, name, 70000, 5)
    assert n.call(None, "surfel_jpeg_capacity", 65535, 65535) == 629 + 4096 * (4096 * 2496 + 4)


def test_device_entries_refuse_host_tensors():
    import torch
    import surfel_video as SV
    with pytest.raises(RuntimeError, match="HIP device"):
        SV.encode_jpeg(torch.zeros((4, 4, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        SV.jpeg_bytes(np.zeros((4, 4, 3), np.uint8))


# ------------------------------------------------------------------------------------------------ 5. the AVI writer
def _check_avi(avi, payloads, H, W, fps):
    assert avi["lists"] == [b"hdrl", b"movi"]
    assert avi["frames"] == payloads
    n = len(payloads)
    assert avi["avih"] == dict(us_per_frame=int(round(1e6 / fps)), flags=0x10, total_frames=n, streams=1, width=W, height=H)
    sh, sf = avi["strh"], avi["strf"]
    assert (sh["type"], sh["handler"], sh["scale"], sh["rate"], sh["length"]) == (b"vids", b"MJPG", 1, fps, n)
    assert sh["rate"] / sh["scale"] == fps and sh["frame"] == (0, 0, W, H)
    assert (sf["size"], sf["width"], sf["height"], sf["planes"], sf["bits"], sf["compression"]) == (40, W, H, 1, 24, b"MJPG")
    assert len(avi["index"]) == n
    for (cc, flags, off, size), chunk_at, data in zip(avi["index"], avi["frame_offsets"], payloads):
        assert (cc, flags, size) == (b"00dc", 0x10, len(data)) and avi["movi"] + off == chunk_at      # relative to the 'movi' fourcc
        assert chunk_at % 2 == 0


def test_avi_writer_round_trip(tmp_path):
    import surfel_video as SV
    frames = VS.frames(7, 37, 51)
    payloads = [VO.encode(f, 95) for f in frames]
    payloads[2] += b"\0" * (1 - len(payloads[2]) % 2)      # at least one odd and one even length
    payloads[3] += b"\0" * (len(payloads[3]) % 2)
    assert len(payloads[2]) % 2 == 1 and len(payloads[3]) % 2 == 0
    path = str(tmp_path / "v.avi")
    with SV.VideoWriter(path, 37, 51, fps=30, quality=95, ring=2) as vw:
        for p in payloads:
            vw.add_jpeg(p)
    assert vw.frames == 7
    buf = open(path, "rb").read()
    avi = VO.read_avi(buf)      # (asserts that the RIFF and LIST sizes tile the file)
    _check_avi(avi, payloads, 37, 51, 30)
    assert buf.count(b"MJPG") == 2 and buf.count(b"idx1") == 1
    for data in avi["frames"][:2]:
        assert _decode(data).size == (51, 37)
    with pytest.raises(RuntimeError, match="after close"):
        vw.add_jpeg(payloads[0])
    empty = str(tmp_path / "empty.avi")
    SV.VideoWriter(empty, 16, 16).close()
    _check_avi(VO.read_avi(empty), [], 16, 16, 60)
    with pytest.raises(ValueError, match="fps"):
        SV.VideoWriter(str(tmp_path / "bad.avi"), 16, 16, fps=29.97)
    assert not os.path.exists(str(tmp_path / "bad.avi"))


def test_avi_writer_refuses_to_pass_2_gib(tmp_path, monkeypatch):
    import surfel_video as SV
    assert SV.VideoWriter.MAX_BYTES == 2 ** 31 - 1
    payloads = [VO.encode(f, 75) for f in VS.frames(5, 16, 16)]
    # room for the headers, three chunks and their index, not for a fourth
    three = 224 + sum(8 + len(p) + len(p) % 2 for p in payloads[:3]) + 8 + 16 * 3
    monkeypatch.setattr(SV.VideoWriter, "MAX_BYTES", three + 20)
    path = str(tmp_path / "big.avi")
    vw = SV.VideoWriter(path, 16, 16)
    for p in payloads:
        vw.add_jpeg(p)
    with pytest.raises(RuntimeError, match=r"frame 3 .*2 GiB"):
        vw.close()
    assert os.path.getsize(path) == three
    _check_avi(VO.read_avi(path), payloads[:3], 16, 16, 60)      # intact, with the frames before the refusal


def test_avi_writer_surfaces_the_threads_error_at_close(tmp_path):
    import surfel_video as SV
    payloads = [VO.encode(f, 75) for f in VS.frames(4, 16, 16)]
    vw = SV.VideoWriter(str(tmp_path / "e.avi"), 16, 16)
    append = vw._append

    def failing(data):
        if len(vw._index) == 2:
            raise OSError("disk on fire")
        append(data)
    vw._append = failing
    for p in payloads:
        vw.add_jpeg(p)
    with pytest.raises(OSError, match="disk on fire"):
        vw.close()
    assert VO.read_avi(str(tmp_path / "e.avi"))["frames"] == payloads[:2]


# ------------------------------------------------------------------------------------------------ 6. the CLI
def test_mesh_cli_video_flags(capsys):
    import inspect
    import surfel_mesh
    import surfel_path
    with pytest.raises(SystemExit):
        surfel_mesh.main(["--help"])
    text = capsys.readouterr().out
    for flag in ("--video", "--video_only", "--video_quality", "--fps"):
        assert flag in text, flag
    parser = surfel_mesh.build_parser()
    args = parser.parse_args(["-m", "x"])
    assert (args.video, args.video_only, args.video_quality, args.fps) == (False, False, 95, 60)
    assert surfel_mesh.path_video_args(args) == {}      # render_path is called as it always was
    args = parser.parse_args(["-m", "x", "--render_path", "--video", "--video_quality", "80", "--fps", "24"])
    assert surfel_mesh.path_video_args(args) == dict(video=True, video_only=False, video_quality=80, fps=24)
    args = parser.parse_args(["-m", "x", "--render_path", "--video_only"])
    assert surfel_mesh.path_video_args(args) == dict(video=True, video_only=True, video_quality=95, fps=60)
    sig = inspect.signature(surfel_path.render_path).parameters
    assert [(k, sig[k].default) for k in ("video", "video_only", "video_quality", "fps")] == [("video", False), ("video_only", False), ("video_quality", 95), ("fps", 60)]
    assert list(sig)[:10] == ["gaussians", "cameras", "render", "pipe", "background", "out_dir", "n_frames", "vis_normals", "workers", "timings"]
