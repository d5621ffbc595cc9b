"""CPU tests of the training log (LOG.md): the host framing of include/surfel_log.h against known answers, the Python restatement
(tests/log_oracle.py) and an independent protobuf parser; the file's round trip; the header, the exports and the kernels' resources;
the framing code alone under the address and undefined-behaviour sanitizers.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import socket
import struct
import subprocess
import sys

import numpy as np
import pytest

import log_oracle as LO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_EVENT = bytes.fromhex("09 00 00 00 00 00 00 F8 3F 10 03 2A 0A 0A 08 0A 01 61 15 00 00 80 3E")


@pytest.fixture(scope="module")
def SL():
    import surfel_log
    return surfel_log


def random_records(rng, n):
    rec = np.zeros(n, LO.RECORD)
    rec["iteration"] = rng.choice([0, 1, 127, 128, 16383, 16384, 30000, 2 ** 31 - 1], size=n)
    rec["points"] = rng.integers(0, 2 ** 31 - 1, size=n)
    for f in ("reg_loss", "total_loss", "ema_dist", "ema_normal", "raw_total"):
        bits = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)      # every bit pattern: denormals, infinities, NaNs
        x = bits.view(np.float32)
        rec[f] = np.where(np.isnan(x), bits | np.uint32(0x00400000), bits).astype(np.uint32).view(np.float32)      # (quiet NaNs: a Python float keeps no signalling one)
    rec["seq"] = np.arange(n)
    return rec


# ------------------------------------------------------------------------------------------------ 1. CRC-32C
def test_crc32c_known_answers_and_mask(SL):
    for data, want in ((b"123456789", 0xE3069283), (bytes(32), 0x8A9136AA)):
        assert SL.crc32c(data) == want == LO.crc32c(data)
        assert SL.masked_crc(data) == ((want >> 15 | want << 17) + 0xa282ead8) % 2 ** 32 == LO.mask(want)
    assert SL.crc32c(b"") == 0 == LO.crc32c(b"")
    rng = np.random.default_rng(0)
    for n in (1, 3, 4, 5, 8, 63, 64, 65, 1000):
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert SL.crc32c(data) == LO.crc32c(data), n


# ------------------------------------------------------------------------------------------------ 2. known-answer bytes
def test_event_known_answer_bytes(SL):
    assert SL.event(1.5, 3, [SL.value_scalar("a", 0.25)]) == KNOWN_EVENT
    assert LO.event(1.5, 3, [LO.scalar_value("a", 0.25)]) == KNOWN_EVENT
    # framing: u64 length, masked crc of the length, payload, masked crc of the payload
    rec = SL.frame(KNOWN_EVENT)
    assert rec == LO.frame(KNOWN_EVENT) and len(rec) == 23 + 16
    assert rec[:8] == struct.pack("<Q", 23) and rec[12:35] == KNOWN_EVENT
    assert struct.unpack("<I", rec[8:12])[0] == LO.mask(LO.crc32c(rec[:8])) and struct.unpack("<I", rec[35:])[0] == LO.mask(LO.crc32c(KNOWN_EVENT))
    assert SL.frame(b"") == LO.frame(b"")
    # an image value, every field in ascending number
    png = bytes(range(200))
    assert SL.event(2.0, 300, [SL.value_image("t/depth", 37, 530, png)]) == LO.event(2.0, 300, [LO.image_value("t/depth", 37, 530, png)])
    assert SL.event(7.0, 0, file_version="brain.Event:2") == LO.event(7.0, 0, file_version="brain.Event:2") == \
        b"\x09" + struct.pack("<d", 7.0) + b"\x1a\x0dbrain.Event:2"


def test_c_encoder_agrees_with_the_restatement_on_random_blocks(SL):
    import surfel_native as n
    rng = np.random.default_rng(1)
    for count in (0, 1, 2, 17, 256):
        rec = random_records(rng, count)
        ms, wall = float(np.float32(rng.uniform(0, 5))), float(rng.uniform(1e9, 2e9))
        got = SL.encode_steps(rec, ms, wall)
        assert got == LO.encode_steps(rec, ms, wall), count
        assert len(got) <= n.call(None, "surfel_log_steps_capacity", count)
    # one byte too little: SURFEL_E_LIMIT, and nothing behind the capacity is written
    rec = random_records(rng, 3)
    full = SL.encode_steps(rec, 1.0, 2.0)
    out = C.create_string_buffer(b"\xAB" * (len(full) + 8), len(full) + 8)
    with pytest.raises(n.LimitError, match="log_encode_steps"):
        n.call(None, "surfel_log_encode_steps", rec.ctypes.data_as(C.c_void_p), 3, 1.0, 2.0, out, len(full) - 1)
    assert out.raw[len(full) - 1:] == b"\xAB" * 9
    assert n.call(None, "surfel_log_encode_steps", rec.ctypes.data_as(C.c_void_p), 3, 1.0, 2.0, out, len(full)) == len(full) and out.raw[:len(full)] == full
    rec["iteration"][1] = -5
    with pytest.raises(RuntimeError, match=r"\(-1\): .*negative iteration"):
        n.call(None, "surfel_log_encode_steps", rec.ctypes.data_as(C.c_void_p), 3, 1.0, 2.0, out, len(full))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*log_frame"):
        n.call(None, "surfel_log_frame", b"x", 1, None)


def test_step_tags_are_the_references(SL):
    assert SL.STEP_TAGS == LO.TAGS == ("train_loss_patches/dist_loss", "train_loss_patches/normal_loss", "train_loss_patches/reg_loss",
                                       "train_loss_patches/total_loss", "iter_time", "total_points")
    ev = SL.parse_event(LO.unframe(SL.encode_steps(random_records(np.random.default_rng(2), 1), 0.5, 1.0))[0])
    assert tuple(v["tag"] for v in ev["values"]) == SL.STEP_TAGS


# ------------------------------------------------------------------------------------------------ 3. round trip
def test_file_round_trip_name_first_record_and_corruption(SL, tmp_path):
    rng = np.random.default_rng(3)
    f = SL.EventFile(str(tmp_path / "model"))
    blocks = [(random_records(rng, k), float(np.float32(0.1 * k)), 100.0 + k) for k in (4, 1, 9)]
    for rec, ms, wall in blocks[:2]:
        f.write_steps(rec, ms, wall)
    png = rng.integers(0, 256, size=777, dtype=np.uint8).tobytes()
    f.write_event(SL.event(5.0, 20, [SL.value_image("test_view_a/depth", 3, 5, png), SL.value_scalar("test/loss_viewpoint - psnr", 31.5)]))
    f.write_steps(*blocks[2])
    f.close()
    name = os.path.basename(f.path)
    m = re.fullmatch(r"events\.out\.tfevents\.(\d{10})\.(.+)\.(\d+)\.0", name)
    assert m and m.group(2) == socket.gethostname() and int(m.group(3)) == os.getpid(), name
    assert SL.event_files(str(tmp_path / "model")) == [f.path] and os.path.getsize(f.path) == f.bytes_written
    events = SL.read_events(f.path)
    assert events[0]["file_version"] == "brain.Event:2" and events[0]["step"] == 0 and not events[0]["values"]
    want = []
    for rec, ms, wall in blocks[:2]:
        want += [(r, ms, wall) for r in rec]
    want.append(None)
    want += [(r, blocks[2][1], blocks[2][2]) for r in blocks[2][0]]
    assert len(events) == 1 + len(want)
    for ev, w in zip(events[1:], want):
        if w is None:
            assert ev["step"] == 20 and ev["wall_time"] == 5.0
            assert ev["values"][0] == {"tag": "test_view_a/depth", "image": {"height": 3, "width": 5, "colorspace": 3, "png": png}}
            assert ev["values"][1] == {"tag": "test/loss_viewpoint - psnr", "simple_value": 31.5}
            continue
        r, ms, wall = w
        assert ev["step"] == int(r["iteration"]) and ev["wall_time"] == wall
        got = [(v["tag"], np.float32(v["simple_value"]).tobytes()) for v in ev["values"]]
        assert got == [(t, np.float32(x).tobytes()) for t, x in LO.step_values(r, ms)]      # bit for bit, NaN payloads included
    # the file is what the restatement writes after the first record
    raw = open(f.path, "rb").read()
    first = len(LO.frame(LO.event(events[0]["wall_time"], 0, file_version="brain.Event:2")))
    assert raw[first:] == b"".join([LO.encode_steps(*blocks[0]), LO.encode_steps(*blocks[1]),
                                    LO.frame(LO.event(5.0, 20, [LO.image_value("test_view_a/depth", 3, 5, png), LO.scalar_value("test/loss_viewpoint - psnr", 31.5)])),
                                    LO.encode_steps(*blocks[2])])
    # a flipped byte is reported with the index of its record: in a payload, in a length, and a truncated file
    offsets = [0]
    for p in LO.unframe(raw):
        offsets.append(offsets[-1] + len(p) + 16)
    for k, delta in ((0, 14), (3, 30), (6, 3), (len(offsets) - 2, 12)):
        bad = bytearray(raw)
        bad[offsets[k] + delta] ^= 0x10
        path = str(tmp_path / ("bad_%d" % k))
        open(path, "wb").write(bad)
        with pytest.raises(SL.CorruptRecord, match="record %d:" % k) as e:
            SL.read_events(path)
        assert e.value.index == k
    open(str(tmp_path / "short"), "wb").write(raw[:offsets[4] + 20])
    with pytest.raises(SL.CorruptRecord, match="record 4: truncated"):
        SL.read_events(str(tmp_path / "short"))


def test_cli_prints_csv_and_writes_images(SL, tmp_path, capsys):
    f = SL.EventFile(str(tmp_path))
    rec = np.zeros(2, LO.RECORD)
    rec["iteration"], rec["points"], rec["reg_loss"] = [1, 2], [10, 11], [0.5, 0.25]
    f.write_steps(rec, 2.0, 1.0)
    f.write_event(SL.event(1.0, 2, [SL.value_image("test_view_x/render", 1, 1, b"\x89PNG-bytes")]))
    f.close()
    assert SL.main([str(tmp_path), "--csv", "--images", str(tmp_path / "img")]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == "step," + ",".join(sorted(SL.STEP_TAGS))
    assert lines[1].split(",")[:3] == ["1", "2", "10"] and lines[2].split(",")[:3] == ["2", "2", "11"]
    assert open(str(tmp_path / "img" / "000002" / "test_view_x__render.png"), "rb").read() == b"\x89PNG-bytes"
    assert SL.main([str(tmp_path / "img")]) == 1      # a folder without event files


# ------------------------------------------------------------------------------------------------ 4. an independent parser
def test_protobuf_parses_what_the_encoder_wrote(SL):
    pytest.importorskip("google.protobuf")
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    T = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="surfel_log_test.proto", package="slt", syntax="proto3")

    def message(name, fields):
        m = fd.message_type.add(name=name)
        for fname, number, ftype, label, type_name in fields:
            m.field.add(name=fname, number=number, type=ftype, label=label, type_name=type_name)
    one, many = T.LABEL_OPTIONAL, T.LABEL_REPEATED
    message("Image", [("height", 1, T.TYPE_INT32, one, None), ("width", 2, T.TYPE_INT32, one, None), ("colorspace", 3, T.TYPE_INT32, one, None),
                      ("encoded_image_string", 4, T.TYPE_BYTES, one, None)])
    message("Value", [("tag", 1, T.TYPE_STRING, one, None), ("simple_value", 2, T.TYPE_FLOAT, one, None), ("image", 4, T.TYPE_MESSAGE, one, ".slt.Image")])
    message("Summary", [("value", 1, T.TYPE_MESSAGE, many, ".slt.Value")])
    message("Event", [("wall_time", 1, T.TYPE_DOUBLE, one, None), ("step", 2, T.TYPE_INT64, one, None), ("file_version", 3, T.TYPE_STRING, one, None),
                      ("summary", 5, T.TYPE_MESSAGE, one, ".slt.Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    Event = message_factory.GetMessageClass(pool.FindMessageTypeByName("slt.Event"))
    rng = np.random.default_rng(4)
    rec = random_records(rng, 40)
    for f in ("reg_loss", "total_loss", "ema_dist", "ema_normal"):      # (NaN != NaN: compare numbers here, bits in the round trip)
        rec[f] = rng.normal(size=40).astype(np.float32)
    payloads = LO.unframe(SL.encode_steps(rec, 0.75, 123.5))
    assert len(payloads) == 40
    for r, p in zip(rec, payloads):
        ev = Event()
        ev.ParseFromString(p)
        assert ev.wall_time == 123.5 and ev.step == int(r["iteration"]) and ev.file_version == ""
        assert [(v.tag, v.simple_value) for v in ev.summary.value] == [(t, float(x)) for t, x in LO.step_values(r, 0.75)]
        assert ev.SerializeToString() == p      # protobuf's own serialiser writes the same bytes: ascending fields, zero step omitted
    png = rng.integers(0, 256, size=300, dtype=np.uint8).tobytes()
    ev = Event()
    ev.ParseFromString(SL.event(9.0, 7000, [SL.value_image("test_view_r_3/rend_dist", 545, 980, png), SL.value_scalar("test/loss_viewpoint - l1_loss", 0.125)]))
    a, b = ev.summary.value
    assert (a.tag, a.image.height, a.image.width, a.image.colorspace, a.image.encoded_image_string) == ("test_view_r_3/rend_dist", 545, 980, 3, png)
    assert (b.tag, b.simple_value, ev.step, ev.wall_time) == ("test/loss_viewpoint - l1_loss", 0.125, 7000, 9.0)
    ev = Event()
    ev.ParseFromString(SL.event(1.0, 0, file_version="brain.Event:2"))
    assert ev.file_version == "brain.Event:2" and ev.step == 0 and len(ev.summary.value) == 0


# ------------------------------------------------------------------------------------------------ 5. header, exports, resources
def test_log_header_signatures_and_exports():
    """include/surfel_log.h <-> SIGNATURES["surfel_log.h"] <-> LOG_EXPORTS <-> the library's exports, both ways"""
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_log.h")
    assert len(protos) == mentions == 6
    assert [p[0] for p in protos] == ["surfel_log_append", "surfel_log_panel", "surfel_log_crc32c", "surfel_log_frame", "surfel_log_steps_capacity",
                                      "surfel_log_encode_steps"]
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_log.h"]) == sorted(n.LOG_EXPORTS)
    others = [name for h, group in n.SIGNATURES.items() if h != "surfel_log.h" for name in group]
    assert not set(n.LOG_EXPORTS) & set(others)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    returns = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    host = {"surfel_log_crc32c", "surfel_log_frame", "surfel_log_steps_capacity", "surfel_log_encode_steps"}
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert C.cast(fn, C.c_void_p).value and fn.restype is returns[ret], (name, ret)
        assert len(fn.argtypes) == len(params), name
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            elif name in host:
                assert ctype.endswith("*") and at is C.c_void_p and pname != "stream", where      # host pointers, no stream
            else:
                assert ctype.endswith("*") and at is (n.Stream if pname == "stream" else n.DevPtr), where
        assert (name in host) == (params[-1][1] != "stream"), name
    hdr = open(os.path.join(REPO, "include", "surfel_log.h")).read()
    import surfel_log as SL
    for macro, value in (("SURFEL_LOG_STATE_BYTES", SL.STATE_BYTES), ("SURFEL_LOG_RECORD_BYTES", SL.RECORD_BYTES),
                         ("SURFEL_LOG_PANEL_SCRATCH_BYTES", SL.PANEL_SCRATCH_BYTES)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value
    for mode, k in SL.MODES.items():
        assert int(re.search(r"#define SURFEL_LOG_PANEL_%s (\d+)" % mode.upper(), hdr).group(1)) == k
    assert SL.RECORD_DTYPE == LO.RECORD and SL.RECORD_DTYPE.itemsize == SL.RECORD_BYTES
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_log_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "train_log.hip" in mod.SOURCES and "log_events.cpp" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["train_log.hip"]
    assert any(h.endswith("surfel_log.h") for h in mod.HEADERS) and "log_jet_table.h" in mod.HEADERS


def test_entries_refuse_bad_arguments_before_any_launch():
    import surfel_native as n
    lib = n.load()
    fake, odd = C.c_void_p(4096), C.c_void_p(4098)      # never dereferenced: every call below is refused
    E_INVALID = lib.surfel_log_append(None, fake, 8, 1, 1, fake, 0.0, 0.0, None)
    assert E_INVALID == -1 and "log_append" in n.last_error()
    for args in ((fake, None, 8, fake), (fake, fake, 0, fake), (fake, fake, 8, None), (C.c_void_p(4100), fake, 8, fake), (fake, odd, 8, fake), (fake, fake, 8, odd)):
        assert lib.surfel_log_append(args[0], args[1], args[2], 1, 1, args[3], 0.0, 0.0, None) == E_INVALID, args
    ok = dict(mode=0, H=4, W=4, planes=fake, dst=fake, scratch=fake, nbytes=64)
    for kw in (dict(mode=-1), dict(mode=5), dict(H=0), dict(W=-1), dict(planes=None), dict(dst=None), dict(scratch=None), dict(planes=odd), dict(scratch=odd),
               dict(nbytes=63)):
        a = dict(ok, **kw)
        assert lib.surfel_log_panel(a["mode"], a["H"], a["W"], a["planes"], a["dst"], a["scratch"], a["nbytes"], None) == E_INVALID, kw
        assert "log_panel" in n.last_error()
    for kw in (dict(H=65537), dict(W=65537)):
        a = dict(ok, **kw)
        assert lib.surfel_log_panel(a["mode"], a["H"], a["W"], a["planes"], a["dst"], a["scratch"], a["nbytes"], None) == n.E_LIMIT, kw
    import torch
    import surfel_log as SL
    with pytest.raises(RuntimeError, match="HIP device"):      # no host fallback
        SL.panel("rgb", torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        SL.append(None, None, 1, 1, torch.zeros(6), 0.0, 0.0)


def test_jet_table_is_generated_from_matplotlib():
    pytest.importorskip("matplotlib")
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import gen_jet_table as G
    assert open(G.HEADER).read() == G.render_header()
    tab = G.parse_header()
    assert np.array_equal(tab, G.table()) and tab[0].tolist() == [0, 0, 127] and tab[255].tolist() == [127, 0, 0]


def test_log_kernels_use_no_scratch_and_spill_nothing():
    """the append runs behind every step and the panel kernels are memory-bound streams: none may touch the private segment"""
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
    import build as B
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + B.EXTRA["train_log.hip"] +
                          ["-S", "--cuda-device-only", "-c", os.path.join(B.CSRC, "train_log.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    seen = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", text, re.S):
        md = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, m.group(2)).group(1)) for k in ("next_free_vgpr", "group_segment_fixed_size", "private_segment_fixed_size")}
        seen[m.group(1)] = md
        assert md["private_segment_fixed_size"] == 0, (m.group(1), md)
        assert md["next_free_vgpr"] <= 64 and md["group_segment_fixed_size"] <= 2048, (m.group(1), md)      # 8 waves / SIMD; the table and the partials
    names = " ".join(seen)
    for k in ("log_append_kernel", "log_reset_kernel", "log_minmax_kernel", "log_quantize_kernel", "log_colour_kernel"):
        assert k in names, (k, names)
    assert len(seen) == 8      # append, reset, minmax, three quantisers, two colour kernels
    spills = [int(x) for x in re.findall(r"\.(?:sgpr|vgpr)_spill_count:\s*(\d+)", text)]
    assert len(spills) == 2 * len(seen) and not any(spills)
    # the fp64 running mean keeps its two products and its sum: no fused multiply-add in the append kernel
    body = re.search(r"^(_ZN6surfel17log_append_kernel\w+):.*?^\.Lfunc_end", text, re.S | re.M).group(0)
    assert "v_mul_f64" in body and "v_add_f64" in body and "v_fma_f64" not in body and "v_fmac_f64" not in body


def test_log_is_opt_in():
    """without --tensorboard no writer is made; Trainer takes logger=None by default"""
    import inspect
    import surfel_trainer as TR
    vargs, rest = TR.parse_viewer_args(["-s", "x", "-m", "y"])
    assert vargs.tensorboard is False and TR.make_logger(vargs, "y") is None and rest == ["-s", "x", "-m", "y"]
    vargs, rest = TR.parse_viewer_args(["-s", "x", "--tensorboard", "-m", "y", "--iterations", "7"])
    assert vargs.tensorboard is True and rest == ["-s", "x", "-m", "y", "--iterations", "7"] and TR.parse_args(rest).iterations == 7
    assert inspect.signature(TR.Trainer.__init__).parameters["logger"].default is None


# ------------------------------------------------------------------------------------------------ 6. the framing code under sanitizers
SANITIZE_MAIN = r"""
// every call gets heap buffers of exactly the size the header promises, so a byte past either end is the sanitizer's to report
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "surfel_log.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

int main() {
    const int64_t lengths[] = {0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 127, 128, 129, 4095, 4096, 4097, 100000};
    for (int64_t n : lengths) {
        uint8_t* p = (uint8_t*)malloc(n ? n : 1);
        for (int64_t i = 0; i < n; i++) p[i] = (uint8_t)rnd();
        uint8_t* out = (uint8_t*)malloc(n + 16);
        if (surfel_log_frame(n ? p : nullptr, n, out) != n + 16) return 1;
        uint64_t len; memcpy(&len, out, 8);
        if ((int64_t)len != n || (n && memcmp(out + 12, p, n))) return 2;
        const uint32_t c = surfel_log_crc32c(p, n);
        uint32_t stored; memcpy(&stored, out + 12 + n, 4);
        if (stored != (uint32_t)(((c >> 15) | (c << 17)) + 0xa282ead8u)) return 3;
        if (n) { uint8_t* q = (uint8_t*)malloc(n + 1); memcpy(q + 1, p, n); if (surfel_log_crc32c(q + 1, n) != c) return 4; free(q); }      // odd address
        free(out); free(p);
    }
    if (surfel_log_frame(nullptr, 4, nullptr) >= 0 || surfel_log_frame(nullptr, -1, nullptr) >= 0) return 5;
    const int64_t counts[] = {0, 1, 2, 5, 256, 1000};
    const int32_t iters[] = {0, 1, 127, 128, 16383, 16384, 2097151, 2097152, 268435455, 268435456, 2147483647};
    for (int64_t n : counts) {
        uint8_t* rec = (uint8_t*)malloc(n * SURFEL_LOG_RECORD_BYTES + 1) + 1;      // an odd address: the encoder copies each record out
        for (int64_t i = 0; i < n * SURFEL_LOG_RECORD_BYTES; i++) rec[i] = (uint8_t)rnd();
        for (int64_t i = 0; i < n; i++) { const int32_t it = iters[rnd() % 11]; memcpy(rec + i * SURFEL_LOG_RECORD_BYTES, &it, 4); }
        const int64_t cap = surfel_log_steps_capacity(n);
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        const int64_t used = surfel_log_encode_steps(rec, n, 0.5f, 1.0e9, out, cap);
        if (used < 0 || used > cap || (n && used < n * 200)) return 6;
        if (used) {      // a buffer of exactly the bytes needed works; one byte less is refused without a write behind it
            uint8_t* tight = (uint8_t*)malloc(used);
            if (surfel_log_encode_steps(rec, n, 0.5f, 1.0e9, tight, used) != used || memcmp(tight, out, used)) return 7;
            free(tight);
            tight = (uint8_t*)malloc(used - 1);
            if (surfel_log_encode_steps(rec, n, 0.5f, 1.0e9, tight, used - 1) != -4) return 8;
            free(tight);
        }
        int64_t p = 0, records = 0;      // walk the records back
        while (p < used) { uint64_t len; memcpy(&len, out + p, 8); p += 16 + (int64_t)len; records++; }
        if (p != used || records != n) return 9;
        free(out); free(rec - 1);
    }
    const int32_t neg = -1;
    uint8_t one[SURFEL_LOG_RECORD_BYTES] = {0}; memcpy(one, &neg, 4);
    uint8_t sink[512];
    if (surfel_log_encode_steps(one, 1, 0.f, 0.0, sink, 512) != -1 || surfel_log_encode_steps(nullptr, 1, 0.f, 0.0, sink, 512) != -1) return 10;
    puts("log_events ok");
    return 0;
}
"""


def test_framing_code_alone_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/log_events.cpp compiles on its own (-DSURFEL_LOG_STANDALONE); with a small main it runs under -fsanitize=address,undefined on
    random and edge-length inputs.  A host program with its own main: no device; it runs in the environment the test has, and the probe
    below skips the test where the sanitizer's runtime cannot start in it."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link or start the sanitizer runtime")
    main = tmp_path / "main.cpp"
    main.write_text(SANITIZE_MAIN)
    exe = str(tmp_path / "log_events_san")
    subprocess.check_call([cxx] + flags + ["-Wall", "-Werror", "-DSURFEL_LOG_STANDALONE", "-I", os.path.join(REPO, "include"), str(main),
                                           os.path.join(REPO, "2d-gaussian-splatting_amd", "csrc", "log_events.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "log_events ok" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_ring_inputs_hold_the_cases_they_claim():
    """the inputs of the GPU ring test (log_oracle.ring_steps): a step with both lambdas 0, an fp32-denormal product, and steps at which
    a contracted running mean, fused either way, would leave other fp64 bits in the state"""
    steps = LO.ring_steps()
    assert len(steps) == 19 and steps[3][3] == steps[3][4] == 0.0
    prod = np.float32(steps[5][4]) * steps[5][2][3]
    assert 0 < prod < np.finfo(np.float32).tiny
    ema, differ = 0.0, [0, 0]
    for _, _, s, _, lam_d in steps:
        v = float(np.float32(lam_d) * s[3])
        unfused = 0.4 * v + 0.6 * ema
        for form, fused in enumerate(LO.fused_ema(ema, v)):
            differ[form] += fused != unfused
        ema = unfused
    assert min(differ) >= 1, differ


def test_oracle_records_and_panels_on_small_cases():
    s = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    rec = LO.records([(1, 10, s, 0.05, 100.0), (2, 11, s, 0.0, 100.0)])
    d1 = 0.4 * float(np.float32(100.0) * np.float32(0.4))
    assert rec["ema_dist"][0] == np.float32(d1) and rec["ema_dist"][1] == np.float32(d1 + 0.6 * d1) and rec["ema_normal"][1] == np.float32(0.6 * (0.4 * float(np.float32(0.05) * np.float32(0.3))))
    assert rec["reg_loss"][0] == np.float32(0.1) and rec["total_loss"][0] == np.float32(0.5) and rec["raw_total"][0] == np.float32(0.6)
    assert rec["seq"].tolist() == [0, 1] and rec["points"].tolist() == [10, 11]
    x = np.array([[[-1.0, 0.0, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf, 0.999, 0.25]]], np.float32)
    assert LO.panel("gray", x)[0, :, 0].tolist() == [0, 0, 127, 255, 255, 0, 255, 0, 254, 63]
    assert LO.panel("normal", np.repeat(x, 3, 0))[0, :, 2].tolist() == [0, 127, 191, 255, 255, 0, 255, 0, 254, 159]
    turbo, jet = LO._table("turbo"), LO._table("jet")
    d = np.array([[[0.0, 1.0, 2.0, 4.0, np.nan, -3.0]]], np.float32)
    assert np.array_equal(LO.panel("turbo_max", d)[0], turbo[[0, 64, 128, 255, 0, 0]])
    assert np.array_equal(LO.panel("jet_minmax", d)[0], jet[[(3 * 256) // 7, (4 * 256) // 7, (5 * 256) // 7, 255, 0, 0]])
    for flat in (np.zeros((1, 2, 2), np.float32), np.full((1, 2, 2), np.nan, np.float32), np.array([[[1.0, np.inf]]], np.float32), -np.ones((1, 1, 1), np.float32)):
        assert np.array_equal(LO.panel("turbo_max", flat), np.broadcast_to(turbo[0], flat.shape[1:] + (3,)))
    for flat in (np.full((1, 2, 2), 3.5, np.float32), np.full((1, 1, 2), np.nan, np.float32), np.array([[[1.0, -np.inf]]], np.float32)):
        assert np.array_equal(LO.panel("jet_minmax", flat), np.broadcast_to(jet[0], flat.shape[1:] + (3,)))
