"""CPU checks of the live viewer (VIEWER.md): the numpy restatement of the image rules against the reference's own bytes
(tests/golden/ref_view.npz, minted by tests/golden/make_golden_view.py), the wire protocol against the reference's recorded byte
streams over socket.socketpair() — no test binds, listens on or connects to an address, and every socket has a timeout — the serve
loop's exit rule with a scripted connection, and the C ABI of include/surfel_view.h."""
import ctypes as C
import json
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import path_oracle as PO
import view_oracle as VO
import view_scenes as VS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_INDETERMINATE = 0.01      # of a frame's pixels


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(REPO, "tests", "golden", "ref_view.npz"))


@pytest.fixture(scope="module")
def SV():
    import surfel_view
    return surfel_view


def _pair(timeout=5.0):
    a, b = socket.socketpair()
    a.settimeout(timeout); b.settimeout(timeout)
    return a, b


def _recv_exactly(sock, n):
    got = b""
    while len(got) < n:
        piece = sock.recv(n - len(got))
        assert piece, "peer closed after %d of %d bytes" % (len(got), n)
        got += piece
    return got


# ------------------------------------------------------------------------------------------------ 1. the image rules
def test_fixture_inputs_are_the_seeded_packages(ref):
    for H, W in VS.GOLDEN_SHAPES:
        pkg = VS.package(H, W)
        for k, v in pkg.items():
            assert np.array_equal(ref["img/%dx%d/%s" % (H, W, k)], v), (H, W, k)


@pytest.mark.parametrize("mode", range(6), ids=VS.RENDER_ITEMS)
@pytest.mark.parametrize("shape", VS.GOLDEN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_reproduces_the_reference_bytes(ref, shape, mode):
    H, W = shape
    name = VS.RENDER_ITEMS[mode]
    pkg = {k: ref["img/%dx%d/%s" % (H, W, k)] for k in ("render", "rend_alpha", "rend_normal", "surf_depth")}
    want = ref["img/%dx%d/%s" % (H, W, name)]
    got, loose = VO.net_image(pkg, mode)
    assert got.shape == want.shape == (H, W, 3) and got.dtype == np.uint8
    differ = (got != want).any(axis=2)
    print("%s %dx%d: %d indeterminate, %d differing pixels of %d" % (name, H, W, int(loose.sum()), int(differ.sum()), H * W))
    assert loose.mean() <= MAX_INDETERMINATE, (name, int(loose.sum()))
    assert not (differ & ~loose).any(), (name, np.argwhere(differ & ~loose)[:5])
    if name in ("RGB", "Normal"):
        assert not loose.any() and not differ.any()
    else:
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 20      # the frame spans the colour map


def test_turbo_header_is_the_reference_table(ref):
    assert ref["turbo"].shape == (256, 3) and ref["turbo"].dtype == np.uint8
    assert np.array_equal(PO.turbo_table(), ref["turbo"])


def test_oracle_rules_for_maps_without_a_range():
    tab = PO.turbo_table()
    const = np.full((3, 4), 2.5, np.float32)
    assert np.array_equal(VO.colour(const)[0], np.broadcast_to(tab[0], (3, 4, 3)))
    m = np.array([[0.0, 1.0, np.nan], [0.5, np.nan, 0.25]], np.float32)
    out, t255 = VO.colour(m)
    assert np.array_equal(out[0, 0], tab[0]) and np.array_equal(out[0, 1], tab[255]) and np.array_equal(out[1, 0], tab[128])      # 127.5 -> even
    assert np.array_equal(out[0, 2], tab[0]) and np.array_equal(out[1, 1], tab[0]) and np.array_equal(out[1, 2], tab[64])        # 63.75
    assert VO.indeterminate(t255)[1, 0] and not VO.indeterminate(t255)[1, 2]
    for special in (np.inf, -np.inf):
        m = np.array([[0.0, 1.0, special]], np.float32)
        assert np.array_equal(VO.colour(m)[0], np.broadcast_to(tab[0], (1, 3, 3)))
    assert np.array_equal(VO.colour(np.full((2, 2), np.nan, np.float32))[0], np.broadcast_to(tab[0], (2, 2, 3)))
    # a single pixel, a single row, a single column: the reference raises there, the rules do not
    for shape in ((1, 1), (1, 5), (7, 1)):
        pkg = VS.package(*shape)
        for mode in range(6):
            assert VO.net_image(pkg, mode)[0].shape == shape + (3,)
    assert float(VO.gradient(np.ones((3, 1, 1), np.float32))[0, 0]) == 0.0
    # the zero padding follows scale and bias: a constant normal map has curvature at its border only
    g = VO.gradient(np.zeros((3, 5, 6), np.float32), 0.5, 0.5)
    assert np.all(g[1:-1, 1:-1] == 0) and np.all(g[0] > 0) and np.all(g[:, -1] > 0)


# ------------------------------------------------------------------------------------------------ 2. the wire protocol
def test_sends_are_the_reference_bytes(ref, SV):
    a, b = _pair()
    conn = SV.Connection(a, device="cpu")
    assert SV.RENDER_ITEMS == VS.RENDER_ITEMS == VO.MODES
    conn.send_items()
    want = ref["wire/items"].tobytes()
    assert _recv_exactly(b, len(want)) == want
    verify, metrics = str(ref["wire/verify"]), json.loads(str(ref["wire/metrics"]))
    conn.send(memoryview(np.ascontiguousarray(ref["wire/image"])), verify, metrics)
    want = ref["wire/frame"].tobytes()
    assert len(want) > 23 * 37 * 3 and _recv_exactly(b, len(want)) == want
    conn.send(None, verify, metrics)
    want = ref["wire/noframe"].tobytes()
    assert _recv_exactly(b, len(want)) == want
    b.settimeout(0.0)
    with pytest.raises(BlockingIOError):      # nothing more was written
        b.recv(1)
    conn.close(); b.close()


def _check_receive(ref, got, k=0):
    import torch
    cam, do_training, keep_alive, scaling_modifier, mode = got
    assert isinstance(cam.world_view_transform, torch.Tensor) and cam.world_view_transform.dtype == torch.float32
    assert np.array_equal(cam.world_view_transform.numpy(), ref["recv/%d/world_view_transform" % k])
    assert np.array_equal(cam.full_proj_transform.numpy(), ref["recv/%d/full_proj_transform" % k])
    # the centre goes through a 4 x 4 fp32 inverse (LAPACK): well conditioned (a rotation and a translation of length 4), so a few ulps
    # of 4 between two BLAS builds
    assert np.allclose(cam.camera_center.numpy(), ref["recv/%d/camera_center" % k], rtol=0, atol=1e-5)
    assert [cam.image_width, cam.image_height] == ref["recv/%d/size" % k].tolist()
    assert np.array_equal(np.array([cam.FoVy, cam.FoVx, cam.znear, cam.zfar, scaling_modifier], np.float64), ref["recv/%d/scalars" % k])
    assert [int(do_training), int(keep_alive), int(mode)] == ref["recv/%d/flags" % k].tolist()
    assert do_training is True and keep_alive is False


def test_receive_is_the_reference_result(ref, SV):
    a, b = _pair()
    conn = SV.Connection(a, device="cpu")
    assert not bool(ref["recv/0/is_none"]) and bool(ref["recv/1/is_none"])
    b.sendall(ref["recv/0/message"].tobytes())
    _check_receive(ref, conn.receive())
    # the flips, said directly: columns 1 and 2 of view_matrix and column 1 of view_projection_matrix change sign
    msg = json.loads(ref["recv/0/message"].tobytes()[4:].decode())
    vm = np.array(msg["view_matrix"], np.float32).reshape(4, 4)
    vp = np.array(msg["view_projection_matrix"], np.float32).reshape(4, 4)
    assert np.array_equal(ref["recv/0/world_view_transform"], vm * np.array([1, -1, -1, 1], np.float32))
    assert np.array_equal(ref["recv/0/full_proj_transform"], vp * np.array([1, -1, 1, 1], np.float32))
    b.sendall(ref["recv/1/message"].tobytes())      # resolution 0
    assert conn.receive() == (None, None, None, None, None)
    for w, h in ((0, 8), (8, 0)):
        b.sendall(VS.frame_message(VS.message(w, h, 0)))
        assert conn.receive() == (None, None, None, None, None)
    conn.close(); b.close()


class _Trickle:
    """a connected socket object whose recv hands out one byte at a time"""

    def __init__(self, sock):
        self.sock, self.calls = sock, 0

    def settimeout(self, t):
        self.sock.settimeout(t)

    def recv(self, n):
        self.calls += 1
        return self.sock.recv(min(n, 1))

    def sendall(self, data):
        self.sock.sendall(data)

    def close(self):
        self.sock.close()


def test_a_message_in_one_byte_pieces_is_read_whole(ref, SV):
    a, b = _pair()
    t = _Trickle(a)
    conn = SV.Connection(t, device="cpu")
    wire = ref["recv/0/message"].tobytes()
    b.sendall(wire)
    _check_receive(ref, conn.receive())
    assert t.calls == len(wire)
    b.close()      # a peer that closes in the middle of a message
    with pytest.raises(ConnectionError, match="closed"):
        conn.receive()
    conn.close()


def test_a_stalled_peer_times_out_and_is_dropped(ref, SV):
    a, b = _pair()
    conn = SV.Connection(a, timeout=0.05, device="cpu")
    b.sendall(ref["recv/0/message"].tobytes()[:40])      # the length and a part of the body, then silence
    with pytest.raises(socket.timeout):
        conn.receive()
    conn.close(); b.close()
    a, b = _pair()
    viewer = SV.Viewer.attached(a, timeout=0.05, device="cpu")
    assert viewer.listener is None and viewer.conn is not None
    want = ref["wire/items"].tobytes()
    assert _recv_exactly(b, len(want)) == want      # the greeting of try_connect
    b.sendall(b"\x10\x00")                          # half a length
    viewer.serve(None, None, None, "", None, 1, 10)      # returns: training goes on
    assert viewer.conn is None and a.fileno() == -1
    viewer.serve(None, None, None, "", None, 2, 10)      # and a Viewer without listener and connection does nothing
    b.close()


# ------------------------------------------------------------------------------------------------ 3. the serve loop and the trainer
class _Script:
    """a connection that plays back receive() results and records what is sent"""

    def __init__(self, steps):
        self.steps, self.sent, self.closed = list(steps), [], False

    def receive(self):
        if not self.steps:
            raise ConnectionError("script exhausted")
        return self.steps.pop(0)

    def send(self, image_bytes, verify, metrics):
        self.sent.append((image_bytes, verify, metrics))

    def close(self):
        self.closed = True


def _serve(SV, monkeypatch, steps, iteration, iterations):
    import surfel_render
    calls = []
    monkeypatch.setattr(surfel_render, "render", lambda cam, g, pipe, bg, sm: calls.append((cam, sm)) or {"pkg": cam})
    monkeypatch.setattr(SV, "net_image", lambda pkg, mode: (pkg["pkg"], mode))
    monkeypatch.setattr(SV.Viewer, "_to_host", lambda self, image: image)
    v = SV.Viewer(listener=False, device="cpu")
    v.conn = conn = _Script(steps)
    v.serve("gaussians", "pipe", "bg", "/capture", lambda: {"#": 7}, iteration, iterations)
    return v, conn, calls


def test_serve_loop_exit_rule(SV, monkeypatch):
    cam = object()
    go, stay = (cam, True, True, 1.0, 0), (cam, False, True, 0.5, 3)
    # train = 0 keeps the loop; train = 1 in the middle of the training leaves it, with the connection kept
    v, conn, calls = _serve(SV, monkeypatch, [stay, stay, go, stay], 5, 10)
    assert v.conn is conn and len(conn.steps) == 1 and len(conn.sent) == 3 and not conn.closed
    assert calls == [(cam, 0.5), (cam, 0.5), (cam, 1.0)]
    assert conn.sent[0] == ((cam, 3), "/capture", {"#": 7}) and conn.sent[2][0] == (cam, 0)
    # at the last iteration keep_alive holds the loop (the script then runs out: the connection is dropped) ...
    v, conn, _ = _serve(SV, monkeypatch, [go, go], 10, 10)
    assert v.conn is None and conn.closed and len(conn.sent) == 2
    # ... and without keep_alive the first train = 1 ends it
    v, conn, _ = _serve(SV, monkeypatch, [(cam, True, False, 1.0, 0), go], 10, 10)
    assert v.conn is conn and len(conn.sent) == 1 and len(conn.steps) == 1
    # an empty image request: nothing is rendered, verify and metrics still go out, and the loop stays
    v, conn, calls = _serve(SV, monkeypatch, [(None, None, None, None, None), go], 5, 10)
    assert calls == [(cam, 1.0)] and conn.sent[0] == (None, "/capture", {"#": 7}) and len(conn.sent) == 2 and v.conn is conn
    # a mode off the list (the renderer or net_image raising) drops the connection and returns
    def boom(pkg, mode):
        raise IndexError(mode)
    v, conn, _ = _serve(SV, monkeypatch, [go], 5, 10)
    monkeypatch.setattr(SV, "net_image", boom)
    v.conn = conn = _Script([(cam, True, True, 1.0, 9), go])
    v.serve("gaussians", "pipe", "bg", "/capture", None, 5, 10)
    assert v.conn is None and conn.closed and conn.sent == []


def test_net_image_names_and_indices(SV):
    assert [SV._mode_name(k) for k in range(6)] == SV.RENDER_ITEMS and SV._mode_name("curvature") == "Curvature"
    with pytest.raises(IndexError):
        SV._mode_name(6)
    with pytest.raises(KeyError):
        SV._mode_name("albedo")
    import torch
    with pytest.raises(RuntimeError, match="HIP device"):
        SV.net_image({"rend_alpha": torch.zeros(1, 4, 4)}, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        SV.net_image({"render": torch.zeros(3, 4, 4)}, 0)


def test_without_port_the_trainer_creates_no_socket(monkeypatch):
    import surfel_trainer as TR

    def refuse(*a, **k):
        raise AssertionError("a socket object was created")
    monkeypatch.setattr(socket, "socket", refuse)
    monkeypatch.setattr(socket, "socketpair", refuse)
    vargs, rest = TR.parse_viewer_args(["-s", "x", "-m", "y"])
    assert vargs.port is None and vargs.ip == "127.0.0.1" and rest == ["-s", "x", "-m", "y"] and TR.make_viewer(vargs) is None
    vargs, rest = TR.parse_viewer_args(["-s", "x", "--port", "6123", "-m", "y", "--ip", "0.0.0.0", "--iterations", "7"])
    assert (vargs.ip, vargs.port) == ("0.0.0.0", 6123) and rest == ["-s", "x", "-m", "y", "--iterations", "7"]
    assert TR.parse_args(rest).iterations == 7      # the training's own flags are what is left
    with pytest.raises(SystemExit):
        TR.parse_viewer_args(["--port", "viewer"])
    with pytest.raises(AssertionError, match="socket object"):      # with --port the listener is what make_viewer builds
        TR.make_viewer(vargs)
    import inspect
    assert inspect.signature(TR.training).parameters["viewer"].default is None


def test_view_cli_flags(SV):
    args = SV.build_parser().parse_args(["-m", "model"])
    assert (args.model_path, args.source_path, args.iteration, args.ip, args.port) == ("model", None, -1, "127.0.0.1", 6009)
    args = SV.build_parser().parse_args(["-m", "m", "-s", "cap", "--iteration", "7000", "--ip", "0.0.0.0", "--port", "6010"])
    assert (args.source_path, args.iteration, args.ip, args.port) == ("cap", 7000, "0.0.0.0", 6010)


# ------------------------------------------------------------------------------------------------ 4. C ABI
def test_view_header_signatures_and_exports(SV):
    import surfel_native as n
    from test_abi_cpu import _prototypes
    lib = n.load()
    protos, mentions = _prototypes("surfel_view.h")
    assert len(protos) == mentions == 2
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES["surfel_view.h"]) == sorted(n.VIEW_EXPORTS)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert C.cast(fn, C.c_void_p).value and fn.restype is C.c_int and ret == "int"
        assert len(fn.argtypes) == len(params), name
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            else:
                assert ctype.endswith("*") and at is (n.Stream if pname == "stream" else n.DevPtr), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where
    out = subprocess.run(["nm", "-D", "--defined-only", n.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(surfel_view_\w+)\b", out))) == sorted(p[0] for p in protos)
    hdr = open(os.path.join(REPO, "include", "surfel_view.h")).read()
    macro = re.search(r"#define SURFEL_VIEW_SCRATCH_BYTES\(H, W\) \((.*)\)\n", hdr).group(1)
    expr = macro.replace("(int64_t)", "")
    for H, W in ((1, 1), (23, 37), (720, 1280), (65536, 65536)):
        assert eval(expr, {"H": H, "W": W}) == SV.scratch_bytes(H, W) == 64 + 4 * H * W
    import importlib.util
    spec = importlib.util.spec_from_file_location("surfel_build_for_view_test", os.path.join(REPO, "2d-gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "view_image.hip" in mod.SOURCES and "-ffp-contract=off" in mod.EXTRA["view_image.hip"]
    assert any(h.endswith("surfel_view.h") for h in mod.HEADERS) and "vis_pixels.h" in mod.HEADERS


def test_view_entries_check_their_arguments_without_a_device():
    import surfel_native as n
    p = C.c_void_p(256)
    big = 1 << 40
    for args in ((0, 4, p, p, p, big), (4, -1, p, p, p, big), (4, 4, None, p, p, big), (4, 4, p, None, p, big), (4, 4, p, p, None, big),
                 (4, 4, C.c_void_p(258), p, p, big), (4, 4, p, p, C.c_void_p(257), big)):
        with pytest.raises(RuntimeError, match=r"\(-1\): view_scalar: bad arguments"):
            n.call(None, "surfel_view_scalar", *args)
    with pytest.raises(RuntimeError, match=r"\(-1\): view_gradient: bad arguments"):
        n.call(None, "surfel_view_gradient", 4, 4, None, 1.0, 0.0, p, p, big)
    with pytest.raises(n.LimitError, match="65536"):
        n.call(None, "surfel_view_scalar", 70000, 4, p, p, p, big)
    with pytest.raises(n.LimitError, match="65536"):
        n.call(None, "surfel_view_gradient", 4, 65537, p, 1.0, 0.0, p, p, big)
    with pytest.raises(RuntimeError, match="SURFEL_VIEW_SCRATCH_BYTES"):
        n.call(None, "surfel_view_scalar", 4, 4, p, p, p, 64 + 4 * 16 - 1)
    with pytest.raises(RuntimeError, match="SURFEL_VIEW_SCRATCH_BYTES"):
        n.call(None, "surfel_view_gradient", 4, 4, p, 0.5, 0.5, p, p, 127)
