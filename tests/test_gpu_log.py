"""GPU tests of the training log (LOG.md): the step ring and the panels of include/surfel_log.h against tests/log_oracle.py, bit for bit
and byte for byte; guard pages around every buffer; a 40-step training run whose event file is read back; and the proof that a Trainer
without a logger makes the calls it always made."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import log_oracle as LO

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def SL(torch):
    import surfel_log
    return surfel_log


# ------------------------------------------------------------------------------------------------ 1. the ring
def test_ring_records_are_the_oracles_bit_for_bit(torch, SL):
    steps = LO.ring_steps()
    capacity, block = 8, 4
    state = torch.zeros(SL.STATE_BYTES, dtype=torch.uint8, device="cuda")
    ring = torch.zeros(capacity * SL.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    blocks, done = [], 0
    for k, (it, points, s, lam_n, lam_d) in enumerate(steps):
        SL.append(state, ring, it, points, torch.from_numpy(s).cuda(), lam_n, lam_d)
        if (k + 1) % block == 0 or k + 1 == len(steps):      # a block boundary, or the final partial block: copy it out, stream-ordered
            first = (done % capacity) * SL.RECORD_BYTES
            blocks.append(ring[first:first + (k + 1 - done) * SL.RECORD_BYTES].clone())
            done = k + 1
    got = np.frombuffer(torch.cat(blocks).cpu().numpy().tobytes(), LO.RECORD)
    want, (ema_dist, ema_normal, count) = LO.records(steps, with_state=True)
    assert len(got) == 19 and got["seq"].tolist() == list(range(19)) and got["iteration"].tolist() == list(range(1, 20))      # none missing or doubled
    for k in range(19):
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    st = state.cpu().numpy()
    assert st[:16].view(np.float64).tolist() == [ema_dist, ema_normal] and st[16:].view(np.int64).tolist() == [count, 0]      # the fp64 means, unfused
    # the ring itself: two wraps, the last three slots' predecessors still there
    final = np.frombuffer(ring.cpu().numpy().tobytes(), LO.RECORD)
    for slot in range(capacity):
        k = max(j for j in range(19) if j % capacity == slot)
        assert final[slot].tobytes() == want[k].tobytes(), slot
    before = LO.records(steps[:3], with_state=True)[1]      # the step with both lambdas 0 only decays the means
    assert want["ema_normal"][3] == np.float32(0.6 * before[1]) and want["ema_dist"][3] == np.float32(0.6 * before[0]) and want["ema_dist"][5] != 0


# ------------------------------------------------------------------------------------------------ 2. the panels
def panel_inputs(Cn, H, W):
    rng = np.random.default_rng(H * 1000 + W + Cn)
    x = rng.normal(0.5, 0.35, size=(Cn, H, W)).astype(np.float32)
    special = rng.uniform(0.0, 2.0, size=(Cn, H, W)).astype(np.float32)
    flat = special.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        flat[(k * 7919 + 1) % flat.size] = v      # (at 1 x 1 the single pixel ends up NaN)
    finite_special = special.copy()
    finite_special[~np.isfinite(finite_special)] = np.nan      # NaN pixels among finite ones: the extrema skip them
    return {"random": x, "constant": np.full((Cn, H, W), 0.37, np.float32), "zero": np.zeros((Cn, H, W), np.float32),
            "outside": (x * 3.0 - 1.0).astype(np.float32), "negative": (-np.abs(x) - 0.1).astype(np.float32), "nan-inf": special, "nan": finite_special}


def order_value(key):
    if key == 0xffffffff:
        return np.float32(np.nan)
    return np.array([key ^ 0x80000000 if key >> 31 else ~key & 0xffffffff], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("H, W", [(1, 1), (16, 16), (37, 53), (64, 65)])
def test_panels_are_the_oracles_byte_for_byte(torch, SL, H, W):
    for mode in SL.MODES:
        Cn = 3 if mode in ("rgb", "normal") else 1
        for name, x in panel_inputs(Cn, H, W).items():
            d = torch.from_numpy(x).cuda()
            want = LO.panel(mode, x)
            runs = []
            for _ in range(2):
                scratch = torch.full((SL.PANEL_SCRATCH_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
                out = SL.panel(mode, d, scratch=scratch)
                assert out.shape == (H, W, 3) and out.dtype == torch.uint8
                runs.append((out.cpu().numpy(), scratch[:8].cpu().numpy().view(np.uint32).tolist()))
            assert np.array_equal(runs[0][0], want), (mode, name, H, W, np.argwhere(runs[0][0] != want)[:4].tolist())
            assert np.array_equal(runs[1][0], want) and runs[0][1] == runs[1][1], (mode, name, "second run")
            if mode in ("turbo_max", "jet_minmax"):      # the extrema themselves, identical over the two runs
                lo, hi = LO.extrema(x[0])
                got_lo, got_hi = order_value(runs[0][1][0]), order_value(runs[0][1][1])
                if np.isnan(hi):
                    assert runs[0][1] == [0xffffffff, 0], (mode, name)      # no pixel had a value: the identities are left
                else:
                    assert got_lo.tobytes() == np.float32(lo).tobytes() and got_hi.tobytes() == np.float32(hi).tobytes(), (mode, name, got_lo, got_hi, lo, hi)
    # a [H, W] plane is one plane; the wrong plane count is refused
    assert np.array_equal(SL.panel("gray", torch.from_numpy(panel_inputs(1, H, W)["random"][0]).cuda()).cpu().numpy(), LO.panel("gray", panel_inputs(1, H, W)["random"]))
    with pytest.raises(ValueError, match="takes"):
        SL.panel("rgb", torch.zeros(1, H, W, device="cuda"))


def test_panel_writes_every_destination_alignment_and_nothing_else(torch, SL):
    x = panel_inputs(3, 5, 7)["random"]
    want = LO.panel("normal", x).reshape(-1)
    for off in range(4):
        buf = torch.full((want.size + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        SL.panel("normal", torch.from_numpy(x).cuda(), out=buf[off:off + want.size])
        got = buf.cpu().numpy()
        assert np.array_equal(got[off:off + want.size], want) and (got[:off] == 0xAB).all() and (got[off + want.size:] == 0xAB).all(), off


# ------------------------------------------------------------------------------------------------ 3. guard pages
def test_guard_pages_around_every_buffer():
    p = subprocess.run([sys.executable, os.path.join(HERE, "log_guard_run.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "log_guard_run: rc %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("ok ") == 17, p.stdout


# ------------------------------------------------------------------------------------------------ 4. end to end
def make_run(torch, logger=None):
    """a synthetic capture (orbit cameras 64 x 64, 2 000 surfels), both regularisers switching on inside 40 steps; four views to train on,
    two held out"""
    import surfel_trainer as TR
    dev = torch.device("cuda:0")
    gt = TR.synthetic_object(2000, dev, seed=0, px_scale=0.08)
    cams = TR.capture_views(gt, TR.orbit_cameras(6, 64, 64, device=dev), torch.zeros(3, device=dev))
    model = TR.synthetic_object(2000, dev, seed=1, px_scale=0.08)
    model.spatial_lr_scale = 1.0
    opt = TR.optimization_params(dist_from_iter=10, normal_from_iter=25, lambda_dist=10.0)
    return TR.Trainer(model, cams[:4], opt, TR.pipeline_params(depth_ratio=1.0), logger=logger), cams[4:]


def step_events(SL, events):
    return [ev for ev in events if [v["tag"] for v in ev["values"]] == list(SL.STEP_TAGS)]


def check_steps(SL, events, steps, blocks):
    """the step Events against the oracle applied to the recorded scalars; iter_time: one positive value per flushed block"""
    want = LO.records(steps)
    evs = step_events(SL, events)
    assert [ev["step"] for ev in evs] == [s[0] for s in steps]
    k = 0
    for ev, rec in zip(evs, want):
        vals = {v["tag"]: np.float32(v["simple_value"]) for v in ev["values"]}
        for tag, x in LO.step_values(rec, 0.0):
            if tag != "iter_time":
                assert vals[tag].tobytes() == np.float32(x).tobytes(), (ev["step"], tag, vals[tag], x)
        assert np.isfinite(vals["iter_time"]) and vals["iter_time"] > 0
    times = [np.float32(next(v["simple_value"] for v in ev["values"] if v["tag"] == "iter_time")) for ev in evs]
    for count in blocks:
        assert len(set(times[k:k + count])) == 1, (k, count, times[k:k + count])
        k += count
    assert k == len(evs)


def test_training_run_leaves_the_log_the_oracle_predicts(torch, SL, tmp_path):
    from PIL import Image
    from surfel_render import render
    writer = SL.EventWriter(str(tmp_path / "run"), block=16)
    tr, test_cams = make_run(torch, writer)
    opt = tr.opt
    steps, panels = [], {}
    for _ in range(40):
        tr.step()
        it = tr.iteration
        s = tr.last["scalars"].float().cpu().numpy().copy()      # (the test may wait; the trainer does not)
        steps.append((it, int(tr.last["points"]), s, opt.lambda_normal if it > opt.normal_from_iter else 0.0, opt.lambda_dist if it > opt.dist_from_iter else 0.0))
        if it == 20:
            ps, l1 = SL.report(tr, writer, "test", test_cams, first=True)
            with torch.no_grad():
                for cam in test_cams:      # the same maps through surfel_log_panel: what every PNG must decode to
                    pkg = render(cam, tr.model, tr.pipe, tr.background)
                    for label, key, mode in SL.PANELS:
                        panels["test_view_%s/%s" % (cam.image_name, label)] = SL.panel(mode, pkg[key]).cpu().numpy()
                    panels["test_view_%s/ground_truth" % cam.image_name] = SL.panel("rgb", cam.original_image).cpu().numpy()
    writer.close()
    assert writer.steps == 40 and writer.stalls >= 0 and os.path.getsize(writer.path) == writer.bytes_written
    assert any(s[3] > 0 for s in steps) and any(s[4] > 0 for s in steps) and steps[0][3] == steps[0][4] == 0.0      # both switch-on points inside the run
    events = SL.read_events(writer.path)
    assert events[0]["file_version"] == "brain.Event:2"
    check_steps(SL, events, steps, blocks=(16, 4, 16, 4))      # the report at step 20 flushes the partial block in front of it
    # order in the file: steps 1..20, the report's Events (step 20), steps 21..40
    order = [ev["step"] for ev in events[1:]]
    assert order == list(range(1, 21)) + [20, 20, 20] + list(range(21, 41))
    images = {}
    for ev in events:
        for v in ev["values"]:
            if "image" in v:
                assert ev["step"] == 20 and v["tag"] not in images
                images[v["tag"]] = v["image"]
    assert sorted(images) == sorted(panels) and len(images) == 2 * 7
    assert sum(tag.endswith("/ground_truth") for tag in images) == 2      # once per view
    for tag, img in images.items():
        assert (img["height"], img["width"], img["colorspace"]) == (64, 64, 3)
        got = np.asarray(Image.open(io.BytesIO(img["png"])).convert("RGB"))
        assert np.array_equal(got, panels[tag]), tag
    assert len({panels[t].tobytes() for t in panels}) >= 10      # the panels are pictures, not blanks
    scal = {v["tag"]: v["simple_value"] for ev in events for v in ev["values"] if v["tag"].startswith("test/")}
    assert scal == {"test/loss_viewpoint - l1_loss": float(np.float32(l1)), "test/loss_viewpoint - psnr": float(np.float32(ps))}
    # the same records through one pinned slot and blocks of two: the training thread has to wait for the writer now and then
    second = SL.EventWriter(str(tmp_path / "tight"), block=2, slots=1)
    for it, points, s, lam_n, lam_d in steps:
        second.append(it, points, torch.from_numpy(s).cuda(), lam_n, lam_d)
    second.close()
    assert second.stalls >= 0 and second.steps == 40
    print("stalls with one pinned slot and blocks of two: %d" % second.stalls)
    check_steps(SL, SL.read_events(second.path), steps, blocks=(2,) * 20)
    with pytest.raises(RuntimeError, match="after close"):
        second.append(41, 1, torch.zeros(6, device="cuda"), 0.0, 0.0)


def test_accumulate_step_appends_once_per_step(torch, SL, tmp_path):
    """the third step mode one GPU can take (views_per_step > 1: the gradients of several views per optimiser step): one append per step
    on the training thread, the records those of the oracle applied to tr.last["scalars"]; both lambdas switch on inside the run"""
    import surfel_native as n
    writer = SL.EventWriter(str(tmp_path), block=4)
    tr, _ = make_run(torch, writer)
    tr.views_per_step = 2
    tr.opt.dist_from_iter, tr.opt.normal_from_iter = 2, 4
    opt, steps, names = tr.opt, [], []
    lib = n.load()
    n._lib = Recorder(lib, names)
    try:
        for _ in range(6):
            tr.step()
            it = tr.iteration
            steps.append((it, int(tr.last["points"]), tr.last["scalars"].float().cpu().numpy().copy(),
                          opt.lambda_normal if it > opt.normal_from_iter else 0.0, opt.lambda_dist if it > opt.dist_from_iter else 0.0))
    finally:
        n._lib = lib
    writer.close()
    assert names.count("surfel_log_append") == 6 and names.count("surfel_rasterize_forward") >= 12 and names[-1] == "surfel_log_append"
    assert steps[-1][3] > 0 and steps[-1][4] > 0 and steps[0][3] == steps[0][4] == 0.0
    check_steps(SL, SL.read_events(writer.path), steps, blocks=(4, 2))


def test_writer_surfaces_the_writer_threads_error(torch, SL, tmp_path):
    w = SL.EventWriter(str(tmp_path), block=2, slots=1)
    w._file.write = lambda data: (_ for _ in ()).throw(OSError("disk full"))
    for k in range(6):      # the failed blocks still release their slot: nobody waits for ever
        w.append(k + 1, 1, torch.zeros(6, device="cuda"), 0.0, 0.0)
    with pytest.raises(OSError, match="disk full"):
        w.close()


# ------------------------------------------------------------------------------------------------ 5. training is untouched
class Recorder:
    """a proxy in the library's place (surfel_native.call looks every function up on the loaded library): the names of the calls the
    training thread makes, in order (the writer thread's host calls into the framing code are its own business)"""

    def __init__(self, lib, names):
        import threading
        object.__setattr__(self, "_lib", lib)
        object.__setattr__(self, "_names", names)
        object.__setattr__(self, "_thread", threading.get_ident())
        object.__setattr__(self, "_ident", threading.get_ident)

    def __getattr__(self, k):
        fn = getattr(self._lib, k)

        def wrapped(*a):
            if self._ident() == self._thread:
                self._names.append(k)
            return fn(*a)
        return wrapped


def run_recorded(torch, steps, call_steps, logger=None):
    import surfel_native as n
    tr, _ = make_run(torch, logger)
    lib, names = n.load(), []
    n._lib = Recorder(lib, names)
    try:
        for _ in range(call_steps):
            tr.step()
    finally:
        n._lib = lib
    for _ in range(steps - call_steps):
        tr.step()
    torch.cuda.synchronize()
    return names, tr.model.theta.clone()


def test_training_without_a_logger_is_untouched(torch, SL, tmp_path):
    base, theta = run_recorded(torch, 30, 10)
    again, theta2 = run_recorded(torch, 30, 10)
    assert base == again and "surfel_log_append" not in base and len(base) > 40      # no launch, buffer or thread without a logger
    with SL.EventWriter(str(tmp_path), block=8) as writer:
        logged, theta3 = run_recorded(torch, 30, 10, writer)
    assert logged.count("surfel_log_append") == 10
    assert [k for k in logged if k != "surfel_log_append"] == base      # the parent's calls plus exactly one append per step
    if torch.equal(theta, theta2):      # two runs of the parent agree bit for bit: then the logged run must too (LOG.md)
        assert torch.equal(theta, theta3)
    else:
        print("two runs without a logger differ: parameters not compared")
    assert len(SL.read_events(writer.path)) == 1 + 30


# ------------------------------------------------------------------------------------------------ 6. the CLI
def test_trainer_cli_with_tensorboard_and_the_reader_cli(torch, SL, tmp_path, capsys):
    """surfel_trainer.py --tensorboard on a small COLMAP capture (tests/test_gpu_scene.py's): the steps, both splits' reports at both test
    iterations, ground_truth on the first only; then surfel_log.py turns the file into CSV and PNG files.  Without the flag: no file."""
    import surfel_trainer as TR
    from test_gpu_scene import _write_capture
    root, model, plain = str(tmp_path / "capture"), str(tmp_path / "model"), str(tmp_path / "plain")
    _write_capture(torch, root)
    common = ["-s", root, "--eval", "--iterations", "12", "--test_iterations", "5", "12", "--save_iterations", "12", "--quiet"]
    assert TR.main(common + ["-m", plain]) == 0 and not [f for f in os.listdir(plain) if f.startswith("events.")]
    assert TR.main(common + ["-m", model, "--tensorboard"]) == 0
    (path,) = SL.event_files(model)
    events = SL.read_events(path)
    assert [ev["step"] for ev in step_events(SL, events)] == list(range(1, 13))
    images = [(ev["step"], v["tag"]) for ev in events for v in ev["values"] if "image" in v]
    assert len(images) == len(set(images)) == (1 + 5) * (7 + 6)      # one held-out view and the train subset's five, at two iterations
    truth = [(step, tag) for step, tag in images if tag.endswith("/ground_truth")]
    assert len(truth) == 6 and {step for step, _ in truth} == {5} and ("test_view_000/ground_truth" in [tag for _, tag in truth])
    assert {tag.split("/")[1] for _, tag in images} == {label for label, _, _ in SL.PANELS} | {"ground_truth"}
    scal = [(ev["step"], v["tag"]) for ev in events for v in ev["values"] if "loss_viewpoint" in v["tag"]]
    assert sorted(scal) == sorted((it, "%s/loss_viewpoint - %s" % (name, what)) for it in (5, 12) for name in ("test", "train") for what in ("l1_loss", "psnr"))
    capsys.readouterr()
    assert SL.main([model, "--csv", "--images", str(tmp_path / "panels")]) == 0
    rows = capsys.readouterr().out.strip().splitlines()
    assert rows[0].split(",")[0] == "step" and [r.split(",")[0] for r in rows[1:]] == [str(k) for k in range(1, 13)]
    from PIL import Image
    png = Image.open(str(tmp_path / "panels" / "000005" / "test_view_000__depth.png"))
    assert png.size == (64, 48) and png.mode == "RGB"
    assert len(os.listdir(str(tmp_path / "panels" / "000012"))) == 6 * 6
