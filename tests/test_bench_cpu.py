"""bench.py launch contract (no GPU needed): `python bench.py --gpus N` run DIRECTLY must spawn N ranks,
the driver's explicit torch.distributed.run form must work too, and a --gpus / WORLD_SIZE mismatch must fail loudly."""
import json
import os
import socket
import subprocess
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def _last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, out
    return json.loads(lines[-1])


def test_direct_invocation_spawns_n_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-spawn"], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert j["n_gpus"] == 2 and j["ranks_in_all_reduce"] == 2


def test_driver_torchrun_form():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), BENCH, "--gpus", "2", "--rehearse-spawn"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _last_json(r.stdout)["n_gpus"] == 2


def test_world_size_mismatch_fails_loudly():
    env = _env(); env.update(WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-spawn"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=4" in (r.stderr + r.stdout)


def test_result_line_is_compact_and_keeps_the_headline():
    """The printed line of a full N = 1 run (every side leg on, profiles/r06_bench_n1_final.json: 21.7 KB as one object) fits in
    bench.LINE_MAX and keeps the headline, its roofline and the CPU baseline; side legs keep their numbers."""
    sys.path.insert(0, REPO)
    import bench
    with open(os.path.join(REPO, "profiles", "r06_bench_n1_final.json")) as f:
        full = json.loads(f.read().strip().splitlines()[-1])
    line = bench.result_line(full)
    assert "\n" not in line and len(line) <= bench.LINE_MAX, len(line)
    j = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline", "step_roofline", "cpu_baseline"):
        assert j[k] == full[k] or k in ("config", "roofline"), k
    assert j["config"]["workload"] == full["config"]["workload"] and j["roofline"]["all_kernels_ms"] == full["roofline"]["all_kernels_ms"]
    assert j["legs"]["C2"]["ms_per_step"] == full["legs"]["C2"]["ms_per_step"]


def test_dump_outputs_sample_is_seeded_and_bounded(tmp_path):
    """--dump-outputs on a stand-in trainer (host tensors in the model's layout): float32 / float64 files, the same sample every
    time, per-surfel rows matching the store, well under 64 MB for a garden-sized model."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    from surfel_model import FLOATS, SECTIONS, _views
    P = 2_200_000
    g = torch.Generator().manual_seed(0)
    m = types.SimpleNamespace(P=P, theta=torch.rand(P * FLOATS, generator=g), m=torch.rand(P * FLOATS, generator=g),
                              v=torch.rand(P * FLOATS, generator=g), xyz_gradient_accum=torch.rand(P, 1, generator=g),
                              denom=torch.rand(P, 1, generator=g), max_radii2D=torch.rand(P, generator=g))
    tr = types.SimpleNamespace(model=m, last=dict(scalars=torch.rand(6, generator=g), radii=torch.randint(0, 9, (P,), dtype=torch.int32)))
    bench.dump_outputs(tr, str(tmp_path / "a"))
    bench.dump_outputs(tr, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "params.npy" in names and "loss_terms.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) < 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    idx = np.load(tmp_path / "a" / "surfel_index.npy").astype(np.int64)
    params = np.load(tmp_path / "a" / "params.npy")
    xyz = _views(m.theta, P)["xyz"].numpy()
    assert params.shape == (len(idx), FLOATS) and SECTIONS[0][0] == "xyz" and np.array_equal(params[:, :3], xyz[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "radii.npy"), tr.last["radii"].numpy()[idx].astype(np.float32))


def test_plain_run_leaves_every_extra_to_full():
    """A plain run is set-up, warm-up, the timed steps and the line: every side leg is off unless --full; under --full, --quick and the
    --no-* options pick among them as before."""
    sys.path.insert(0, REPO)
    import bench
    extras = ("no_legs", "no_cpu_baseline", "no_1080p", "no_raster_only", "no_full_train", "no_sweep", "no_scale_leg")
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not plain.full and all(getattr(plain, k) for k in extras) and (plain.gpus, plain.steps, plain.warmup) == (1, 7, 3)
    full = bench.parse_args(["--full"])
    assert full.full and not any(getattr(full, k) for k in extras)
    quick = bench.parse_args(["--full", "--quick"])
    assert quick.full and all(getattr(quick, k) for k in extras if k != "no_scale_leg") and not quick.no_scale_leg
    some = bench.parse_args(["--full", "--no-sweep"])
    assert some.no_sweep and not any(getattr(some, k) for k in extras if k != "no_sweep")
