"""bench.py on the GPU: a plain run prints the headline of its timed steps and measures nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ("legs", "raster_fwd_bwd", "fwd_1080p", "fwd_1080p_sweep", "full_train_config3", "cpu_baseline", "cpu_baseline_dense_torch_C1",
        "hbm_copy_probe", "scale_leg_C4")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--workload", "C2", "--steps", "6", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert (j["n_gpus"], j["steps"], j["warmup"], j["unit"], j["dtype"], j["higher_is_better"]) == (1, 6, 2, "train-iters/s", "f32", True)
    assert j["value"] > 0 and abs(j["value"] * j["ms_per_step"] / 1e3 - 1.0) < 1e-2
    assert j["box_probe"] is None and j["roofline"] is None and j["step_roofline"] is None and "instances_R_mean" not in j["config"]
    assert not any(k in j for k in SIDE), [k for k in SIDE if k in j]
    loss = np.load(tmp_path / "loss_terms.npy")
    assert np.isfinite(loss).all() and os.path.exists(tmp_path / "params.npy")
