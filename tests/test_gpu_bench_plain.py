"""bench.py on one GPU, the two forms of a run: a plain run times its steps and prints the
headline entries only; --full adds the diagnostic passes' entries to the same line.
--dump-outputs writes the last timed step's {bestp, cost} (what hpe_track_raw_sequence_dev
left in the caller's 27 doubles), the same from run to run and from form to form: the
diagnostic passes restart from the warm-up state and never reach the dumped arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hand_data

pytestmark = pytest.mark.gpu

FULL_ONLY = ("kernels", "roofline", "roofline_kernels", "dominant_kernel", "tracking_err_mm",
             "refine_exact_ms_per_step", "per_frame_graph_ms_per_step", "cpu_baseline")


def _bench(out, *extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, str(hand_data.ROOT / "bench.py"), "--gpus", "1", "--config", "p32",
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), np.load(out / "bestp.npy"), np.load(out / "cost.npy")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


def test_plain_run_times_the_steps_only(plain):
    r, bestp, cost = plain
    assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1 and not r["full"]
    assert r["unit"] == "particle-evals/s" and r["higher_is_better"] and r["dtype"] == "f32+f64"
    assert r["ms_per_step"] > 0
    # value = P * (G + 1) evaluations per step over the timed steps' wall time
    assert r["value"] == pytest.approx(32 * 11 / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert not any(k in r for k in FULL_ONLY)
    assert bestp.dtype == np.float64 and bestp.shape == (26,) and np.all(np.isfinite(bestp))
    assert cost.dtype == np.float64 and cost.shape == (1,) and cost[0] == r["final_cost"]


def test_full_run_adds_the_diagnostics(plain, tmp_path):
    r, bestp, cost = _bench(tmp_path, "--full", "--no-cpu-baseline")
    assert r["full"] and all(k in r for k in FULL_ONLY if k != "cpu_baseline")
    assert r["kernels"]["k_pso_gen"]["launches"] > 0 and r["kernels"]["frame_graph"]["avg_us"] > 0
    assert r["tracking_err_mm"]["sum_wrist_tips_mean"] > 0
    np.testing.assert_array_equal(bestp, plain[1])
    np.testing.assert_array_equal(cost, plain[2])
