"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run times the headline and nothing else (every other leg is behind
--full), and spends little time outside its steps.

Like tests/test_a_gpu_dp.py this file sorts before the GPU tests that initialise the card in the pytest process, and does not
touch the GPU itself: the benchmark runs as a child process."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("cpu_baseline", "torch_gpu_baseline", "three_products_everywhere", "strong_scaling_anchor", "data_parallel",
             "sampling", "deep_flow", "native_dims")


def test_plain_bench_run_is_the_headline_only(tmp_path):
    """One plain run with --dump-outputs: one JSON line with the headline fields, no record of a --full leg, the dump of the last
    timed step, and at most 30 s of wall time (start to exit) beyond (K + W) x ms_per_step."""
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: run tests/test_a_gpu_bench.py on its own or first")
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU")
    steps, warmup = 10, 3
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "dump")]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=360)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-1500:]
    rec = json.loads(lines[0])
    assert rec["metric"].startswith("FLAME frames/s, full training step") and rec["unit"] == "frames/s"
    assert rec["higher_is_better"] is True and rec["dtype"].startswith("f32")
    assert rec["n_gpus"] == 1 and rec["steps"] == steps and rec["warmup"] == warmup
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["final_loss"] == rec["final_loss"]
    assert rec["roofline"]["launches_timed"] > 0
    assert not [k for k in FULL_ONLY if k in rec], sorted(rec)
    assert rec["hipgraph_replay"] is None and rec["gpu_state_under_load"] is None and rec["host_issue_ms_per_step"] is None
    # only the roofline kernels' events, which sit inside the timed region
    assert all(t == "gemm_cond_fwd" or t.startswith("enc_fwd.") for t in rec["kernel_timing"]), rec["kernel_timing"]
    assert sorted(os.listdir(tmp_path / "dump")) == ["loss.npy", "parameters.npy"]
    outside = wall - (steps + warmup) * rec["ms_per_step"] * 1e-3
    assert outside < 30.0, "%.1f s outside the steps (wall %.1f s)" % (outside, wall)
