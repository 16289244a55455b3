"""GPU, two ranks on ONE card over gloo: the non-finite step guard under data parallelism (tools/dp_gloo_check.py --guard). Only
rank 1's shard is poisoned, on step 2 of 4; the decision is taken on the all-reduced gradient, so both ranks report the skip, the
parameters are identical across ranks after every step and equal to the pre-step values after step 2.

As tests/test_a_gpu_dp.py: this file sorts early and must not touch the GPU itself - the check runs in a subprocess."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _launch(extra, limit=240):
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: run tests/test_a_gpu_dp_guard.py on its own or first")
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "dp_gloo_check.py"), "--guard"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit + 60)
    # (two ranks write to one pipe: their lines can run into each other, so everything below looks for text, not for whole lines)
    tail = "\n".join([ln for ln in r.stdout.splitlines() if "guard" in ln] + r.stdout.splitlines()[-15:])
    assert r.returncode == 0, tail
    return r, r.stdout, tail


def test_two_rank_guard_skips_on_every_rank_when_one_shard_is_poisoned():
    r, out, tail = _launch([])
    for rank in (0, 1):
        for step in (1, 2, 3, 4):
            skip = step == 2
            want = "guard rank %d step %d: apply %d, parameters unchanged %s, ranks identical True" % (rank, step, 0 if skip else 1, skip)
            assert want in out, tail
        assert "guard rank %d: skipped 1 consecutive 0 applied 3 step_count 3" % rank in out, tail
    assert re.search(r"skipped on every rank, ranks identical after every step: True", r.stdout), tail


def test_two_rank_guard_as_two_graphs_matches_the_eager_data_parallel_step():
    """Eight steps, rank 1's shard poisoned on the sixth - a replay of the two captured graphs, whose eager decide launch reads the
    host's step number from the graph's params block: skipped on every rank, and the parameters after the eight steps are bit-identical
    to the eager data-parallel run's."""
    r, out, tail = _launch(["--graph"], limit=300)
    for rank in (0, 1):
        assert "guard rank %d: graph leg bit-identical to the eager leg: True; steps on captured graphs: " % rank in out, tail
        assert out.count("guard rank %d: skipped 1 consecutive 0 applied 7 step_count 7" % rank) == 2, tail
        assert out.count("guard rank %d step 6: apply 0, parameters unchanged True, ranks identical True" % rank) == 2, tail
    assert re.search(r"skipped on every rank, ranks identical after every step: True", r.stdout), tail
