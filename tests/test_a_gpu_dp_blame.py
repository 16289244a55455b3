"""GPU, two ranks on ONE card over gloo: the step guard's blame record under data parallelism (tools/dp_gloo_check.py --blame). Three
eager steps, rank 1's shard poisoned on the second: the gradient is blamed after the all-reduce, so both ranks name the same gradient
tensors for step 2, while only rank 1 - whose shard held the NaN - names an input (p1_face, with row, frame and column) and non-finite
NLL entries.

As tests/test_a_gpu_dp_guard.py: this file sorts early and must not touch the GPU itself - the check runs in a subprocess, and its
time is process start-up."""
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


def test_two_ranks_blame_the_same_gradients_and_only_the_poisoned_rank_an_input():
    limit = 240
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: run tests/test_a_gpu_dp_blame.py on its own or first")
    if not os.path.exists("/dev/kfd"):
        pytest.skip("no GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "dp_gloo_check.py"), "--blame"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit + 60)
    out = r.stdout
    tail = "\n".join([ln for ln in out.splitlines() if "blame" in ln or "guard" in ln] + out.splitlines()[-15:])
    assert r.returncode == 0, tail
    # (two ranks write to one pipe: their lines can run into each other, so everything below looks for text, not for whole lines)
    found = {int(m.group(1)): m for m in re.finditer(
        r"blame rank (\d): step (\d+), gradient tensors blamed (\d+) \(same on every rank (True|False)\), inputs (\[.*?\]), "
        r"non-finite NLL entries (-?\d+)", out)}
    assert sorted(found) == [0, 1], tail
    for rank, m in found.items():
        assert m.group(2) == "2" and int(m.group(3)) > 0 and m.group(4) == "True", tail
    assert found[0].group(3) == found[1].group(3), tail
    assert found[0].group(5) == "[]" and found[0].group(6) == "0", tail
    assert re.fullmatch(r"\[\('p1_face', \(3, \d+, 1\)\)\]", found[1].group(5)) and int(found[1].group(6)) > 0, tail
    assert re.search(r"skipped on every rank, ranks identical after every step: True", out), tail
