#!/usr/bin/env python3
"""Keyed against unkeyed streaming sessions (open_stream(row_seeds=...) against open_stream()) of one build on one box, in
alternating blocks: per-call host time, device synchronised at both ends of a block (profiles/stream_row_keys.md).
   python tools/stream_row_keys.py [--blocks 8] [--out FILE.json]
final_model widths at K = 16 (tests/test_gpu_stream.py's _final_setup), bf16x3, the caller on a stream of its own. Cases: step() at
B = 1, 16, 256; step_candidates(8) + commit() at B = 16; rollout_candidates(n = 8, ncand = 8) + commit() at B = 16. Every block
starts from reset(seed) and two untimed calls. Prints one JSON line per case: every block's microseconds per call for both arms,
and their min / median / max."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_parity import to_dev  # noqa: E402
from test_gpu_stream import _final_setup, _frame, _seed  # noqa: E402
from test_gpu_stream_chunk import _chunk  # noqa: E402


def measure(name, B, calls, body, blocks, dev, K=16):
    _, m, _, data, _, _ = _final_setup(dev, B, 8, K=K)
    m.precision = "bf16x3"
    data = to_dev(data, dev)
    seed = _seed(data, 24)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        arms = {"unkeyed": m.open_stream(seed), "keyed": m.open_stream(seed, row_seeds=list(range(1000, 1000 + B)))}
        fr1, frn = _frame(data, 24), _chunk(data, 24, 0, 8)
        times = {k: [] for k in arms}
        for st in arms.values():
            for _ in range(20):
                body(st, fr1, frn)
        for _ in range(blocks):
            for arm, st in arms.items():
                st.reset(seed)
                body(st, fr1, frn)
                body(st, fr1, frn)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    body(st, fr1, frn)
                torch.cuda.synchronize()
                times[arm].append((time.perf_counter() - t0) / calls * 1e6)
        for st in arms.values():
            st.close()
    rec = {"case": name, "B": B, "K": K, "calls_per_block": calls, "blocks_us": times}
    for arm, v in times.items():
        s = sorted(v)
        rec[arm] = {"min": s[0], "median": (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, "max": s[-1]}
    print(json.dumps(rec), flush=True)
    return rec


def step(st, fr1, frn):
    st.step(fr1)


def cands(st, fr1, frn):
    st.step_candidates(fr1, 8)
    st.commit()


def rollouts(st, fr1, frn):
    st.rollout_candidates(frn, 8)
    st.commit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = [measure("step", B, 300, step, a.blocks, dev) for B in (1, 16, 256)]
    results.append(measure("step_candidates(8)+commit", 16, 200, cands, a.blocks, dev))
    results.append(measure("rollout_candidates(n=8, ncand=8)+commit", 16, 60, rollouts, a.blocks, dev))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
