"""What the step guard's blame launch (`print_nan_grads: true`) costs - tools/guard_cost.py's protocol: the training step of
final_model_synthetic.yaml at the benchmark's shape, two models in one process, the guard on in both and blame off / on, blocks of steps
interleaved, warm-up discarded, medians of the blocks, every block timed by device events - once with eager launches and once with
step_graph. Nothing is poisoned, so every blame launch returns before its first load: the case that has to cost next to nothing. Then
the entry points alone: lfi_segment_stats_guard behind a taken step (three launches that return at once) and lfi_segment_stats over the
whole gradient (what a skipped step, or a track_grad_norm log line, pays). No threshold: the on arm is judged against the off arm's own
block-to-block range.
usage: python tools/blame_cost.py [--out profiles/blame_cost.md] [--batch 256] [--seq-len 80] [--blocks 7] [--block-steps 20]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from ema_cost import synthetic_batch, timed_ms  # noqa: E402


def build(hparams_file, batch, seq_len, precision, blame, graph, device):
    """tools/guard_cost.py's model with the guard on, and print_nan_grads as asked."""
    import random
    from argparse import Namespace

    import numpy as np
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    from lets_face_it_amd.glow.utils import load_hparams_file
    from lets_face_it_amd.trainer import Trainer
    hp = load_hparams_file(hparams_file)
    hp["batch_size"], hp["engine_precision"] = batch, precision
    hp["Train"]["seq_len"] = seq_len
    hp["Train"]["use_negative_nll_loss"] = False      # one graph per arm, the same launches in every step
    hp["Optim"]["skip_nonfinite"] = True
    hp["print_nan_grads"] = bool(blame)
    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    ns = Namespace(**hp)
    model = LetsFaceItGlow(ns).to(device).train()
    model.step_graph = bool(graph)
    return model, Trainer(ns, device=device, checkpoint_dir="").lr_at(0)


def step_arms(a, graph, device):
    arms = {}
    for name in ("off", "on"):
        model, lr = build(a.hparams, a.batch, a.seq_len, a.precision, name == "on", graph, device)
        spec = model.seq_glow.spec
        batches = [synthetic_batch(a.batch, a.seq_len, spec.C, spec.S, 1234 + i, device) for i in range(2)]
        arms[name] = (model, lambda i, m=model, bt=batches, lr=lr: m.fused_training_step(bt[i & 1], lr, 1, None))
    for name in arms:      # warm-up, discarded: ActNorm init, workspace growth, the capture
        timed_ms(arms[name][1], a.warmup)
    blocks = {"off": [], "on": []}
    for r in range(a.blocks):
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            blocks[name].append(timed_ms(arms[name][1], a.block_steps))
    steps = a.warmup + a.blocks * a.block_steps
    for name in arms:
        eng = arms[name][0].seq_glow.engine
        gs = eng.guard_state()
        assert gs["applied"] == steps and gs["skipped"] == 0, gs
        assert (eng.blame is not None) == (name == "on")
        if graph:
            graphs = [v for v in arms[name][0].__dict__.get("_step_graphs", {}).values() if isinstance(v, dict)]
            assert len(graphs) == 1, "the %s arm did not run on a captured step" % name
    eng = arms["on"][0].seq_glow.engine
    assert eng.blame_state() is None and eng._blame_launches == steps
    return blocks, eng


def entries_alone(eng, launches, reps):
    """Median microseconds per call of the two entry points over the engine's own gradient segments: the guarded one behind a taken
    step (APPLY = 1), the guarded one filling (APPLY = 0, header cleared before every call by a 16-byte memset that is timed with it),
    and the unconditional one."""
    from lets_face_it_amd import _lib
    L = eng.L
    st = torch.cuda.current_stream().cuda_stream
    keys, table = eng._segment_table()
    work = eng._stats_work([])
    out = torch.zeros(_lib.SEG_SLOTS * len(keys), dtype=torch.int64, device=eng.device)
    blame = torch.zeros(_lib.BLAME_HEAD + _lib.SEG_SLOTS * len(keys), dtype=torch.int64, device=eng.device)
    rec = {flag: torch.zeros(_lib.GUARD_SLOTS, dtype=torch.int64, device=eng.device) for flag in (0, 1)}
    rec[1][_lib.GUARD_APPLY] = 1
    g, n = eng.grads.data_ptr(), eng.n_params

    def plain(i):
        _lib.check(L.lfi_segment_stats(g, n, table.data_ptr(), len(keys), 0, None, None, out.data_ptr(), work.data_ptr(), st), "lfi_segment_stats")

    def taken(i):
        _lib.check(L.lfi_segment_stats_guard(g, n, table.data_ptr(), len(keys), 0, None, None, rec[1].data_ptr(), blame.data_ptr(),
                                             work.data_ptr(), st), "lfi_segment_stats_guard")

    def filling(i):
        blame[:_lib.BLAME_HEAD].zero_()
        _lib.check(L.lfi_segment_stats_guard(g, n, table.data_ptr(), len(keys), 0, None, None, rec[0].data_ptr(), blame.data_ptr(),
                                             work.data_ptr(), st), "lfi_segment_stats_guard")

    res = {}
    for name, fn in (("taken", taken), ("filling", filling), ("plain", plain)):
        timed_ms(fn, launches)      # warm-up
        res[name] = 1e3 * statistics.median(timed_ms(fn, launches) for _ in range(reps))
    torch.cuda.synchronize()
    assert torch.equal(blame[_lib.BLAME_HEAD:], out), "the two entry points disagree"
    return res, len(keys), max(int(v) for v in table.view(-1, 2)[:, 1].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blame_cost.md"))
    ap.add_argument("--hparams", default=os.path.join(ROOT, "lets_face_it_amd", "hparams", "final_model_synthetic.yaml"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=80)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-steps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/blame_cost.py measures on the GPU; none found")
    device = torch.device("cuda:0")
    results, alone = {}, None
    for mode, graph in (("eager", False), ("step_graph", True)):
        blocks, eng = step_arms(a, graph, device)
        results[mode] = blocks
        if alone is None:
            alone = entries_alone(eng, launches=50, reps=5) + (eng.n_params,)
        del eng
        torch.cuda.empty_cache()
    res, ntensors, longest, n = alone
    from lets_face_it_amd import _lib
    CH = _lib.lib().lfi_segment_stats_chunk()

    lines = [
        "# Cost of the step guard's blame launch (`print_nan_grads: true`)",
        "",
        "`python tools/blame_cost.py` on one MI355X: `%s`, batch %d, T = %d, %s; %d parameters in %d tensors (the longest %d floats)."
        % (os.path.basename(a.hparams), a.batch, a.seq_len, a.precision, n, ntensors, longest),
        "Two models in one process, the step guard on in both, blame off (the parent commit's behaviour) and on; %d warm-up steps each"
        % a.warmup,
        "discarded, then %d blocks of %d steps per arm, arms alternating (the order flips every round), each block timed by device events"
        % (a.blocks, a.block_steps),
        "around it. Nothing is poisoned: every step is taken, so each of the on arm's three blame launches per step returns before its first",
        "load of data (the record stayed empty, checked). The arrays of a step: the %d gradient tensors, four input tensors, the per-frame NLL."
        % ntensors,
        "",
    ]
    for mode in ("eager", "step_graph"):
        blocks = results[mode]
        med = {k: statistics.median(v) for k, v in blocks.items()}
        lo, hi = min(blocks["off"]), max(blocks["off"])
        inside = lo <= med["on"] <= hi
        lines += ["## Training step, %s" % mode, "", "| arm | median ms per step | blocks (ms per step) |", "|---|---|---|"]
        for k in ("off", "on"):
            lines.append("| blame %s | %.3f | %s |" % (k, med[k], ", ".join("%.3f" % v for v in blocks[k])))
        lines += [
            "",
            "Difference of the medians: %+.3f ms (%+.2f %%). The off arm's own blocks range over %.3f .. %.3f ms: the on arm's median lies %s"
            % (med["on"] - med["off"], 100.0 * (med["on"] - med["off"]) / med["off"], lo, hi,
               "inside that range." if inside else "OUTSIDE that range (the figure is reported as measured)."),
            "",
        ]
    lines += [
        "## The entry points alone",
        "",
        "Median of 5 timings of 50 back-to-back calls over the gradient buffer of %d floats (%.1f MB) cut into the model's %d segments, no"
        % (n, 4 * n / 1e6, ntensors),
        "extra arrays; each call is three launches (plan, one workgroup per chunk of %d floats, finish). The filling arm clears the header"
        % CH,
        "before every call (a 16-byte memset, timed with it).",
        "",
        "| call | us per call | gradient bytes read | achieved TB/s |",
        "|---|---|---|---|",
        "| `lfi_segment_stats_guard` behind a taken step (APPLY = 1) | %.1f | 0 | - |" % res["taken"],
        "| `lfi_segment_stats_guard` filling the record (APPLY = 0, FILLED = 0) | %.1f | %.0f MB | %.2f |"
        % (res["filling"], 4 * n / 1e6, 4 * n / (res["filling"] * 1e-6) / 1e12),
        "| `lfi_segment_stats` (unconditional: `grad_tensor_norms`) | %.1f | %.0f MB | %.2f |"
        % (res["plain"], 4 * n / 1e6, 4 * n / (res["plain"] * 1e-6) / 1e12),
        "",
    ]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
