"""What weight averaging (Optim.ema_decay) costs: the training step of final_model_synthetic.yaml at the benchmark's shape with the
average off and on - two models in one process, blocks of steps interleaved, warm-up discarded, medians of the blocks - and
lfi_ema_update alone under HIP events, with its achieved bytes/s (12 bytes per parameter: two reads, one write) beside the same
figure for the Adam kernel (28 bytes per parameter: p, g, m, v read; p, m, v written). No threshold: the expectation is the byte
arithmetic of DESIGN.md section 13.
usage: python tools/ema_cost.py [--out profiles/ema_cost.md] [--batch 256] [--seq-len 80] [--blocks 7] [--block-steps 20]"""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(hparams_file, batch, seq_len, precision, ema_decay, device):
    """bench.py's model: random init under seed_everything(1234)."""
    from argparse import Namespace
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    from lets_face_it_amd.glow.utils import load_hparams_file
    from lets_face_it_amd.trainer import Trainer
    hp = load_hparams_file(hparams_file)
    hp["batch_size"], hp["engine_precision"] = batch, precision
    hp["Train"]["seq_len"] = seq_len
    if ema_decay:
        hp["Optim"]["ema_decay"] = ema_decay
    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    ns = Namespace(**hp)
    model = LetsFaceItGlow(ns).to(device).train()
    return model, Trainer(ns, device=device, checkpoint_dir="").lr_at(0)


def synthetic_batch(B, T, C, S, seed, device):
    g = torch.Generator().manual_seed(seed)
    return {name: torch.randn(B, T, d, generator=g, dtype=torch.float32).to(device).contiguous()
            for name, d in (("p1_face", C), ("p2_face", C), ("p1_speech", S), ("p2_speech", S))}


def timed_ms(fn, count):
    """Milliseconds per call of `count` back-to-back calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(count):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / count


def kernel_rates(n, decay, device, sets, launches, reps):
    """Median microseconds per launch of lfi_ema_update and lfi_adam_clip_step on buffers of n floats: `sets` = 1 is the same buffers
    back to back (they may stay in the last-level cache), more rotates over that many buffer sets."""
    from lets_face_it_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    bufs = [[torch.randn(n, device=device) * 0.01 for _ in range(4)] for _ in range(sets)]
    for b in bufs:
        b[3].abs_()      # second moments are not negative
    sumsq = torch.zeros(1, dtype=torch.float64, device=device)

    def ema(i):
        e, p = bufs[i % sets][0], bufs[i % sets][1]
        _lib.check(L.lfi_ema_update(e.data_ptr(), p.data_ptr(), n, decay, st), "lfi_ema_update")

    def adam(i):
        p, g, m, v = bufs[i % sets]
        _lib.check(L.lfi_adam_clip_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, sumsq.data_ptr(), 0.0, 1.0, 1e-5,
                                        0.9, 0.9999, 1e-8, 1 + i, st), "lfi_adam_clip_step")

    out = {}
    for name, fn in (("ema", ema), ("adam", adam)):
        timed_ms(fn, launches)      # warm-up
        out[name] = 1e3 * statistics.median(timed_ms(fn, launches) for _ in range(reps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_cost.md"))
    ap.add_argument("--hparams", default=os.path.join(ROOT, "lets_face_it_amd", "hparams", "final_model_synthetic.yaml"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=80)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-steps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_cost.py measures on the GPU; none found")
    device = torch.device("cuda:0")
    arms = {}
    for name, decay in (("off", None), ("on", a.decay)):
        model, lr = build(a.hparams, a.batch, a.seq_len, a.precision, decay, device)
        spec = model.seq_glow.spec
        batches = [synthetic_batch(a.batch, a.seq_len, spec.C, spec.S, 1234 + i, device) for i in range(2)]
        arms[name] = (model, lambda i, m=model, bt=batches, lr=lr: m.fused_training_step(bt[i & 1], lr, 1, None))
    for name in arms:      # warm-up, discarded: ActNorm init, workspace growth, the first copy of the average
        timed_ms(arms[name][1], a.warmup)
    blocks = {"off": [], "on": []}
    for r in range(a.blocks):
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            blocks[name].append(timed_ms(arms[name][1], a.block_steps))
    eng = arms["on"][0].seq_glow.engine
    n = eng.n_params
    assert eng.ema_updates == a.warmup + a.blocks * a.block_steps and arms["off"][0].seq_glow.engine.ema is None
    med = {k: statistics.median(v) for k, v in blocks.items()}
    same = kernel_rates(n, a.decay, device, sets=1, launches=50, reps=5)
    cold = kernel_rates(n, a.decay, device, sets=6, launches=48, reps=5)

    def rate(bytes_per_param, us):
        return bytes_per_param * n / (us * 1e-6) / 1e12

    lines = [
        "# Cost of weight averaging (`Optim.ema_decay`)",
        "",
        "`python tools/ema_cost.py` on one MI355X: `%s`, batch %d, T = %d, %s, decay %g; %d parameters (%.1f MB per flat buffer)."
        % (os.path.basename(a.hparams), a.batch, a.seq_len, a.precision, a.decay, n, 4 * n / 1e6),
        "Two models in one process, the average off and on; %d warm-up steps each discarded, then %d blocks of %d steps per arm,"
        % (a.warmup, a.blocks, a.block_steps),
        "arms alternating (the order flips every round), each block timed by device events around it.",
        "",
        "## Training step",
        "",
        "| arm | median ms per step | blocks (ms per step) |",
        "|---|---|---|",
    ]
    for k in ("off", "on"):
        lines.append("| `ema_decay` %s | %.3f | %s |" % (k, med[k], ", ".join("%.3f" % v for v in blocks[k])))
    spread = max(max(v) - min(v) for v in blocks.values())
    lines += [
        "",
        "Difference of the medians: %+.3f ms (%+.2f %%); largest block-to-block range within one arm: %.3f ms."
        % (med["on"] - med["off"], 100.0 * (med["on"] - med["off"]) / med["off"], spread),
        "",
        "## Kernels alone",
        "",
        "Median of 5 timings of ~50 back-to-back launches on buffers of %d floats. Bytes per launch: `lfi_ema_update` 12 n (two reads,"
        % n,
        "one write), `lfi_adam_clip_step` 28 n (four reads, three writes).",
        "",
        "| kernel | buffers | us per launch | achieved TB/s |",
        "|---|---|---|---|",
    ]
    for label, res in (("the same buffers every launch", same), ("rotating over 6 buffer sets", cold)):
        lines.append("| `lfi_ema_update` | %s | %.1f | %.2f |" % (label, res["ema"], rate(12, res["ema"])))
        lines.append("| `lfi_adam_clip_step` | %s | %.1f | %.2f |" % (label, res["adam"], rate(28, res["adam"])))
    lines += [
        "",
        "The byte arithmetic expected 12 n = %.0f MB per update; fusing the update into the optimiser kernel would save one read of the"
        % (12 * n / 1e6),
        "parameters, 4 n = %.0f MB, i.e. about %.0f us of the rotating-buffers figure above." % (4 * n / 1e6, cold["ema"] / 3.0),
        "",
    ]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
