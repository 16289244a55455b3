"""Latency of one streaming sampling step (SeqGlow.open_stream -> SampleStream.step) at final_model.yaml, against the only correct
alternative without a session: re-running SeqGlow.inference over the whole prefix for every new frame.

  python tools/stream_latency.py [--batches 1,16,256] [--steps 200] [--warmup 20] [--prefixes 50,150,300] [--out FILE]
                                 [--churn 1,16,64 [--churn-batch 256]] [--migrate 16 [--migrate-batch 256]] [--nll 1,256]
                                 [--observe 1,16,256] [--rows 1,16,256] [--observe-many 16,64,250]
                                 [--step-many 4,16,64] [--observe-ragged 16,64,250] [--rows-many 4,16,64]
                                 [--candidates 16,8 [--passes 5]]
                                 [--rollouts 16,8,8 [--passes 5]]

Per batch size: the wall-clock time from step() to the generated frame on the host (a synchronise after every step: what a live agent
waits for), its GPU time (HIP events around the step), and a per-kernel breakdown from the engine's enable_timing on an eager session
(LFI_NO_GRAPH=1: inside a replayed graph there are no per-kernel events). Then inference() over a prefix of t frames in total (t - 24
generated), the cost of frame t without a session. Prints a markdown report (and writes it to --out); the shader clock under load is
read by bench.py's rocm-smi helper, started before this process touches the GPU.

--churn r1,r2,..: a session of --churn-batch rows serving conversations that come and go - before every step r rows (a different set
each step) are reseeded with SampleStream.reset_rows. Per r and per caller (on the legacy default stream, as the legs above, and on a
stream of its own), interleaved step by step in one session: a plain step, reseed + step, and the reseed alone, each timed as above
(wall clock with a synchronise after it, and HIP events around it).

--migrate r1,r2,..: two sessions of --migrate-batch rows; before every step of the first, r of its rows (a different set each step) are
saved with SampleStream.save_rows and loaded into rows of the second with load_rows - a conversation moving to another session. Per r
and caller as --churn, interleaved step by step in one process: a plain step, save + load + step, and the save + load pair alone.

--nll b1,b2,..: per batch size two sessions on the same seed, frames and noise, one opened with return_nll=True (every step also
returns the frame's NLL) and one without, interleaved step by step in one process: what the likelihood costs a step. Then
inference() over --nll-frames generated frames with and without return_nll, the two alternated call by call.

--observe b1,b2,..: per batch size a generating session (step()) and a teacher-forced one (observe(), NLL only and with z) on the same
seed and conditioning, interleaved step by step in one process, which goes first alternating; the observed faces are what an untimed
generating session produced beforehand.

--rows b1,b2,..: this leg ALONE (nothing of the above runs), written to --out (default profiles/stream_step_rows.md): per batch size,
a caller on its own stream, every leg interleaved step by step in one process with the order rotating - (a) step(return_nll=True) and
observe(); (b) step_rows() with every row generating and with every row observing; (c) step_rows() with the first half of the 16-row
tiles observing and the rest generating (B >= 32); (d) step_rows() with odd rows observing, even rows generating (B >= 2); (e) what a
server has without step_rows: step() on one session of B / 2 rows, then observe() on another (B >= 2).

--observe-many n1,n2,..: this leg ALONE, written to --out (default profiles/stream_observe_many.md): per batch size of --batches and per
chunk length n, two sessions on one seed, both one observed frame into their sequence: n observe() calls in a Python loop on the one,
one observe_many(n) on the other, alternating which goes first, --reps times after two untimed rounds (sessions are reset(seed) in
between, graphs kept). Per frame: wall clock (a synchronise after the whole loop / call) and GPU time (HIP events around it). Then the
front end / chain split of one observe_many per n from the engine's enable_timing.

--step-many n1,n2,..: this leg ALONE, written to --out (default profiles/stream_step_many.md): per batch size of --batches and per n, two
sessions on one seed, both one generated frame into their sequence: n step() calls in a Python loop on the one, one step_many(n) on
the other, the same conditioning and noise, alternating which goes first, --reps times after two untimed rounds (sessions are
reset(seed) in between, graphs kept). Per frame: wall clock and GPU time as --observe-many. Then where one step_many call's GPU time
goes (windows in, static part, the sampler's n front ends and chains) from the engine's enable_timing.

--observe-ragged n1,n2,..: this leg ALONE, written to --out (default profiles/stream_observe_ragged.md): per batch size of --batches and
per n, observe_many(n) with per-row lengths beside the dense call, every arm of a (B, n) on a session of its own one observed frame
into its sequence, the order rotating, --reps times after two untimed rounds: (a) dense against lengths all n, with the dense arm's
own rep-to-rep spread; (b) (B > 16) the first 16-row tile at length n and every other row at 0 - joiners warmed up in place - with
its front end / chain split (LFI_CHUNK_ONLY) and, beside it, the side-session recipe: open_stream for 16 rows, observe_many, save_rows,
load_rows into the big session; (c) lengths spread evenly over 0 .. n. Then the register figures of the dense and the ragged chain
kernels from tools/kernel_resources.py (compiled for gfx950 while the GPU is still untouched).

--rows-many n1,n2,..: this leg ALONE, written to --out (default profiles/stream_step_rows_many.md): per batch size of --batches and per
n, every arm on a session of its own one generated frame into its sequence, the same conditioning, faces and noise, the order
rotating, --reps times after two untimed rounds: (a) n step_rows() calls in a Python loop (host masks, as the chunk call takes them);
(b) step_rows_many(n) with the first half of the 16-row tiles observing and the rest generating (B >= 32; the loop runs this mask
there); (c) step_rows_many(n) with odd rows observing and even rows generating - every tile mixed (B >= 2; at B = 1 the one row
alternates frame by frame; below B = 32 the loop runs this mask); (d) step_rows_many(n) with a prompt-then-continue mask, prompt
lengths spread over n / 4 .. 3 n / 4, with the plan on and (e) with LFI_ROWS_MANY_OBSERVE_RUN=0. Per frame: wall clock and GPU time
as --step-many. Then where the GPU time of arms (d) and (e) goes, from the engine's enable_timing.

--candidates B,ncand: this leg ALONE, written to --out (default: printed only): best-of-N per frame for B conversations, two arms
alternated as whole passes, --passes of each (the recipe first) of --steps timed frames after --warmup untimed ones, a caller on the
legacy default stream. (new) step_candidates(frame, ncand, noise) + commit() on a session of B rows. (recipe) what INTEGRATION.md
prescribed before those calls existed, on a session of B * ncand rows opened with return_nll=True, conversation r at home in row
r * ncand: save_rows(home rows), load_rows(every row, entries = row // ncand), step() with every row's conditioning repeated ncand
times (the repeats are made before the clock starts), the arg-min per conversation read on the host, save_rows(the winners'
rows), load_rows(home rows). Per pass: the median frame's wall clock (a synchronise after the frame) and GPU time (HIP events). Then
the stream_advance / stream_static / stream_chain timers of both arms from the engine's enable_timing on eager sessions
(LFI_NO_GRAPH=1), and the shader clock under the new arm's load.

--rollouts B,ncand,n: this leg ALONE, written to --out (default: printed only): best-of-N over n frames for B conversations, two
arms alternated as whole passes, --passes of each (the recipe first) of --steps timed rollouts after --warmup untimed ones, a
caller on the legacy default stream. (new) rollout_candidates(frames, ncand, noise) + commit() on a session of B rows. (recipe) what
INTEGRATION.md prescribes with rows, on a session of B * ncand rows opened with return_nll=True, conversation r at home in row
r * ncand: save_rows(home rows), load_rows(every row, entries = row // ncand), step_many() with every row's conditioning repeated
ncand times (the repeats are made before the clock starts), the arg-min of the summed NLL per conversation read on the host,
save_rows(the winners' rows), load_rows(home rows). Per pass: the median rollout's wall clock (a synchronise after it) and GPU time
(HIP events), per committed frame. Then where the new arm's GPU time goes, from the engine's enable_timing: windows in, static part,
candidates in, front end + chain, commit; the front end alone from a call with LFI_CHUNK_ONLY=front, the chain by difference."""
import argparse
import contextlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--prefixes", default="50,150,300")
    ap.add_argument("--out", default=None)
    ap.add_argument("--churn", default=None, help="rows reseeded before every step, e.g. 1,16,64 (default: no churn leg)")
    ap.add_argument("--churn-batch", type=int, default=256)
    ap.add_argument("--migrate", default=None, help="rows saved and loaded into a second session before every step, e.g. 16")
    ap.add_argument("--migrate-batch", type=int, default=256)
    ap.add_argument("--nll", default=None, help="batch sizes of the return_nll leg, e.g. 1,256 (default: no such leg)")
    ap.add_argument("--nll-frames", type=int, default=0, help="with --nll: also inference() over this many generated frames, flag off / on")
    ap.add_argument("--observe", default=None, help="batch sizes of the observe() leg, e.g. 1,16,256 (default: no such leg)")
    ap.add_argument("--rows", default=None, help="batch sizes of the step_rows() leg, e.g. 1,16,256: runs this leg alone")
    ap.add_argument("--observe-many", default=None, help="chunk lengths of the observe_many() leg, e.g. 16,64,250: runs this leg alone")
    ap.add_argument("--step-many", default=None, help="frames per call of the step_many() leg, e.g. 4,16,64: runs this leg alone")
    ap.add_argument("--observe-ragged", default=None, help="chunk lengths of the ragged observe_many() leg: runs this leg alone")
    ap.add_argument("--rows-many", default=None, help="frames per call of the step_rows_many() leg, e.g. 4,16,64: runs this leg alone")
    ap.add_argument("--candidates", default=None, help="B,ncand of the best-of-N leg, e.g. 16,8: runs this leg alone")
    ap.add_argument("--rollouts", default=None, help="B,ncand,n of the best-of-N-over-n-frames leg, e.g. 16,8,8: runs this leg alone")
    ap.add_argument("--passes", type=int, default=5, help="with --candidates / --rollouts: whole passes per arm, alternated")
    ap.add_argument("--reps", type=int, default=7, help="with --observe-many / --step-many / --observe-ragged: timed rounds per (batch size, chunk length)")
    a = ap.parse_args()
    resources = chain_kernel_resources() if a.observe_ragged else None     # (compiles; before the GPU is initialised)
    import bench
    helper = bench.start_smi_helper()       # (before the GPU is initialised: see bench.py)
    import copy
    from argparse import Namespace

    import torch
    from lets_face_it_amd.glow.models import SeqGlow
    from lets_face_it_amd.glow.utils import load_hparams_file

    dev = torch.device("cuda:0")
    hp = load_hparams_file(os.path.join(ROOT, "lets_face_it_amd", "hparams", "final_model.yaml"))
    torch.manual_seed(1234)
    m = SeqGlow(Namespace(**copy.deepcopy(hp)))
    g = torch.Generator().manual_seed(4321)
    with torch.no_grad():     # LinearZeros / ActNorm off their zero init: at init the coupling ignores its conditioning
        for name, p in m.named_parameters():
            if "final_linear" in name:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
            elif "actnorm" in name:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    m.to(dev)
    m.glow.set_actnorm_init(True)
    m.eval()
    s = m.spec
    start, C = s.start, s.C
    dims = {"p1_face": C, "p2_face": C, "p1_speech": s.S, "p2_speech": s.S}
    if a.candidates:
        B, ncand = (int(v) for v in a.candidates.split(","))
        text = candidates_report(m, dev, B, ncand, a.passes, a.steps, a.warmup, dims, start, C, torch.cuda.get_device_name(dev), bench, helper)
        bench.stop_smi_helper(helper)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    if a.rollouts:
        B, ncand, n = (int(v) for v in a.rollouts.split(","))
        text = rollouts_report(m, dev, B, ncand, n, a.passes, a.steps, a.warmup, dims, start, C, torch.cuda.get_device_name(dev))
        bench.stop_smi_helper(helper)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    if a.rows:
        text = rows_report(m, dev, [int(v) for v in a.rows.split(",")], a.steps, a.warmup, dims, start, C, torch.cuda.get_device_name(dev))
        bench.stop_smi_helper(helper)
        print(text)
        out = a.out or os.path.join(ROOT, "profiles", "stream_step_rows.md")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    if a.observe_many:
        text = observe_many_report(m, dev, [int(v) for v in a.batches.split(",")], [int(v) for v in a.observe_many.split(",")], a.reps,
                                   dims, start, C, torch.cuda.get_device_name(dev))
        bench.stop_smi_helper(helper)
        print(text)
        out = a.out or os.path.join(ROOT, "profiles", "stream_observe_many.md")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    if a.step_many:
        text = step_many_report(m, dev, [int(v) for v in a.batches.split(",")], [int(v) for v in a.step_many.split(",")], a.reps,
                                dims, start, C, torch.cuda.get_device_name(dev))
        bench.stop_smi_helper(helper)
        print(text)
        out = a.out or os.path.join(ROOT, "profiles", "stream_step_many.md")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    if a.rows_many:
        text = rows_many_report(m, dev, [int(v) for v in a.batches.split(",")], [int(v) for v in a.rows_many.split(",")], a.reps,
                                dims, start, C, torch.cuda.get_device_name(dev))
        bench.stop_smi_helper(helper)
        print(text)
        out = a.out or os.path.join(ROOT, "profiles", "stream_step_rows_many.md")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    if a.observe_ragged:
        text = observe_ragged_report(m, dev, [int(v) for v in a.batches.split(",")], [int(v) for v in a.observe_ragged.split(",")],
                                     a.reps, dims, start, C, torch.cuda.get_device_name(dev), resources)
        bench.stop_smi_helper(helper)
        print(text)
        out = a.out or os.path.join(ROOT, "profiles", "stream_observe_ragged.md")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        return
    batches = [int(v) for v in a.batches.split(",")]
    prefixes = [int(v) for v in a.prefixes.split(",")]
    total = a.warmup + a.steps
    lines = ["# Streaming step latency (tools/stream_latency.py)", "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d, longest history %d), engine precision %s, per-frame "
             "arithmetic picked at the open; %d timed steps after %d warm-up steps per batch size; torch %s, device %s."
             % (C, s.S, s.Ks, s.H, s.D, start, m.precision, a.steps, a.warmup, torch.__version__, torch.cuda.get_device_name(dev)), ""]
    rows, kernels, prefix_rows = [], {}, []
    for B in batches:
        gd = torch.Generator().manual_seed(B)
        T = start + total
        data = {k: torch.randn(B, T, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + n].contiguous() for k, v in data.items() if k != "p1_face"} for n in range(total)]
        noise = (torch.randn(total, B, C, generator=gd) * 0.8).to(dev)
        st = m.open_stream(seed)
        wall, gpu = [], []
        for n in range(total):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            st.step(frames[n], noise[n])
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            if n >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                gpu.append(e0.elapsed_time(e1))
        fp = st.frame_precision
        replays = st.replays
        clk = None
        if B == batches[-1]:
            clk = bench.gpu_state_under_load(lambda i: st.step(frames[i % total], noise[i % total]), dev, helper)
        st.close()
        wall.sort()
        rows.append((B, statistics.median(wall), wall[int(0.9 * (len(wall) - 1))], statistics.median(gpu), fp, replays))
        # per-kernel breakdown: an eager session with the engine's events on
        os.environ["LFI_NO_GRAPH"] = "1"
        eng = m.engine
        st = m.open_stream(seed)
        for n in range(a.warmup):
            st.step(frames[n], noise[n])
        eng.enable_timing(True)
        for n in range(a.warmup, total):
            st.step(frames[n], noise[n])
        kernels[B] = eng.timing_summary()
        eng.enable_timing(False)
        st.close()
        del os.environ["LFI_NO_GRAPH"]
        for t in prefixes:
            if t <= start:
                continue
            pd = {k: (v[:, :start].contiguous() if k == "p1_face" else torch.randn(B, t, dims[k], generator=gd).to(dev))
                  for k, v in data.items()}
            pn = (torch.randn(t - start, B, C, generator=gd) * 0.8).to(dev)
            times = []
            for i in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.inference(t, pd, noise=pn)
                torch.cuda.synchronize()
                if i >= 2:     # (call 1 eager, call 2 captures the per-run graphs)
                    times.append((time.perf_counter() - t0) * 1e3)
            prefix_rows.append((B, t, statistics.median(times)))
        if clk is not None:
            kernels["clock"] = clk
    churn = []
    if a.churn:
        churn = churn_leg(m, dev, a.churn_batch, [int(v) for v in a.churn.split(",")], a.steps, a.warmup, dims, start, C)
    migrate = []
    if a.migrate:
        migrate = churn_leg(m, dev, a.migrate_batch, [int(v) for v in a.migrate.split(",")], a.steps, a.warmup, dims, start, C, migrate=True)
    nll = []
    if a.nll:
        nll = nll_leg(m, dev, [int(v) for v in a.nll.split(",")], a.steps, a.warmup, dims, start, C, a.nll_frames)
    observe = []
    if a.observe:
        observe = observe_leg(m, dev, [int(v) for v in a.observe.split(",")], a.steps, a.warmup, dims, start, C)
    bench.stop_smi_helper(helper)

    lines += ["## One streaming step", "",
              "| B | wall ms, median | wall ms, p90 | GPU ms, median (events around step) | per-frame arithmetic | replayed steps |",
              "|---|---|---|---|---|---|"]
    for B, med, p90, gmed, fp, rep in rows:
        lines.append("| %d | %.3f | %.3f | %.3f | %d | %d of %d |" % (B, med, p90, gmed, fp, rep, total))
    lines += ["", "## Per-kernel breakdown of an eager step (LFI_NO_GRAPH=1, HIP events; mean ms per step)", ""]
    tags = sorted({t for B in batches for t in kernels[B]})
    lines += ["| tag | " + " | ".join("B = %d" % B for B in batches) + " |", "|---|" + "---|" * len(batches)]
    for t in tags:
        lines.append("| %s | " % t + " | ".join("%.3f" % kernels[B][t][1] if t in kernels[B] else "-" for B in batches) + " |")
    lines += ["", "`stream_static` spans the window encoders (`enc_fwd.*`, nested inside it) and the static cond_transform columns; "
              "`stream_chain` is lfi_flow_sample_seq_from for one frame.", "",
              "## Without a session: inference() over the whole prefix for frame t", "",
              "| B | t (frames in total) | ms per call (median of 5, graphs replayed) |", "|---|---|---|"]
    for B, t, ms in prefix_rows:
        lines.append("| %d | %d | %.3f |" % (B, t, ms))
    clk = kernels.get("clock")
    lines += ["", "GPU state under streaming steps at B = %d: %s" % (batches[-1], clk if clk else "not read (no rocm-smi helper)")]
    if churn:
        lines += ["", "## Churn: r rows reseeded before every step (B = %d, --churn)" % a.churn_batch, "",
                  "| r | caller | leg | wall ms, median | wall ms, p90 | GPU ms, median (events) |", "|---|---|---|---|---|---|"]
        for r, caller, leg, med, p90, gmed in churn:
            lines.append("| %d | %s | %s | %.3f | %.3f | %.3f |" % (r, caller, leg, med, p90, gmed))
    if migrate:
        lines += ["", "## Migration: r rows saved and loaded into a second session before every step (B = %d both, --migrate)"
                  % a.migrate_batch, "",
                  "| r | caller | leg | wall ms, median | wall ms, p90 | GPU ms, median (events) |", "|---|---|---|---|---|---|"]
        for r, caller, leg, med, p90, gmed in migrate:
            lines.append("| %d | %s | %s | %.3f | %.3f | %.3f |" % (r, caller, leg, med, p90, gmed))
    if nll:
        lines += ["", "## Likelihood: a session opened with return_nll=True beside one without, step by step (--nll)", "",
                  "| B | leg | wall ms, median | wall ms, p90 | GPU ms, median (events) | GPU ms, p90 |", "|---|---|---|---|---|---|"]
        for B, leg, med, p90, gmed, gp90 in nll:
            lines.append("| %d | %s | %.3f | %.3f | %.3f | %.3f |" % (B, leg, med, p90, gmed, gp90))
    if observe:
        lines += ["", "## Teacher-forced steps: observe() beside step(), session by session, step by step (--observe)", "",
                  "| B | leg | wall ms, median | wall ms, p90 | GPU ms, median (events) | GPU ms, p90 |", "|---|---|---|---|---|---|"]
        for B, leg, med, p90, gmed, gp90 in observe:
            lines.append("| %d | %s | %.3f | %.3f | %.3f | %.3f |" % (B, leg, med, p90, gmed, gp90))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


def churn_leg(m, dev, B, rs, steps, warmup, dims, start, C, migrate=False):
    """Per r and caller: (r, caller, leg, wall median, wall p90, GPU median) for the legs step / reseed + step / reseed, interleaved
    in one session. migrate: the legs step / save + load + step / save + load - r rows of the session saved and loaded into other rows
    of a second session of the same size (which has stepped once) in place of the reseed."""
    import torch
    gd = torch.Generator().manual_seed(B + 1)
    total = warmup + steps
    data = {k: torch.randn(B, start + total, d, generator=gd).to(dev) for k, d in dims.items()}
    seed = {k: v[:, :start].contiguous() for k, v in data.items()}
    frames = [{k: v[:, start + n].contiguous() for k, v in data.items() if k != "p1_face"} for n in range(total)]
    noise = (torch.randn(total, B, C, generator=gd) * 0.8).to(dev)
    joining = {k: torch.randn(max(rs), start, d, generator=gd).to(dev) for k, d in dims.items()}   # the new conversations' seeds
    out = []
    own = torch.cuda.Stream(device=dev)
    for r, caller in [(r, c) for r in rs for c in ("default stream", "own stream")]:
        nseed = {k: v[:r].contiguous() for k, v in joining.items()}
        order = torch.randperm(B, generator=gd).tolist()
        move = "save + load" if migrate else "reseed"
        legs = {"step": ([], []), move + " + step": ([], []), move: ([], [])}
        own.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(own if caller == "own stream" else torch.cuda.current_stream(dev)), m.open_stream(seed) as st, \
                contextlib.ExitStack() as stack:
            if migrate:
                st2 = stack.enter_context(m.open_stream(seed))
                st2.step(frames[0], noise[0])
            for n in range(total):
                rows = [order[(n * r + j) % B] for j in range(r)]
                for leg, (wall, gpu) in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    if leg != "step" and migrate:
                        st2.load_rows([(b + 1) % B for b in rows], st.save_rows(rows))
                    elif leg != "step":
                        st.reset_rows(rows, nseed)
                    if leg != move:
                        st.step(frames[n], noise[n])
                    e1.record()
                    e1.synchronize()
                    t1 = time.perf_counter()
                    if n >= warmup:
                        wall.append((t1 - t0) * 1e3)
                        gpu.append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        for leg, (wall, gpu) in legs.items():
            wall.sort()
            out.append((r, caller, leg, statistics.median(wall), wall[int(0.9 * (len(wall) - 1))], statistics.median(gpu)))
    return out


def nll_leg(m, dev, batches, steps, warmup, dims, start, C, nframes=0):
    """Per batch size: (B, leg, wall median, wall p90, GPU median, GPU p90) of a step without and with return_nll, two sessions
    interleaved step by step (which of the two goes first alternates), then of inference() over nframes generated frames likewise."""
    import torch
    out = []
    total = warmup + steps
    for B in batches:
        gd = torch.Generator().manual_seed(B + 2)
        data = {k: torch.randn(B, start + total, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + n].contiguous() for k, v in data.items() if k != "p1_face"} for n in range(total)]
        noise = (torch.randn(total, B, C, generator=gd) * 0.8).to(dev)
        legs = {"step": ([], []), "step, return_nll": ([], [])}

        def timed(fn, wall, gpu, keep):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            if keep:
                wall.append((t1 - t0) * 1e3)
                gpu.append(e0.elapsed_time(e1))

        with m.open_stream(seed) as off, m.open_stream(seed, return_nll=True) as on:
            sessions = {"step": off, "step, return_nll": on}
            for n in range(total):
                for leg in (list(legs) if n % 2 == 0 else list(legs)[::-1]):
                    timed(lambda: sessions[leg].step(frames[n], noise[n]), *legs[leg], n >= warmup)
        if nframes > 0:
            t = start + nframes
            pd = {k: (v[:, :start].contiguous() if k == "p1_face" else torch.randn(B, t, dims[k], generator=gd).to(dev))
                  for k, v in data.items()}
            pn = (torch.randn(nframes, B, C, generator=gd) * 0.8).to(dev)
            calls = {"inference, %d frames" % nframes: False, "inference, %d frames, return_nll" % nframes: True}
            for leg in calls:
                legs[leg] = ([], [])
            for i in range(12):          # (a flip of the flag recaptures: each leg's graphs are made on its second call in a row)
                for leg, flag in (list(calls.items()) if i % 2 == 0 else list(calls.items())[::-1]):
                    for j in range(3):
                        timed(lambda: m.inference(t, pd, noise=pn, return_nll=flag), *legs[leg], i >= 2 and j == 2)
        for leg, (wall, gpu) in legs.items():
            wall.sort()
            gpu.sort()
            out.append((B, leg, statistics.median(wall), wall[int(0.9 * (len(wall) - 1))], statistics.median(gpu),
                        gpu[int(0.9 * (len(gpu) - 1))]))
    return out


def observe_leg(m, dev, batches, steps, warmup, dims, start, C):
    """Per batch size: (B, leg, wall median, wall p90, GPU median, GPU p90) of step(), observe() and observe(return_z=True): three
    sessions on one seed, interleaved step by step, the order rotating. The faces observed are those of an untimed generating
    session run first with the same noise (so every session sees the same sequence)."""
    import torch
    out = []
    total = warmup + steps
    for B in batches:
        gd = torch.Generator().manual_seed(B + 3)
        data = {k: torch.randn(B, start + total, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + n].contiguous() for k, v in data.items() if k != "p1_face"} for n in range(total)]
        noise = (torch.randn(total, B, C, generator=gd) * 0.8).to(dev)
        with m.open_stream(seed) as ref:
            faces = [ref.step(frames[n], noise[n]) for n in range(total)]
        with m.open_stream(seed) as gen, m.open_stream(seed) as obs, m.open_stream(seed) as obz:
            calls = [("step", lambda n: gen.step(frames[n], noise[n])),
                     ("observe", lambda n: obs.observe(frames[n], faces[n])),
                     ("observe, return_z", lambda n: obz.observe(frames[n], faces[n], return_z=True))]
            legs = {name: ([], []) for name, _ in calls}
            for n in range(total):
                for name, fn in calls[n % 3:] + calls[:n % 3]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    fn(n)
                    e1.record()
                    e1.synchronize()
                    t1 = time.perf_counter()
                    if n >= warmup:
                        legs[name][0].append((t1 - t0) * 1e3)
                        legs[name][1].append(e0.elapsed_time(e1))
        for leg, (wall, gpu) in legs.items():
            wall.sort()
            gpu.sort()
            out.append((B, leg, statistics.median(wall), wall[int(0.9 * (len(wall) - 1))], statistics.median(gpu),
                        gpu[int(0.9 * (len(gpu) - 1))]))
    return out


def rows_leg(m, dev, batches, steps, warmup, dims, start, C):
    """Per batch size: (B, leg, wall median, wall p90, GPU p10, GPU median, GPU p90) of the legs the module's docstring lists under
    --rows, on a stream of the caller's own, interleaved step by step with the order rotating. The faces observed are those of an
    untimed generating session run first with the same noise."""
    import torch
    out = []
    total = warmup + steps
    own = torch.cuda.Stream(device=dev)
    for B in batches:
        gd = torch.Generator().manual_seed(B + 4)
        data = {k: torch.randn(B, start + total, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + n].contiguous() for k, v in data.items() if k != "p1_face"} for n in range(total)]
        noise = (torch.randn(total, B, C, generator=gd) * 0.8).to(dev)
        h = B // 2
        lo = lambda x: x[:h].contiguous()
        hi = lambda x: x[h:].contiguous()
        rows = torch.arange(B, device=dev)
        masks = {"all generate": rows < 0, "all observe": rows >= 0, "tile-aligned halves": (rows // 16) < (B // 32),
                 "interleaved in every tile": rows % 2 == 1}
        own.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(own), contextlib.ExitStack() as stack:
            opened = lambda sd, **kw: stack.enter_context(m.open_stream(sd, **kw))
            with m.open_stream(seed) as ref:
                faces = [ref.step(frames[n], noise[n]) for n in range(total)]
            gen, obs = opened(seed, return_nll=True), opened(seed)
            calls = [("(a) step(return_nll=True)", lambda n: gen.step(frames[n], noise[n])),
                     ("(a) observe()", lambda n: obs.observe(frames[n], faces[n]))]

            def rows_call(tag, mask):
                st = opened(seed)
                return (tag, lambda n: st.step_rows(frames[n], faces[n], mask, noise[n]))

            calls += [rows_call("(b) step_rows, all generate", masks["all generate"]),
                      rows_call("(b) step_rows, all observe", masks["all observe"])]
            if B >= 32:
                calls.append(rows_call("(c) step_rows, tile-aligned halves", masks["tile-aligned halves"]))
            if B >= 2:
                calls.append(rows_call("(d) step_rows, interleaved in every tile", masks["interleaved in every tile"]))
                seed_lo, seed_hi = {k: lo(v) for k, v in seed.items()}, {k: hi(v) for k, v in seed.items()}
                fr_lo = [{k: lo(v) for k, v in f.items()} for f in frames]
                fr_hi = [{k: hi(v) for k, v in f.items()} for f in frames]
                nz_lo, fc_hi = [lo(z) for z in noise], [hi(f) for f in faces]
                two_g, two_o = opened(seed_lo), opened(seed_hi)

                def two(n):
                    two_g.step(fr_lo[n], nz_lo[n])
                    two_o.observe(fr_hi[n], fc_hi[n])
                calls.append(("(e) step() on %d rows, then observe() on %d rows: two sessions" % (h, B - h), two))
            legs = {name: ([], []) for name, _ in calls}
            k = len(calls)
            for n in range(total):
                for name, fn in calls[n % k:] + calls[:n % k]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    fn(n)
                    e1.record()
                    e1.synchronize()
                    t1 = time.perf_counter()
                    if n >= warmup:
                        legs[name][0].append((t1 - t0) * 1e3)
                        legs[name][1].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        for leg, (wall, gpu) in legs.items():
            wall.sort()
            gpu.sort()
            q = lambda v, f: v[int(f * (len(v) - 1))]
            out.append((B, leg, statistics.median(wall), q(wall, 0.9), q(gpu, 0.1), statistics.median(gpu), q(gpu, 0.9)))
    return out


def rows_report(m, dev, batches, steps, warmup, dims, start, C, device_name):
    """The --rows report: the table, then the two conditions of the feature read off it."""
    s = m.spec
    got = rows_leg(m, dev, batches, steps, warmup, dims, start, C)
    lines = ["# step_rows(): generating and observing rows in one step (tools/stream_latency.py --rows)", "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; caller on its own stream; every "
             "leg of a batch size interleaved step by step in one process, the order rotating; %d timed steps after %d warm-up steps; "
             "wall = step to result on the host (a synchronise after every call), GPU = HIP events around the call. Device %s."
             % (C, s.S, s.Ks, s.H, s.D, m.precision, steps, warmup, device_name), "",
             "| B | leg | wall ms, median | wall ms, p90 | GPU ms, p10 | GPU ms, median | GPU ms, p90 |", "|---|---|---|---|---|---|---|"]
    table = {}
    for B, leg, med, p90, g10, gmed, g90 in got:
        lines.append("| %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f |" % (B, leg, med, p90, g10, gmed, g90))
        table[(B, leg[:3])] = table.get((B, leg[:3]), []) + [(leg, med, g10, gmed, g90)]
    lines += ["", "## The two conditions", ""]
    for B in batches:
        a, b = table.get((B, "(a)"), []), table.get((B, "(b)"), [])
        for (pl, pw, p10, pg, p90), (rl, rw, _, rg, _) in zip(a, b):
            lines.append("- B = %d: %s %.3f ms GPU (%.3f wall) against %s %.3f (%.3f): %+.3f ms GPU, %+.3f ms wall; the pure leg's own "
                         "p10 .. p90 spread is %.3f ms GPU." % (B, rl[4:], rg, rw, pl[4:], pg, pw, rg - pg, rw - pw, p90 - p10))
        c, e = table.get((B, "(c)")), table.get((B, "(e)"))
        if c and e:
            lines.append("- B = %d: (c) tile-aligned halves %.3f ms GPU (%.3f wall) against (e) two sessions of %d rows %.3f (%.3f): "
                         "step_rows %s." % (B, c[0][3], c[0][1], B // 2, e[0][3], e[0][1],
                                            "is faster" if c[0][1] < e[0][1] and c[0][3] < e[0][3] else "is NOT faster"))
        d = table.get((B, "(d)"))
        if c and d:
            lines.append("- B = %d: (d) roles interleaved inside every tile %.3f ms GPU (%.3f wall): %.2f x the tile-aligned step."
                         % (B, d[0][3], d[0][1], d[0][3] / c[0][3]))
    return "\n".join(lines) + "\n"


def observe_many_report(m, dev, batches, ns, reps, dims, start, C, device_name):
    """The --observe-many report: per (B, n) the per-frame time of the observe() loop and of observe_many(n), then where a chunk
    call's GPU time goes."""
    import torch
    s = m.spec
    eng = m._ensure_engine(dev)
    top = max(ns)
    lines = ["# observe_many(): a chunk of recorded frames per call (tools/stream_latency.py --observe-many)", "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; both legs of a (B, n) in one "
             "process, alternating which goes first; %d timed rounds after 2 untimed ones; per FRAME: wall = call to result on the host "
             "(one synchronise after the n calls / the one call) / n, GPU = HIP events around them / n. Device %s."
             % (C, s.S, s.Ks, s.H, s.D, m.precision, reps, device_name), "",
             "| B | n | observe() loop: wall ms / frame | GPU ms / frame | observe_many: wall ms / frame | GPU ms / frame | "
             "loop / chunk, wall | frames per launch |", "|---|---|---|---|---|---|---|---|"]
    split = []
    for B in batches:
        gd = torch.Generator().manual_seed(B + 5)
        data = {k: torch.randn(B, start + top + 1, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + i].contiguous() for k, v in data.items() if k != "p1_face"} for i in range(top + 1)]
        noise = (torch.randn(top + 1, B, C, generator=gd) * 0.8).to(dev)
        with m.open_stream(seed) as ref:
            faces = [ref.step(frames[i], noise[i]) for i in range(top + 1)]
        clip = torch.stack(faces, 1)
        with m.open_stream(seed) as loop, m.open_stream(seed) as many:
            for n in ns:
                chunk = {k: v[:, start + 1:start + 1 + n].contiguous() for k, v in data.items() if k != "p1_face"}
                cfaces = clip[:, 1:1 + n].contiguous()
                calls = [("loop", loop, lambda: [loop.observe(frames[i], faces[i]) for i in range(1, n + 1)]),
                         ("many", many, lambda: many.observe_many(chunk, cfaces))]
                legs = {"loop": ([], []), "many": ([], [])}
                for r in range(reps + 2):
                    for name, st, fn in (calls if r % 2 == 0 else calls[::-1]):
                        st.reset(seed)
                        st.observe(frames[0], faces[0])
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        t1 = time.perf_counter()
                        if r >= 2:
                            legs[name][0].append((t1 - t0) * 1e3 / n)
                            legs[name][1].append(e0.elapsed_time(e1) / n)
                lw, lg, mw, mg = (statistics.median(v) for v in legs["loop"] + legs["many"])
                lines.append("| %d | %d | %.4f | %.4f | %.4f | %.4f | %.2f x | %d |" % (B, n, lw, lg, mw, mg, lw / mw, min(n, many._chunk_cap())))
                many.reset(seed)
                many.observe(frames[0], faces[0])
                eng.enable_timing(True)
                many.observe_many(chunk, cfaces)
                summary = eng.timing_summary()
                eng.enable_timing(False)
                parts = {t: v[0] * v[1] for t, v in summary.items() if t.startswith("stream_chunk")}
                # the two parts of the chain entry point, each alone (LFI_CHUNK_ONLY, a diagnostic of lfi_flow_score_seq_chunk): the
                # chain first, on the gic the whole call above left in the work area
                for part in ("chain", "front"):
                    os.environ["LFI_CHUNK_ONLY"] = part
                    try:
                        eng.enable_timing(True)
                        many.observe_many(chunk, cfaces)
                        got = eng.timing_summary().get("stream_chunk_chain")
                    finally:
                        eng.enable_timing(False)
                        del os.environ["LFI_CHUNK_ONLY"]
                    parts[part] = got[0] * got[1] if got else 0.0
                split.append((B, n, parts))
    lines += ["", "## Where a chunk call's GPU time goes (enable_timing, HIP events; ms per call, all its launches of a kind summed)", "",
              "| B | n | windows in | static part (window encoders + static cond_transform columns) | front end + chain, one call | "
              "front end alone (gather, encoded kinds, window product, gic) | chain alone (one launch) | chain share of the call |",
              "|---|---|---|---|---|---|---|---|"]
    for B, n, t in split:
        a, b, c = (t.get("stream_chunk_" + k, 0.0) for k in ("in", "static", "chain"))
        lines.append("| %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.0f %% |"
                     % (B, n, a, b, c, t["front"], t["chain"], 100.0 * t["chain"] / max(a + b + c, 1e-9)))
    return "\n".join(lines) + "\n"


def step_many_report(m, dev, batches, ns, reps, dims, start, C, device_name):
    """The --step-many report: per (B, n) the per-frame time of the step() loop and of step_many(n), then where a step_many call's GPU
    time goes."""
    import torch
    s = m.spec
    eng = m._ensure_engine(dev)
    top = max(ns)
    lines = ["# step_many(): several generated frames per call (tools/stream_latency.py --step-many)", "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; both legs of a (B, n) in one "
             "process on the same conditioning and noise, alternating which goes first; %d timed rounds after 2 untimed ones; per "
             "FRAME: wall = call to result on the host (one synchronise after the n calls / the one call) / n, GPU = HIP events around "
             "them / n. Device %s." % (C, s.S, s.Ks, s.H, s.D, m.precision, reps, device_name), "",
             "| B | n | step() loop: wall ms / frame | GPU ms / frame | step_many: wall ms / frame | GPU ms / frame | loop / call, wall | "
             "loop / call, GPU | frames per round |", "|---|---|---|---|---|---|---|---|---|"]
    split, slower = [], []
    for B in batches:
        gd = torch.Generator().manual_seed(B + 7)
        data = {k: torch.randn(B, start + top + 1, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + i].contiguous() for k, v in data.items() if k != "p1_face"} for i in range(top + 1)]
        noise = (torch.randn(top + 1, B, C, generator=gd) * 0.8).to(dev)
        with m.open_stream(seed) as loop, m.open_stream(seed) as many:
            for n in ns:
                chunk = {k: v[:, start + 1:start + 1 + n].contiguous() for k, v in data.items() if k != "p1_face"}
                cnoise = noise[1:1 + n]
                calls = [("loop", loop, lambda: [loop.step(frames[i], noise[i]) for i in range(1, n + 1)]),
                         ("many", many, lambda: many.step_many(chunk, cnoise))]
                legs = {"loop": ([], []), "many": ([], [])}
                for r in range(reps + 2):
                    for name, st, fn in (calls if r % 2 == 0 else calls[::-1]):
                        st.reset(seed)
                        st.step(frames[0], noise[0])
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        t1 = time.perf_counter()
                        if r >= 2:
                            legs[name][0].append((t1 - t0) * 1e3 / n)
                            legs[name][1].append(e0.elapsed_time(e1) / n)
                lw, lg, mw, mg = (statistics.median(v) for v in legs["loop"] + legs["many"])
                lines.append("| %d | %d | %.4f | %.4f | %.4f | %.4f | %.2f x | %.2f x | %d |"
                             % (B, n, lw, lg, mw, mg, lw / mw, lg / mg, min(n, many._chunk_cap())))
                if n == 16 and not (mw < lw and mg < lg):
                    slower.append(B)
                many.reset(seed)
                many.step(frames[0], noise[0])
                eng.enable_timing(True)
                many.step_many(chunk, cnoise)
                summary = eng.timing_summary()
                eng.enable_timing(False)
                split.append((B, n, {t: v[0] * v[1] for t, v in summary.items() if t.startswith("stream_chunk")}))
    lines += ["", "Per-frame time of step_many(16) below the same run's step() loop at every batch size: %s."
              % ("yes" if not slower else "NO, not at B = %s" % slower), "",
              "## Where a step_many call's GPU time goes (enable_timing, HIP events; ms per call, all its launches of a kind summed)", "",
              "| B | n | windows in | static part (window encoders + static cond_transform columns) | sampler: n front ends + n chains | "
              "sampler per frame | sampler share of the call |", "|---|---|---|---|---|---|---|"]
    for B, n, t in split:
        a, b, c = (t.get("stream_chunk_" + k, 0.0) for k in ("in", "static", "gen_chain"))
        lines.append("| %d | %d | %.3f | %.3f | %.3f | %.4f | %.0f %% |" % (B, n, a, b, c, c / n, 100.0 * c / max(a + b + c, 1e-9)))
    return "\n".join(lines) + "\n"


def rows_many_report(m, dev, batches, ns, reps, dims, start, C, device_name):
    """The --rows-many report: per (B, n) the per-frame time of the step_rows() loop and of step_rows_many(n) under the masks the
    module's docstring lists, then where the prompt-then-continue call's GPU time goes with the plan on and off."""
    import torch
    s = m.spec
    eng = m._ensure_engine(dev)
    top = max(ns)
    switch = "LFI_ROWS_MANY_OBSERVE_RUN"
    arms = ("loop", "halves", "mixed", "prompt", "prompt, plan off")
    lines = ["# step_rows_many(): per-row roles over a chunk of frames (tools/stream_latency.py --rows-many)", "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; every arm of a (B, n) in one "
             "process on a session of its own, the same conditioning, faces and noise, the order rotating; %d timed rounds after 2 "
             "untimed ones; per FRAME: wall = call to result on the host (one synchronise after the n calls / the one call) / n, GPU = "
             "HIP events around them / n; wall / GPU in every cell. Device %s." % (C, s.S, s.Ks, s.H, s.D, m.precision, reps, device_name),
             "", "Masks: halves = the first half of the 16-row tiles observes, the rest generates (B >= 32); mixed = odd rows observe, "
             "even rows generate, every tile mixed (B = 1: the row alternates frame by frame); prompt = row b observes its first "
             "lengths[b] frames and generates the rest, lengths spread over n / 4 .. 3 n / 4, with the plan on (runs every row observes "
             "go to the chunk forward chain) and with %s=0 (everything on the rows chain). The step_rows() loop runs the halves mask "
             "where there is one (its cheaper case: one chain per tile), the mixed mask below B = 32." % switch, "",
             "| B | n | step_rows() loop, ms / frame | step_rows_many: halves | mixed | prompt | prompt, plan off | loop / halves, GPU | "
             "loop / mixed, GPU | plan off / on, GPU | plan of the prompt call |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    split, slower, plan_slower = [], [], []
    for B in batches:
        gd = torch.Generator().manual_seed(B + 11)
        data = {k: torch.randn(B, start + top + 1, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + i].contiguous() for k, v in data.items() if k != "p1_face"} for i in range(top + 1)]
        noise = (torch.randn(top + 1, B, C, generator=gd) * 0.8).to(dev)
        given = (torch.randn(B, top + 1, C, generator=gd) * 0.5).to(dev)
        face = [given[:, i].contiguous() for i in range(top + 1)]
        tiles = (B + 15) // 16
        sessions = {name: m.open_stream(seed) for name in arms}
        try:
            for n in ns:
                chunk = {k: v[:, start + 1:start + 1 + n].contiguous() for k, v in data.items() if k != "p1_face"}
                cnoise, cfaces = noise[1:1 + n], given[:, 1:1 + n].contiguous()
                halves = (torch.arange(B) // 16 < tiles // 2).expand(n, B).contiguous() if B >= 32 else None
                mixed = ((torch.arange(B) % 2 == 1).expand(n, B) if B >= 2 else (torch.arange(n) % 2 == 1)[:, None]).contiguous()
                lengths = torch.tensor([n // 4 + (b * (n // 2)) // max(B - 1, 1) for b in range(B)]) if B > 1 else torch.tensor([n // 2])
                prompt = torch.arange(n)[:, None] < lengths[None, :]
                loop_mask = (halves if halves is not None else mixed).tolist()

                def many(name, mask, off=False):
                    def call():
                        if off:
                            os.environ[switch] = "0"
                        try:
                            return sessions[name].step_rows_many(chunk, cfaces, mask, cnoise)
                        finally:
                            os.environ.pop(switch, None)
                    return call

                def loop():
                    st = sessions["loop"]
                    return [st.step_rows(frames[i], face[i], loop_mask[i - 1], noise[i]) for i in range(1, n + 1)]

                calls = [("loop", loop), ("mixed", many("mixed", mixed)), ("prompt", many("prompt", prompt)),
                         ("prompt, plan off", many("prompt, plan off", prompt, True))]
                if halves is not None:
                    calls.insert(1, ("halves", many("halves", halves)))
                legs = {name: ([], []) for name, _ in calls}
                for r in range(reps + 2):
                    k = r % len(calls)
                    for name, fn in calls[k:] + calls[:k]:
                        st = sessions[name]
                        st.reset(seed)
                        st.step(frames[0], noise[0])
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        t1 = time.perf_counter()
                        if r >= 2:
                            legs[name][0].append((t1 - t0) * 1e3 / n)
                            legs[name][1].append(e0.elapsed_time(e1) / n)
                med = {name: (statistics.median(w), statistics.median(g)) for name, (w, g) in legs.items()}
                cell = lambda name: "%.4f / %.4f" % med[name] if name in med else "-"
                ratio = lambda a, b: "%.2f x" % (med[a][1] / med[b][1]) if a in med and b in med else "-"
                plan = sessions["prompt"].last_plan
                lines.append("| %d | %d | %s | %s | %s | %s | %s | %s | %s | %s | %s |"
                             % (B, n, cell("loop"), cell("halves"), cell("mixed"), cell("prompt"), cell("prompt, plan off"),
                                ratio("loop", "halves"), ratio("loop", "mixed"), ratio("prompt, plan off", "prompt"),
                                " ".join("%s %d+%d" % run for run in plan)))
                if n == 16 and not all(med[name][0] < med["loop"][0] and med[name][1] < med["loop"][1] for name in med if name != "loop"):
                    slower.append(B)
                if med["prompt"][1] > med["prompt, plan off"][1]:
                    plan_slower.append((B, n))
                for name, off in (("prompt", False), ("prompt, plan off", True)):
                    st = sessions[name]
                    st.reset(seed)
                    st.step(frames[0], noise[0])
                    eng.enable_timing(True)
                    many(name, prompt, off)()
                    summary = eng.timing_summary()
                    eng.enable_timing(False)
                    split.append((B, n, name, {t: v[0] * v[1] for t, v in summary.items() if t.startswith("stream_chunk")}))
        finally:
            for st in sessions.values():
                st.close()
    lines += ["", "Per-frame time of step_rows_many(16), every mask, below the same run's step_rows() loop at every batch size (wall "
              "and GPU): %s." % ("yes" if not slower else "NO, not at B = %s" % slower),
              "The prompt mask with the plan on not slower than with it off (GPU, medians): %s."
              % ("yes, at every (B, n)" if not plan_slower else "NO, slower at (B, n) = %s" % plan_slower), "",
              "## Where a prompt-then-continue call's GPU time goes (enable_timing, HIP events; ms per call, all its launches of a kind summed)",
              "", "| B | n | arm | role words + windows in | static part (window encoders + static cond_transform columns) | the plan's runs: "
              "front ends + chains | runs per frame |", "|---|---|---|---|---|---|---|"]
    for B, n, name, t in split:
        a, b, c = (t.get("stream_chunk_" + k, 0.0) for k in ("in", "static", "rows_chain"))
        lines.append("| %d | %d | %s | %.3f | %.3f | %.3f | %.4f |" % (B, n, name, a, b, c, c / n))
    return "\n".join(lines) + "\n"


def candidates_report(m, dev, B, ncand, passes, steps, warmup, dims, start, C, device_name, bench, helper):
    """The --candidates report: per pass the median frame of step_candidates + commit() and of the save / load / step / save / load
    recipe, alternated as whole passes; then the timer split of both arms on eager sessions."""
    import torch
    s = m.spec
    eng = m._ensure_engine(dev)
    V, total = B * ncand, warmup + steps
    gd = torch.Generator().manual_seed(B * 1000 + ncand)
    data = {k: torch.randn(B, start + total, d, generator=gd).to(dev) for k, d in dims.items()}
    seed = {k: v[:, :start].contiguous() for k, v in data.items()}
    frames = [{k: v[:, start + n].contiguous() for k, v in data.items() if k != "p1_face"} for n in range(total)]
    noise = (torch.randn(total, B, ncand, C, generator=gd) * 0.8).to(dev)
    # the recipe's session: every conversation's seed, conditioning and noise in ncand neighbouring rows
    seed_v = {k: v.repeat_interleave(ncand, 0).contiguous() for k, v in seed.items()}
    frames_v = [{k: v.repeat_interleave(ncand, 0).contiguous() for k, v in f.items()} for f in frames]
    noise_v = noise.view(total, V, C)
    home, every, parent = [r * ncand for r in range(B)], list(range(V)), [v // ncand for v in range(V)]
    base = torch.tensor(home, device=dev)

    def new_frame(st, n):
        st.step_candidates(frames[n], ncand, noise[n])
        return st.commit()[0]

    def recipe_frame(st, n):
        st.load_rows(every, st.save_rows(home), parent)
        out, nll = st.step(frames_v[n], noise_v[n])
        win = (base + nll.view(B, ncand).argmin(1)).tolist()        # (the arg-min on the host side: the row lists are host data)
        st.load_rows(home, st.save_rows(win))
        return out[win]

    def run(st, frame_fn, timed=True):
        wall, gpu = [], []
        for n in range(total):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            frame_fn(st, n)
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            if n >= warmup:
                wall.append((t1 - t0) * 1e3)
                gpu.append(e0.elapsed_time(e1))
        return statistics.median(wall), statistics.median(gpu)

    series = {"recipe": [], "new": []}
    with m.open_stream(seed) as st_new, m.open_stream(seed_v, return_nll=True) as st_old:
        arms = (("recipe", st_old, seed_v, recipe_frame), ("new", st_new, seed, new_frame))
        for p in range(passes):
            for name, st, sd, fn in arms:
                st.reset(sd)
                series[name].append(run(st, fn))
        st_new.reset(seed)
        clk = bench.gpu_state_under_load(lambda i: new_frame(st_new, i % total), dev, helper)
    # the timer split: eager sessions, the engine's events on
    os.environ["LFI_NO_GRAPH"] = "1"
    split = {}
    for name, sd, fn, nll in (("recipe", seed_v, recipe_frame, True), ("new", seed, new_frame, False)):
        with m.open_stream(sd, return_nll=nll) as st:
            for n in range(warmup):
                fn(st, n)
            eng.enable_timing(True)
            for n in range(warmup, total):
                fn(st, n)
            split[name] = eng.timing_summary()
            eng.enable_timing(False)
    del os.environ["LFI_NO_GRAPH"]
    lines = ["# Best-of-N per frame: step_candidates + commit() against the save / load recipe (tools/stream_latency.py --candidates %d,%d)"
             % (B, ncand), "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; B = %d conversations, ncand = %d "
             "candidates per frame (the recipe's session has %d rows); %d whole passes per arm, alternated, the recipe first; a pass is "
             "the median of %d timed frames after %d untimed ones. wall = call to result on the host (a synchronise after the frame), "
             "GPU = HIP events around the frame. Device %s." % (C, s.S, s.Ks, s.H, s.D, m.precision, B, ncand, V, passes, steps, warmup,
                                                                 device_name), "",
             "| pass | recipe: wall ms / frame | recipe: GPU ms / frame | new: wall ms / frame | new: GPU ms / frame |", "|---|---|---|---|---|"]
    for p in range(passes):
        (rw, rg), (nw, ng) = series["recipe"][p], series["new"][p]
        lines.append("| %d | %.4f | %.4f | %.4f | %.4f |" % (p + 1, rw, rg, nw, ng))
    for i, what in ((0, "wall"), (1, "GPU")):
        new_med = statistics.median(v[i] for v in series["new"])
        low = min(v[i] for v in series["recipe"])
        lines += ["", "%s: the new calls' median over the passes %.4f ms, the recipe's lowest pass %.4f ms (%.2f x): %s."
                  % (what, new_med, low, low / new_med, "below it" if new_med < low else "NOT below it")]
    lines += ["", "## Timer split of an eager frame (LFI_NO_GRAPH=1, HIP events; mean ms per launch x launches per frame)", "",
              "| tag | recipe | new |", "|---|---|---|"]
    for t in sorted(set(split["recipe"]) | set(split["new"])):
        if t.startswith("stream_"):
            lines.append("| %s | " % t + " | ".join("%.4f x %.0f" % (split[k][t][1], split[k][t][0] / steps) if t in split[k] else "-"
                                                    for k in ("recipe", "new")) + " |")
    lines += ["", "`stream_static`: window encoders + static cond_transform columns (%d windows in the recipe, %d in the new calls); "
              "`stream_chain`: front end + reverse chain (lfi_flow_sample_seq_nll over %d rows; lfi_flow_sample_cand_from: front end for %d "
              "rows, chain over %d virtual rows). The save / load launches of the recipe and the commit launch carry no timer: they are "
              "the rest of the frame's GPU time." % (V, B, V, B, V), "",
              "GPU state under the new calls' load: %s" % (clk if clk else "not read (no rocm-smi helper)")]
    return "\n".join(lines) + "\n"


def rollouts_report(m, dev, B, ncand, n, passes, steps, warmup, dims, start, C, device_name):
    """The --rollouts report: per pass the median rollout of rollout_candidates + commit() and of the save / load / step_many / save /
    load recipe, per committed frame, alternated as whole passes; then where the new calls' GPU time goes."""
    import torch
    s = m.spec
    eng = m._ensure_engine(dev)
    V, total = B * ncand, warmup + steps
    gd = torch.Generator().manual_seed(B * 1000 + ncand * 10 + n)
    # every rollout runs under the same n frames of conditioning and its own draws, from wherever the last commit left the session
    data = {k: torch.randn(B, start + n, d, generator=gd).to(dev) for k, d in dims.items()}
    seed = {k: v[:, :start].contiguous() for k, v in data.items()}
    frames = {k: v[:, start:].contiguous() for k, v in data.items() if k != "p1_face"}
    noise = (torch.randn(8, n, B, ncand, C, generator=gd) * 0.8).to(dev)
    seed_v = {k: v.repeat_interleave(ncand, 0).contiguous() for k, v in seed.items()}
    frames_v = {k: v.repeat_interleave(ncand, 0).contiguous() for k, v in frames.items()}
    noise_v = noise.view(8, n, V, C)
    home, every, parent = [r * ncand for r in range(B)], list(range(V)), [v // ncand for v in range(V)]
    base = torch.tensor(home, device=dev)

    def new_rollout(st, i):
        st.rollout_candidates(frames, ncand, noise[i % 8])
        return st.commit()[0]

    def recipe_rollout(st, i):
        st.load_rows(every, st.save_rows(home), parent)
        out, nll = st.step_many(frames_v, noise_v[i % 8])
        tot = nll[0].clone()
        for f in range(1, n):
            tot += nll[f]
        win = (base + tot.view(B, ncand).argmin(1)).tolist()        # (the arg-min on the host side: the row lists are host data)
        st.load_rows(home, st.save_rows(win))
        return out[win]

    def run(st, fn):
        wall, gpu = [], []
        for i in range(total):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn(st, i)
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            if i >= warmup:
                wall.append((t1 - t0) * 1e3 / n)
                gpu.append(e0.elapsed_time(e1) / n)
        return statistics.median(wall), statistics.median(gpu)

    series = {"recipe": [], "new": []}
    with m.open_stream(seed) as st_new, m.open_stream(seed_v, return_nll=True) as st_old:
        arms = (("recipe", st_old, seed_v, recipe_rollout), ("new", st_new, seed, new_rollout))
        for p in range(passes):
            for name, st, sd, fn in arms:
                st.reset(sd)
                series[name].append(run(st, fn))
        # where the new calls' GPU time goes: the engine's events around every group of launches
        st_new.reset(seed)
        for i in range(3):
            new_rollout(st_new, i)
        eng.enable_timing(True)
        for i in range(steps):
            new_rollout(st_new, i)
        split = eng.timing_summary()
        eng.enable_timing(False)
        # the front end alone (LFI_CHUNK_ONLY=front: no chain is launched; what the call returns is not meaningful and is dropped)
        os.environ["LFI_CHUNK_ONLY"] = "front"
        try:
            eng.enable_timing(True)
            for i in range(steps):
                st_new.rollout_candidates(frames, ncand, noise[i % 8])
                st_new.discard()
            front = eng.timing_summary().get("stream_rollout_chain")
        finally:
            eng.enable_timing(False)
            del os.environ["LFI_CHUNK_ONLY"]
        # the recipe's static part and chain, the same way
        st_old.reset(seed_v)
        for i in range(3):
            recipe_rollout(st_old, i)
        eng.enable_timing(True)
        for i in range(steps):
            recipe_rollout(st_old, i)
        split_old = eng.timing_summary()
        eng.enable_timing(False)
    lines = ["# Best-of-N over n frames: rollout_candidates + commit() against the save / load recipe (tools/stream_latency.py --rollouts "
             "%d,%d,%d)" % (B, ncand, n), "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; B = %d conversations, ncand = %d "
             "candidates of n = %d frames (the recipe's session has %d rows); %d whole passes per arm, alternated, the recipe first; a "
             "pass is the median of %d timed rollouts after %d untimed ones, divided by n: ms per COMMITTED frame. wall = call to result "
             "on the host (a synchronise after the rollout), GPU = HIP events around it. Device %s."
             % (C, s.S, s.Ks, s.H, s.D, m.precision, B, ncand, n, V, passes, steps, warmup, device_name), "",
             "| pass | recipe: wall ms / frame | recipe: GPU ms / frame | new: wall ms / frame | new: GPU ms / frame |", "|---|---|---|---|---|"]
    for p in range(passes):
        (rw, rg), (nw, ng) = series["recipe"][p], series["new"][p]
        lines.append("| %d | %.4f | %.4f | %.4f | %.4f |" % (p + 1, rw, rg, nw, ng))
    for i, what in ((0, "wall"), (1, "GPU")):
        new_med = statistics.median(v[i] for v in series["new"])
        low = min(v[i] for v in series["recipe"])
        lines += ["", "%s: the new calls' median over the passes %.4f ms, the recipe's lowest pass %.4f ms (%.2f x): %s."
                  % (what, new_med, low, low / new_med, "below it" if new_med < low else "NOT below it")]

    def per_call(summary, tag):
        v = summary.get(tag)
        return v[0] * v[1] / steps if v else 0.0

    both = per_call(split, "stream_rollout_chain")
    fr = front[0] * front[1] / steps if front else 0.0
    lines += ["", "## Where a rollout's GPU time goes (enable_timing, HIP events; ms per call of n = %d frames, a kind's launches summed)" % n, "",
              "| part | new: rollout_candidates + commit | recipe: step_many over %d rows |" % V, "|---|---|---|",
              "| windows in (lfi_stream_chunk_gen_in) | %.4f | %.4f |" % (per_call(split, "stream_chunk_in"), per_call(split_old, "stream_chunk_in")),
              "| static part (window encoders + static cond_transform columns; %d rows against %d) | %.4f | %.4f |"
              % (B, V, per_call(split, "stream_chunk_static"), per_call(split_old, "stream_chunk_static")),
              "| candidates in (lfi_stream_cand_seq_in) | %.4f | - |" % per_call(split, "stream_rollout_in"),
              "| front end + chain (lfi_flow_sample_cand_seq / lfi_flow_sample_seq_nll, %d rows both) | %.4f | %.4f |"
              % (V, both, per_call(split_old, "stream_chunk_gen_chain")),
              "| - front end alone (LFI_CHUNK_ONLY=front) | %.4f | - |" % fr,
              "| - chain (the difference) | %.4f | - |" % (both - fr),
              "| commit (lfi_stream_chunk_out + lfi_stream_commit_cand_seq) | %.4f | - |" % per_call(split, "stream_rollout_commit"),
              "", "The recipe's save_rows / load_rows launches and its window launch out carry no timer: they are the rest of its GPU time."]
    return "\n".join(lines) + "\n"


def chain_kernel_resources():
    """tools/kernel_resources.py on the two chunk units, side by side -> the chain kernels' lines."""
    import subprocess
    units = (("lfi_flow_chunk.hip", "flow_fwd_seq_chain_kernel"), ("lfi_flow_chunk_rows.hip", "flow_fwd_seq_rows_chain_kernel"))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                               os.path.join(ROOT, "lets_face_it_amd", "csrc", unit), name], stdout=subprocess.PIPE, text=True)
             for unit, name in units]
    return [line for p in procs for line in p.communicate()[0].splitlines() if "chain_kernel" in line]


def observe_ragged_report(m, dev, batches, ns, reps, dims, start, C, device_name, resources):
    """The --observe-ragged report: per (B, n) the GPU and wall time per call of the arms the module's docstring lists."""
    import torch
    s = m.spec
    eng = m._ensure_engine(dev)
    top = max(ns)
    lines = ["# observe_many(lengths=...): ragged chunks (tools/stream_latency.py --observe-ragged)", "",
             "final_model.yaml as shipped (C = %d, S = %d, K = %d, H = %d, D = %d), engine precision %s; every arm of a (B, n) on a "
             "session of its own in one process, the order rotating; %d timed rounds after 2 untimed ones; per CALL: wall = call to "
             "result on the host (one synchronise after it), GPU = HIP events around it; median (min .. max). Device %s."
             % (C, s.S, s.Ks, s.H, s.D, m.precision, reps, device_name), "",
             "| B | n | arm | wall ms | GPU ms | GPU ms / live frame-row x 1e3 |", "|---|---|---|---|---|---|"]
    notes, split = [], []
    for B in batches:
        gd = torch.Generator().manual_seed(B + 9)
        data = {k: torch.randn(B, start + top + 1, d, generator=gd).to(dev) for k, d in dims.items()}
        seed = {k: v[:, :start].contiguous() for k, v in data.items()}
        frames = [{k: v[:, start + i].contiguous() for k, v in data.items() if k != "p1_face"} for i in range(top + 1)]
        noise = (torch.randn(top + 1, B, C, generator=gd) * 0.8).to(dev)
        with m.open_stream(seed) as ref:
            faces = [ref.step(frames[i], noise[i]) for i in range(top + 1)]
        clip = torch.stack(faces, 1)
        seed16 = {k: v[:16].contiguous() for k, v in seed.items()}
        with contextlib.ExitStack() as stack:
            for n in ns:
                chunk = {k: v[:, start + 1:start + 1 + n].contiguous() for k, v in data.items() if k != "p1_face"}
                cfaces = clip[:, 1:1 + n].contiguous()
                chunk16, cfaces16 = {k: v[:16].contiguous() for k, v in chunk.items()}, cfaces[:16].contiguous()
                arms = [("(a) dense", None), ("(a) lengths all n", [n] * B)]
                if B > 16:
                    arms.append(("(b) rows 0 .. 15 at n, %d rows at 0" % (B - 16), [n] * 16 + [0] * (B - 16)))
                    arms.append(("(b) side session: open_stream(16 rows), observe_many, save_rows, load_rows", "side"))
                arms.append(("(c) lengths spread evenly over 0 .. n", [round(r * n / (B - 1)) if B > 1 else n // 2 for r in range(B)]))
                sessions = {name: stack.enter_context(m.open_stream(seed)) for name, _ in arms}
                legs = {name: ([], []) for name, _ in arms}

                def call(st, lens):
                    if lens == "side":
                        with m.open_stream(seed16) as side:
                            side.observe(frames16[0], faces16[0])
                            side.observe_many(chunk16, cfaces16)
                            st.load_rows(list(range(16)), side.save_rows(list(range(16))))
                    else:
                        st.observe_many(chunk, cfaces, lengths=lens)
                frames16, faces16 = [{k: v[:16].contiguous() for k, v in frames[0].items()}], [faces[0][:16].contiguous()]
                k = len(arms)
                for r in range(reps + 2):
                    for name, lens in arms[r % k:] + arms[:r % k]:
                        st = sessions[name]
                        st.reset(seed)
                        st.observe(frames[0], faces[0])
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        call(st, lens)
                        e1.record()
                        e1.synchronize()
                        t1 = time.perf_counter()
                        if r >= 2:
                            legs[name][0].append((t1 - t0) * 1e3)
                            legs[name][1].append(e0.elapsed_time(e1))
                fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
                for name, lens in arms:
                    live = n * B if lens is None else 16 * n if lens == "side" else sum(lens)
                    lines.append("| %d | %d | %s | %s | %s | %.3f |" % (B, n, name, fmt(legs[name][0]), fmt(legs[name][1]),
                                                                      1e3 * statistics.median(legs[name][1]) / max(live, 1)))
                dense, full = legs["(a) dense"][1], legs["(a) lengths all n"][1]
                diff, spread = statistics.median(full) - statistics.median(dense), max(dense) - min(dense)
                notes.append("- B = %d, n = %d: lengths all n %+.3f ms GPU against dense; the dense arm's own spread over its %d rounds is "
                             "%.3f ms: %s." % (B, n, diff, reps, spread, "inside it" if abs(diff) <= spread else "BEYOND it"))
                if B > 16:
                    # the front end / chain split of arm (b): each part alone (LFI_CHUNK_ONLY, honoured by the ragged entry point as by
                    # the dense one), the chain on the gic a whole call left in the work area
                    name, lens = arms[2]
                    st = sessions[name]
                    st.reset(seed)
                    st.observe(frames[0], faces[0])
                    st.observe_many(chunk, cfaces, lengths=lens)
                    parts = {}
                    for part in ("chain", "front"):
                        os.environ["LFI_CHUNK_ONLY"] = part
                        try:
                            eng.enable_timing(True)
                            st.observe_many(chunk, cfaces, lengths=lens)
                            summary = eng.timing_summary()
                        finally:
                            eng.enable_timing(False)
                            del os.environ["LFI_CHUNK_ONLY"]
                        got = summary.get("stream_chunk_chain")
                        parts[part] = got[0] * got[1] if got else 0.0
                        if part == "front":
                            for t in ("stream_chunk_in", "stream_chunk_static"):
                                parts[t] = summary[t][0] * summary[t][1] if t in summary else 0.0
                    split.append((B, n, parts))
                for st in sessions.values():
                    st.close()
    lines += ["", "## (a) Dense against lengths all n", ""] + notes
    if split:
        lines += ["", "## (b) Where the GPU time of the one-live-tile call goes (enable_timing, HIP events; ms per call)", "",
                  "The front end stays dense over n * B windows whatever the lengths; the chain runs one tile.", "",
                  "| B | n | windows in | static part | front end alone | chain alone (one launch, one live tile) |", "|---|---|---|---|---|---|"]
        for B, n, t in split:
            lines.append("| %d | %d | %.3f | %.3f | %.3f | %.3f |" % (B, n, t["stream_chunk_in"], t["stream_chunk_static"], t["front"], t["chain"]))
    lines += ["", "## Register figures of the two chain kernels (tools/kernel_resources.py, gfx950)", "", "```"] + (resources or []) + ["```"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
