"""GPU: per-array statistics (lfi_segment_stats) and the blame record behind the non-finite step guard (lfi_segment_stats_guard), from
the kernels through the C ABI to GlowEngine.blame_state() on the eager and the captured training step. Reference:
tests/blame_expected.py (numpy fp64). Counts and first indices are exact; SUMSQ is held to |SUMSQ - ref| <= 2 len 2^-53 ref, derived,
not measured: squares of fp32 values are exact in fp64, any summation order of len non-negative terms errs by at most len 2^-53
relative, and the reference's own sum gets the same allowance."""
import copy
import ctypes
import math
import struct
from argparse import Namespace

import numpy as np
import pytest
import torch

from blame_expected import NONE, sumsq_bound, table
from helpers import Fixture, report

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
BAND = 64                                        # 8-byte slots of sentinel around the record and the work buffer
SENTINEL = struct.unpack("<q", struct.pack("<d", 12345.0))[0]
POISON = (NAN, INF, -INF)


def _L():
    from lets_face_it_amd import _lib
    return _lib, _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _clean(n, gen):
    return (torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 4 - 2)).numpy()


class _Case:
    """A flat buffer whose segments sit at odd offsets with NaN-filled gaps of 1 - 3 floats, plus extra arrays that start 0 - 3 floats
    into their own allocations; poison at the first and last element of every array, on both sides of every chunk boundary and - the
    gaps apart - an Inf just outside some segments."""

    def __init__(self, lengths, extra_lengths, device, poisoned, seed=0):
        _lib, L = _L()
        CH = L.lfi_segment_stats_chunk()
        gen = torch.Generator().manual_seed(seed)
        self.segs, off = [], 1
        for i, n in enumerate(lengths):
            self.segs.append((off, n))
            off += n + 1 + i % 3
        self.n = off + 2
        flat = np.full(self.n, NAN, dtype=np.float32)
        for i, (o, n) in enumerate(self.segs):
            flat[o:o + n] = _clean(n, gen)
            if i % 4 == 1:
                flat[o + n] = INF      # just outside: the element behind the segment's last
        extras = [_clean(n, gen).astype(np.float32) for n in extra_lengths]
        if poisoned:
            k = 0
            for i, arr in enumerate([flat[o:o + n] for o, n in self.segs] + extras):
                n = arr.shape[0]
                if i % 5 == 4 and n > 4:
                    continue      # every fifth array stays clean
                spots = {0, n - 1} | {c * CH - 1 for c in range(1, n // CH + 1)} | {c * CH for c in range(1, n // CH + 1) if c * CH < n}
                if i % 2:
                    spots.discard(0)      # ... so that FIRST is not always 0
                for s in sorted(x for x in spots if 0 <= x < n):
                    arr[s] = POISON[k % 3]
                    k += 1
        self.flat_host, self.extras_host = flat, extras
        self.flat = torch.from_numpy(flat).to(device)
        self.table = torch.tensor(self.segs, dtype=torch.int64).reshape(-1).to(device) if lengths else None
        self.extra_bufs = [torch.zeros(n + 3, device=device) for n in extra_lengths]
        self.extras = []
        for j, (buf, x) in enumerate(zip(self.extra_bufs, extras)):
            v = buf[j % 4:j % 4 + x.shape[0]]
            v.copy_(torch.from_numpy(x))
            self.extras.append(v)
        self.narr = len(lengths) + len(extra_lengths)
        nx = len(extra_lengths)
        self.xp = (ctypes.c_void_p * max(nx, 1))(*[v.data_ptr() for v in self.extras])
        self.xl = (ctypes.c_long * max(nx, 1))(*extra_lengths)
        self.nseg, self.nextra = len(lengths), nx
        floats = L.lfi_segment_stats_work_floats(self.n, self.nseg, nx, self.xl)
        assert floats > 0 and floats % 2 == 0
        self.work_slots = floats // 2
        self.lens = list(lengths) + list(extra_lengths)

    def expected(self):
        return table(self.flat_host, self.segs, self.extras_host)

    def arena(self, head=0):
        """BAND | record (head + 4 slots per array) | BAND | work | BAND, all sentinels."""
        _lib, _ = _L()
        rec_slots = head + _lib.SEG_SLOTS * self.narr
        whole = torch.full((3 * BAND + rec_slots + self.work_slots,), SENTINEL, dtype=torch.int64, device=self.flat.device)
        return whole, BAND, rec_slots, 2 * BAND + rec_slots

    def run(self, whole, rec0, work0, guard=None):
        _lib, L = _L()
        base = whole.data_ptr()
        seg_ptr = self.table.data_ptr() if self.table is not None else None
        flat_ptr = self.flat.data_ptr() if self.nseg else None
        if guard is None:
            rc = L.lfi_segment_stats(flat_ptr, self.n, seg_ptr, self.nseg, self.nextra, self.xp, self.xl, base + 8 * rec0, base + 8 * work0, _st())
        else:
            rc = L.lfi_segment_stats_guard(flat_ptr, self.n, seg_ptr, self.nseg, self.nextra, self.xp, self.xl, guard.data_ptr(),
                                           base + 8 * rec0, base + 8 * work0, _st())
        assert rc == 0, L.lfi_last_error()
        torch.cuda.synchronize()


def _f64(word):
    return struct.unpack("<d", struct.pack("<q", int(word)))[0]


def _check_table(words, want, lens, what):
    _lib, _ = _L()
    worst = 0.0
    for i, (w, n) in enumerate(zip(want, lens)):
        r = words[_lib.SEG_SLOTS * i:_lib.SEG_SLOTS * (i + 1)]
        got = (int(r[_lib.SEG_NAN]), int(r[_lib.SEG_INF]), int(r[_lib.SEG_FIRST]) & (2 ** 64 - 1))
        assert got == (w["nan"], w["inf"], w["first"]), "%s: array %d (length %d): counts / first %r, expected %r" % (
            what, i, n, got, (w["nan"], w["inf"], w["first"]))
        s = _f64(r[_lib.SEG_SUMSQ])
        err, bound = abs(s - w["sumsq"]), sumsq_bound(n, w["sumsq"])
        assert err <= bound, "%s: array %d (length %d): SUMSQ %r vs %r, |diff| %.3e > bound %.3e" % (what, i, n, s, w["sumsq"], err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    return worst


def _lengths(CH):
    return [1, 3, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 5, 0]


def _extra_lengths(CH, k):
    return [CH + 1, 0, 5, 257, 2 * CH + 5, 1, 3, 256][:k]


# ------------------------------------------------------------------ 1. the kernel through the C ABI
@pytest.mark.parametrize("nseg,nextra", [(10, 0), (10, 1), (10, 8), (1, 0), (1, 8), (300, 1), (0, 8), (0, 1)])
@pytest.mark.parametrize("poisoned", [False, True], ids=["clean", "poisoned"])
def test_segment_stats_through_the_c_abi(nseg, nextra, poisoned, gpu_device):
    _lib, L = _L()
    CH = L.lfi_segment_stats_chunk()
    base = _lengths(CH)
    if nseg == 1:
        lengths = [2 * CH + 5]
    elif nseg == 300:      # the boundary lengths once, then many small tensors (56 is the smallest of the shipped model)
        lengths = base + [(56, 0, 1, 2, 3, 4, 5, 255, 257, 1023)[i % 10] for i in range(290)]
    else:
        lengths = base[:nseg]
    case = _Case(lengths, _extra_lengths(CH, nextra), gpu_device, poisoned, seed=nseg * 10 + nextra)
    want = case.expected()
    if poisoned and nseg == 10:
        assert any(w["nan"] for w in want) and any(w["inf"] >= 2 for w in want) and any(w["first"] not in (0, NONE) for w in want)
    if not poisoned:
        assert all(w["nan"] == 0 and w["inf"] == 0 and w["first"] == NONE for w in want), "a NaN of a gap or an Inf behind a segment was counted by the reference"
    whole, rec0, rec_slots, work0 = case.arena()
    before = whole.clone()
    case.run(whole, rec0, work0)
    first = whole.clone()
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[rec0:rec0 + rec_slots] = False
    outside[work0:work0 + case.work_slots] = False
    assert torch.equal(whole[outside], before[outside]), "a launch wrote outside the record and the work buffer"
    worst = _check_table(whole[rec0:rec0 + rec_slots].cpu().tolist(), want, case.lens, "nseg %d nextra %d" % (nseg, nextra))
    # a second run over buffers that hold the first run's leftovers: the same bits
    case.run(whole, rec0, work0)
    assert torch.equal(whole[rec0:rec0 + rec_slots], first[rec0:rec0 + rec_slots]), "two runs differ"
    assert torch.equal(whole[outside], before[outside])
    report("lfi_segment_stats nseg %d nextra %d %s: counts and first indices exact, worst |SUMSQ - ref| / bound %.3f, two runs bit-equal, "
           "bands untouched" % (nseg, nextra, "poisoned" if poisoned else "clean", worst))


def test_empty_call_and_zero_length_arrays(gpu_device):
    _lib, L = _L()
    whole = torch.full((3 * BAND + 8,), SENTINEL, dtype=torch.int64, device=gpu_device)
    before = whole.clone()
    assert L.lfi_segment_stats(None, 0, None, 0, 0, None, None, whole.data_ptr() + 8 * BAND, whole.data_ptr() + 8 * (2 * BAND + 4), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(whole, before)
    case = _Case([0, 0], [0], gpu_device, False)
    whole, rec0, rec_slots, work0 = case.arena()
    case.run(whole, rec0, work0)
    assert whole[rec0:rec0 + rec_slots].cpu().tolist() == [0, 0, 0, -1] * 3


# ------------------------------------------------------------------ 2. the guarded entry
def _guard_rec(device, apply, applied=7, skipped=5):
    _lib, _ = _L()
    s = [0] * _lib.GUARD_SLOTS
    s[_lib.GUARD_APPLY], s[_lib.GUARD_APPLIED], s[_lib.GUARD_SKIPPED] = apply, applied, skipped
    return torch.tensor(s, dtype=torch.int64, device=device)


def test_guarded_entry_fills_first_and_leaves_otherwise(gpu_device):
    _lib, L = _L()
    CH = L.lfi_segment_stats_chunk()
    case = _Case(_lengths(CH), _extra_lengths(CH, 3), gpu_device, True, seed=3)
    H = _lib.BLAME_HEAD
    # the unconditional entry's table, for the comparison bit by bit
    plain, p_rec0, p_slots, p_work0 = case.arena()
    case.run(plain, p_rec0, p_work0)
    want_table = plain[p_rec0:p_rec0 + p_slots].clone()

    whole, rec0, rec_slots, work0 = case.arena(head=H)
    whole[rec0:rec0 + H] = 0      # the header as the host clears it; table and work buffer keep their sentinels
    before = whole.clone()
    # APPLY = 1: a taken step - the blame record and the work buffer keep their bits
    taken = _guard_rec(gpu_device, 1)
    taken_before = taken.clone()
    case.run(whole, rec0, work0, guard=taken)
    assert torch.equal(whole, before) and torch.equal(taken, taken_before), "a taken step wrote"
    # APPLY = 0, FILLED = 0: the table of the unconditional entry, STEP = APPLIED + SKIPPED, FILLED = 1; the guard record is only read
    skipped = _guard_rec(gpu_device, 0, applied=7, skipped=5)
    skipped_before = skipped.clone()
    case.run(whole, rec0, work0, guard=skipped)
    assert torch.equal(skipped, skipped_before)
    head = whole[rec0:rec0 + H].cpu().tolist()
    assert head[_lib.BLAME_FILLED] == 1 and head[_lib.BLAME_STEP] == 12
    assert torch.equal(whole[rec0 + H:rec0 + rec_slots], want_table), "the guarded table differs from the unconditional entry's"
    outside = torch.ones_like(whole, dtype=torch.bool)
    outside[rec0:rec0 + rec_slots] = False
    outside[work0:work0 + case.work_slots] = False
    assert torch.equal(whole[outside], before[outside])
    # APPLY = 0, FILLED = 1: a second skipped step before the host looked - nothing moves, although the data has changed
    filled = whole.clone()
    case.flat[case.segs[0][0]] = 1.0
    later = _guard_rec(gpu_device, 0, applied=7, skipped=6)
    case.run(whole, rec0, work0, guard=later)
    assert torch.equal(whole, filled), "a filled record was written again"
    # cleared by the host: the next skipped step fills it with its own number and the new data
    whole[rec0:rec0 + H] = 0
    case.run(whole, rec0, work0, guard=later)
    assert whole[rec0:rec0 + H].cpu().tolist() == [1, 13]
    assert not torch.equal(whole[rec0 + H:rec0 + H + _lib.SEG_SLOTS], want_table[:_lib.SEG_SLOTS])


# ------------------------------------------------------------------ the engine and the training step
def _module(fx_name, gpu_device, blame=True, masks=True, ema_decay=None):
    """The module of test_gpu_guard (fixture weights, injected masks, exact-f32 GEMMs, Adam, clip 5) with print_nan_grads."""
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    fx = Fixture(fx_name)
    hp = Namespace(**copy.deepcopy(fx.hp))
    hp.Train["use_negative_nll_loss"] = False
    hp.gradient_clip_val = 5.0
    hp.Optim["name"] = "adam"
    hp.Optim["args"]["adam"] = {"betas": [0.9, 0.9999], "eps": 1e-8}
    hp.Optim["skip_nonfinite"] = True
    hp.print_nan_grads = bool(blame)
    if ema_decay is not None:
        hp.Optim["ema_decay"] = ema_decay
    hp.engine_precision = "f32"
    lm = LetsFaceItGlow(hp)
    lm.seq_glow.load_state_dict(fx.state_dict(torch.float32))
    lm.to(gpu_device)
    lm.seq_glow.glow.set_actnorm_init(True)
    lm.train()
    lm.seq_glow.injected_masks = ({k: v.to(gpu_device) for k, v in fx.masks(torch.float32).items()} if fx.masks() else None) if masks else None
    return lm, {k: v.to(gpu_device) for k, v in fx.batch(torch.float32).items()}, fx


def _poisoned(batch, fx, value, row=1, chan=2, frame=1):
    """One element of p1_face at modelled frame `frame` (t = start + frame) of one row."""
    out = {k: v.clone() for k, v in batch.items()}
    out["p1_face"][row, fx.start + frame, chan] = value
    return out


def test_flat_segments_and_per_tensor_norms(gpu_device):
    _lib, L = _L()
    lm, batch, fx = _module("mid", gpu_device, blame=False)
    eng = lm.seq_glow._ensure_engine(gpu_device)
    segs = eng.flat_segments()
    assert [k for k, _, _ in segs] == [k for k, _ in lm.seq_glow.named_parameters()]
    assert set(k for k, _, _ in segs) <= set(lm.seq_glow.state_dict())
    spans = sorted((o, o + n) for _, o, n in segs)
    assert spans[0][0] >= 0 and spans[-1][1] <= eng.n_params
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "segments overlap"
    for key, o, n in segs:
        assert n == dict(lm.seq_glow.named_parameters())[key].numel()
        assert key.startswith("glow.flow.") or key.startswith("feature_encoder."), key
        assert (o >= eng.flow_offset) == key.startswith("glow.flow."), key      # the flow block is the all-reduce's first bucket
    assert any(k.startswith("glow.flow.") for k, _, _ in segs) and any(o < eng.flow_offset for _, o, _ in segs)
    lm.fused_training_step(batch, 1e-3)
    stats = eng.grad_tensor_stats()
    total = torch.zeros(1 + 1024, dtype=torch.float64, device=gpu_device)
    assert L.lfi_grad_sumsq(eng.grads.data_ptr(), eng.n_params, total.data_ptr(), total.data_ptr() + 8, _st()) == 0
    whole = float(total[0])
    covered = sum(n for _, _, n in segs)
    if covered < eng.n_params:      # alignment padding between tensors: never written, so it adds nothing to the total
        mask = torch.ones(eng.n_params, dtype=torch.bool, device=gpu_device)
        for _, o, n in segs:
            mask[o:o + n] = False
        assert not eng.grads[mask].any()
    summed = math.fsum(r["sumsq"] for r in stats)
    assert whole > 0 and abs(summed - whole) <= 2.0 * eng.n_params * 2.0 ** -53 * whole, (summed, whole)
    norms = eng.grad_tensor_norms(gmul=-0.5)
    g = eng.grads.cpu().double()
    worst = 0.0
    for (key, o, n), r in zip(segs, stats):
        assert r["key"] == key and (r["nan"], r["inf"], r["first"]) == (0, 0, None)
        ref = float((g[o:o + n] ** 2).sum())
        assert abs(r["sumsq"] - ref) <= sumsq_bound(n, ref), key
        # the root halves the relative error of the square and adds its own rounding on either side: (n + 2) 2^-53 <= 2 n 2^-53 for
        # n >= 2, and the root of one exact square is exact - the bound of the squares holds for the norms as it stands
        ref_norm = 0.5 * math.sqrt(ref)
        assert abs(norms[key] - ref_norm) <= sumsq_bound(n, ref_norm), key
        if ref > 0:
            worst = max(worst, abs(r["sumsq"] - ref) / sumsq_bound(n, ref))
    report("per-tensor gradient statistics on mid (%d tensors): sum of SUMSQ vs lfi_grad_sumsq rel %.2e (bound %.2e), worst tensor "
           "|SUMSQ - ref| / bound %.3f" % (len(segs), abs(summed - whole) / whole, 2.0 * eng.n_params * 2.0 ** -53, worst))


def test_blame_names_the_one_gradient_tensor_that_was_poisoned(gpu_device):
    lm, batch, fx = _module("tiny", gpu_device)
    sg = lm.seq_glow
    eng = sg._ensure_engine(gpu_device)
    eng.enable_step_guard()
    eng.enable_step_blame()
    assert eng.blame_state() is None
    segs = eng.flat_segments()
    key, off, n = next(s for s in segs[len(segs) // 2:] if s[2] >= 3)
    x = batch["p1_face"]
    masks = sg._draw_masks(x.shape[0], x.shape[1] - fx.start, gpu_device)
    _, nll = eng.forward(batch, masks, with_stash=True)
    eng.backward(1.0 / nll.numel())
    eng.grads[off + n - 2] = INF
    before = eng.params.clone()
    eng.optimizer_step(1e-3, 0.9, 0.9999, 1e-8, clip=5.0)
    st = eng.blame_state(clear=False)
    assert torch.equal(eng.params, before), "the step was not skipped"
    assert st is not None and st["step"] == 1
    assert st["gradients"] == [{"key": key, "nan": 0, "inf": 1, "first": n - 2}]
    assert st["inputs"] == {} and (st["nll"]["nan"], st["nll"]["inf"], st["nll"]["first"]) == (0, 0, None)
    assert st["nll"]["count"] == nll.numel() and st["tensors"] == len(segs) and set(st["norms"]) == {k for k, _, _ in segs}
    assert all(math.isfinite(v) for v in st["norms"].values())
    assert eng.blame_state() == st and eng.blame_state() is None, "clear=False keeps the record, clear=True empties it"
    # nothing of it reaches the optimiser state
    assert "blame" not in eng.optimizer_state()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "step_graph"])
def test_poisoned_batch_is_traced_to_its_input_frame_and_row(graph, gpu_device):
    """Steps 1-3 clean (the captured step is recorded at the third), 4 and 5 poisoned, a look, 6 poisoned elsewhere, 7 clean."""
    row, frame, chan = 1, 1, 2
    runs = {}
    for blame in (True, False):
        torch.manual_seed(7)
        lm, batch, fx = _module("tiny", gpu_device, blame=blame, masks=not graph, ema_decay=0.99)
        lm.step_graph = graph
        eng = lm.seq_glow._ensure_engine(gpu_device)
        bad = _poisoned(batch, fx, NAN, row, chan, frame)
        other = _poisoned(batch, fx, INF, row=0, chan=0, frame=2)
        for step, b in enumerate((batch, batch, batch, bad, bad), start=1):
            lm.fused_training_step(b, 1e-3)
        if blame:
            nll = eng._last.nll
            nonfinite = ~torch.isfinite(nll)      # (N, B): the last step's, whichever way it ran
            assert bool(nonfinite.any()) and not bool(nonfinite[:, [r for r in range(nll.shape[1]) if r != row]].any())
            st = eng.blame_state(clear=True)
            assert st is not None and st["step"] == 4, "the FIRST skipped step is the one kept"
            assert st["inputs"] == {"p1_face": {"nan": 1, "inf": 0, "first": (row, fx.start + frame, chan)}}
            assert st["nll"]["first"] == (frame, row) and st["nll"]["nan"] + st["nll"]["inf"] == int(nonfinite.sum())
            assert st["nll"]["count"] == nll.numel()
            assert len(st["gradients"]) > 0 and {g["key"] for g in st["gradients"]} <= set(lm.seq_glow.state_dict())
            assert eng.blame_state() is None
        lm.fused_training_step(other, 1e-3)
        if blame:
            st = eng.blame_state()
            assert st is not None and st["step"] == 6
            assert st["inputs"] == {"p1_face": {"nan": 0, "inf": 1, "first": (0, fx.start + 2, 0)}} and st["nll"]["first"] == (2, 0)
        lm.fused_training_step(batch, 1e-3)
        graphs = [v for v in getattr(lm, "_step_graphs", {}).values() if isinstance(v, dict)]
        assert len(graphs) == (1 if graph else 0) and not getattr(lm, "_step_graphs", {}).get("broken")
        gs = eng.guard_state()
        assert (gs["skipped"], gs["applied"]) == (3, 4)
        assert (eng.blame is not None) == blame
        runs[blame] = (eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.ema.clone())
    for a, b, what in zip(runs[True], runs[False], ("params", "adam_m", "adam_v", "ema")):
        assert torch.equal(a, b), "%s differs between blame on and off" % what


def test_blame_off_makes_no_call_into_the_new_entry_points(gpu_device, monkeypatch):
    lm, batch, fx = _module("tiny", gpu_device, blame=False)
    eng = lm.seq_glow._ensure_engine(gpu_device)

    def refuse(*args):
        raise AssertionError("a blame launch with print_nan_grads off")

    monkeypatch.setattr(eng.L, "lfi_segment_stats_guard", refuse)
    monkeypatch.setattr(eng.L, "lfi_segment_stats", refuse)
    for b in (batch, _poisoned(batch, fx, NAN), batch):
        lm.fused_training_step(b, 1e-3)
    gs = eng.guard_state()
    assert (gs["skipped"], gs["applied"]) == (1, 2) and eng.blame is None
    with pytest.raises(RuntimeError, match="blame is off"):
        eng.blame_state()
