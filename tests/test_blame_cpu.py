"""CPU: the blame record's reference (tests/blame_expected.py) against planted cases, the host-side decoding and report
(lets_face_it_amd/blame.py), `print_nan_grads` validation, the Trainer's report and extended error text with a stand-in engine, and the
refusals of both C entry points (no kernels run)."""
import copy
import ctypes
import math
import re
import struct
from argparse import Namespace

import numpy as np
import pytest
import torch

from blame_expected import NONE, BlameRecord, record, sumsq_bound, table
from helpers import Fixture
from lets_face_it_amd import _lib
from lets_face_it_amd import blame as blame_mod
from lets_face_it_amd.trainer import Trainer
from test_guard_cpu import _Data, _Engine, _Recorder, _trainer_hparams, no_device_wait  # noqa: F401  (the fixture is used by name)

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ the reference, by hand
def test_record_by_hand():
    assert record([3.0, -4.0]) == {"sumsq": 25.0, "nan": 0, "inf": 0, "first": NONE}
    assert record([]) == {"sumsq": 0.0, "nan": 0, "inf": 0, "first": NONE}
    assert record([1.0, NAN, 2.0, INF, NAN]) == {"sumsq": 5.0, "nan": 2, "inf": 1, "first": 1}
    # an Inf and a -Inf in one array are two Infs (their sum would be a NaN: nothing is summed that is not finite)
    assert record([INF, 1.0, -INF]) == {"sumsq": 1.0, "nan": 0, "inf": 2, "first": 0}
    # +-3e38 is finite: it enters SUMSQ, which fp64 holds without overflow
    r = record([3e38, -3e38])
    big = float(np.float32(3e38)) ** 2
    assert (r["nan"], r["inf"], r["first"]) == (0, 0, NONE) and r["sumsq"] == 2 * big and math.isfinite(r["sumsq"])


def test_a_nan_in_a_gap_is_not_counted():
    flat = np.arange(12, dtype=np.float32)
    flat[5] = NAN      # between the segments [1, 5) and [6, 9)
    flat[0] = INF      # in front of the first
    got = table(flat, [(1, 4), (6, 3), (9, 0)], extras=[np.array([NAN], dtype=np.float32)])
    assert got[0] == {"sumsq": 1.0 + 4 + 9 + 16, "nan": 0, "inf": 0, "first": NONE}
    assert got[1] == {"sumsq": 36.0 + 49 + 64, "nan": 0, "inf": 0, "first": NONE}
    assert got[2] == {"sumsq": 0.0, "nan": 0, "inf": 0, "first": NONE}
    assert got[3] == {"sumsq": 0.0, "nan": 1, "inf": 0, "first": 0}
    flat[6] = NAN      # now inside the second segment, at its element 0
    assert table(flat, [(1, 4), (6, 3)])[1] == {"sumsq": 49.0 + 64, "nan": 1, "inf": 0, "first": 0}


def test_sumsq_bound_is_the_derived_one():
    assert sumsq_bound(1000, 2.0) == 2.0 * 1000 * 2.0 ** -53 * 2.0 and sumsq_bound(0, 5.0) == 0.0


def test_fill_first_then_clear():
    b = BlameRecord()
    assert not b.call(1, 7, 0, lambda: "never") and b.read() is None
    assert b.call(0, 7, 1, lambda: "first") and not b.call(0, 7, 2, lambda: "second") and not b.call(1, 8, 2, lambda: "taken")
    assert b.read(clear=False) == {"step": 8, "table": "first"} and b.read() == {"step": 8, "table": "first"}
    assert b.read() is None
    assert b.call(0, 8, 3, lambda: "third") and b.read() == {"step": 11, "table": "third"}


# ------------------------------------------------------------------ host-side decoding
def test_index_arithmetic():
    B, T, dim = 5, 7, 3
    x = np.arange(B * T * dim).reshape(B, T, dim)
    for row, frame, col in ((0, 0, 0), (4, 6, 2), (2, 5, 1), (3, 0, 2)):
        assert blame_mod.input_index(int(x[row, frame, col]), (B, T, dim)) == (row, frame, col)
    N = 4
    nll = np.arange(N * B).reshape(N, B)      # frame-major, as the engine's (N, B) per-frame NLL
    for frame, row in ((0, 0), (3, 4), (2, 1)):
        assert blame_mod.nll_index(int(nll[frame, row]), B) == (frame, row)


def _words(step, records, filled=1):
    w = [filled, step]
    for r in records:
        w += [struct.unpack("<q", struct.pack("<d", r["sumsq"]))[0], r["nan"], r["inf"], r["first"] if r["first"] != NONE else -1]
    return w      # (signed words, as a torch.int64 tensor's .tolist() gives them)


def _example_state():
    keys = ["enc.weight", "flow.0.bias", "flow.1.bias"]
    B, T, dim, N = 4, 6, 3, 2
    face = np.zeros((B, T, dim), dtype=np.float32)
    face[2, 5, 1] = NAN
    speech = np.ones((B, T, dim), dtype=np.float32)
    nll = np.zeros((N, B), dtype=np.float32)
    nll[1, 2] = NAN
    grads = [np.array([3.0, 4.0], dtype=np.float32), np.array([NAN, 1.0, INF], dtype=np.float32), np.array([2.0], dtype=np.float32)]
    recs = [record(g) for g in grads] + [record(face), record(speech), record(nll)]
    inputs = [("p1_face", (B, T, dim)), ("p1_speech", (B, T, dim))]
    return keys, inputs, (N, B), recs


def test_decode_names_inputs_frames_and_tensors():
    keys, inputs, nll_shape, recs = _example_state()
    assert blame_mod.decode(_words(9, recs, filled=0), keys, inputs, nll_shape) is None
    st = blame_mod.decode(_words(9, recs), keys, inputs, nll_shape, gmul=-0.5)
    assert st["step"] == 9 and st["tensors"] == 3
    assert st["inputs"] == {"p1_face": {"nan": 1, "inf": 0, "first": (2, 5, 1)}}
    assert st["nll"] == {"nan": 1, "inf": 0, "count": 8, "first": (1, 2)}
    assert st["gradients"] == [{"key": "flow.0.bias", "nan": 1, "inf": 1, "first": 0}]
    assert st["norms"] == {"enc.weight": 2.5, "flow.0.bias": 0.5, "flow.1.bias": 1.0}      # finite part x |gmul|
    line = blame_mod.report(st)
    assert line == ("step 9: inputs: p1_face 1 non-finite (first: row 2, frame 5, column 1); NLL: 1 of 8 frames (first: frame 1, row 2); "
                    "gradients: 1 of 3 tensors non-finite (first: flow.0.bias)")
    assert "\n" not in line


def test_report_cuts_long_lists_with_a_count():
    keys = ["t%02d" % i for i in range(11)]
    recs = [record([NAN]) for _ in keys]
    st = blame_mod.decode(_words(3, recs), keys, [], None)
    line = blame_mod.report(st)
    assert "11 of 11 tensors non-finite (first: t00, t01, t02, t03, t04, t05, t06, t07 ... and 3 more)" in line
    assert "t08" not in line and "inputs: finite" in line and "NLL" not in line


# ------------------------------------------------------------------ hparams
def _hparams(optim=None, **top):
    hp = Namespace(**copy.deepcopy(Fixture("tiny").hp))
    hp.Optim.update(optim or {})
    for k, v in top.items():
        setattr(hp, k, v)
    return hp


def test_print_nan_grads_is_off_by_default_and_implies_the_guard():
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    for off in ({}, {"print_nan_grads": None}, {"print_nan_grads": False}):
        lm = LetsFaceItGlow(_hparams(**off))
        assert lm.print_nan_grads is False and lm.skip_nonfinite is False
    lm = LetsFaceItGlow(_hparams(print_nan_grads=True))
    assert lm.print_nan_grads is True and lm.skip_nonfinite is True
    assert LetsFaceItGlow(_hparams({"skip_nonfinite": True})).print_nan_grads is False


@pytest.mark.parametrize("value", [1, 0, "true", 1.0, [True]])
def test_bad_print_nan_grads_raises_at_construction(value):
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    with pytest.raises(ValueError, match="print_nan_grads"):
        LetsFaceItGlow(_hparams(print_nan_grads=value))


def test_the_graph_key_tells_blamed_steps_apart():
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    eng = Namespace(precision="f32", backward_products="auto", pass_skip={})
    batch = {"p1_face": torch.zeros(2, 3, 4)}
    keys = {LetsFaceItGlow(_hparams({"skip_nonfinite": True}, print_nan_grads=on))._graph_key(batch, False, eng) for on in (False, True)}
    assert len(keys) == 2


# ------------------------------------------------------------------ the Trainer
class _BlamingEngine(_Engine):
    """_Engine plus what print_nan_grads adds: a blame record that keeps the first skipped step until it is read."""

    def __init__(self):
        super().__init__()
        self.blame = object()
        self.rec = BlameRecord()
        self.fetches = 0

    def take(self, poisoned):
        super().take(poisoned)
        c = self.counts
        keys, inputs, nll_shape, recs = _example_state()
        self.rec.call(0 if poisoned else 1, c["applied"], c["skipped"], lambda: recs)

    def blame_state(self, clear=True):
        self.fetches += 1
        got = self.rec.read(clear)
        if got is None:
            return None
        keys, inputs, nll_shape, _ = _example_state()
        return blame_mod.decode(_words(got["step"], got["table"]), keys, inputs, nll_shape)

    def grad_tensor_norms(self, gmul=1.0):
        return {"a.weight": 3.0 * gmul, "b.bias": 4.0 * gmul}


class _BlamingRecorder(_Recorder):
    def __init__(self, poisoned):
        super().__init__(poisoned)
        eng = self.eng = _BlamingEngine()
        self.seq_glow.engine = eng
        self.seq_glow._ensure_engine = lambda device: eng
        self.logged = {}

    def log(self, name, value, **kwargs):
        self.logged[name] = value


def test_the_report_is_printed_and_appended_to_the_stopping_error(tmp_path, capsys, no_device_wait):
    m = _BlamingRecorder(poisoned={3})
    tr = Trainer(_trainer_hparams(terminate_on_nan=True, print_nan_grads=True), device="cpu", log_every=2, checkpoint_dir=str(tmp_path))
    with pytest.raises(ValueError) as err:
        tr.fit(m, _Data())
    text = str(err.value)
    want = ("step 3: inputs: p1_face 1 non-finite (first: row 2, frame 5, column 1); NLL: 1 of 8 frames (first: frame 1, row 2); "
            "gradients: 1 of 3 tensors non-finite (first: flow.0.bias)")
    assert re.search(r"between step 3 and step 4 .*terminate_on_nan", text), "the existing text comes first, on one line"
    assert text.endswith(want) and "\n" not in text
    assert text.index("The weights are those of the last step taken.") < text.index("step 3: inputs")
    out = capsys.readouterr().out
    assert "non-finite gradient: " + want in out
    assert m.eng.fetches == 1, "fetched once, at the look that saw the new skip"


def test_a_survived_skip_is_reported_once_and_the_run_goes_on(capsys, no_device_wait):
    m = _BlamingRecorder(poisoned={3, 4, 7})
    Trainer(_trainer_hparams({"skip_nonfinite": True}, print_nan_grads=True), device="cpu", log_every=2, checkpoint_dir="").fit(m, _Data())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("non-finite gradient: ")]
    # steps 3 and 4 are seen together at the log point of step 4: the record kept the first; step 7 is seen at step 8
    assert [ln.split(":")[1].strip() for ln in lines] == ["step 3", "step 7"] and m.steps == 10


def test_an_engine_without_blame_state_still_stops_as_before(tmp_path, no_device_wait):
    m = _Recorder(poisoned={3})      # its engine has neither `blame` nor `blame_state`
    tr = Trainer(_trainer_hparams(terminate_on_nan=True, print_nan_grads=True), device="cpu", log_every=2, checkpoint_dir=str(tmp_path))
    with pytest.raises(ValueError, match=r"between step 3 and step 4 .*terminate_on_nan") as err:
        tr.fit(m, _Data())
    assert str(err.value).endswith("The weights are those of the last step taken.") and m.steps == 4


def test_track_grad_norm_logs_a_norm_per_tensor_and_leaves_the_line_alone(capsys, no_device_wait):
    m = _BlamingRecorder(poisoned=())
    Trainer(_trainer_hparams(track_grad_norm=2, max_steps=2), device="cpu", log_every=1, checkpoint_dir="").fit(m, _Data())
    assert m.logged == {"grad_2.0_norm/a.weight": 3.0, "grad_2.0_norm/b.bias": 4.0, "grad_2.0_norm_total": 5.0}
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch 0 step")]
    assert len(lines) == 2 and all(re.search(r"loss 0\.0000 grad_norm 1\.5000e\+00 skipped 0  \d+ frames/s$", ln) for ln in lines)
    m = _BlamingRecorder(poisoned=())
    Trainer(_trainer_hparams({"skip_nonfinite": True}, max_steps=1), device="cpu", log_every=1, checkpoint_dir="").fit(m, _Data())
    assert m.logged == {}


# ------------------------------------------------------------------ the C ABI refuses before it touches a device
def test_constants_match_the_header():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfi.h")).read()
    for name in ("SEG_SUMSQ", "SEG_NAN", "SEG_INF", "SEG_FIRST", "SEG_SLOTS", "BLAME_FILLED", "BLAME_STEP", "BLAME_HEAD"):
        assert int(re.search(r"#define LFI_%s (\d+)" % name, text).group(1)) == getattr(_lib, name), name
    assert _lib.SEG_NONE == NONE


def test_both_entry_points_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = 4096      # any non-null, 8-byte aligned address: a refused call never dereferences nor launches
    one_ptr, one_len = (ctypes.c_void_p * 1)(ok), (ctypes.c_long * 1)(4)
    neg_len = (ctypes.c_long * 1)(-1)
    nine_ptr, nine_len = (ctypes.c_void_p * 9)(*([ok] * 9)), (ctypes.c_long * 9)(*([1] * 9))
    null_ptr = (ctypes.c_void_p * 1)(None)

    def plain(flat=ok, n=16, segs=ok, nseg=1, nextra=0, xp=None, xl=None, out=ok, work=ok):
        return L.lfi_segment_stats(flat, n, segs, nseg, nextra, xp, xl, out, work, None)

    def guarded(flat=ok, n=16, segs=ok, nseg=1, nextra=0, xp=None, xl=None, rec=ok, blame=ok, work=ok):
        return L.lfi_segment_stats_guard(flat, n, segs, nseg, nextra, xp, xl, rec, blame, work, None)

    common = [dict(nseg=-1), dict(n=-1), dict(flat=None), dict(segs=None), dict(segs=ok + 4), dict(work=None), dict(work=ok + 4),
              dict(nextra=9, xp=nine_ptr, xl=nine_len), dict(nextra=-1), dict(nextra=1, xp=None, xl=one_len),
              dict(nextra=1, xp=one_ptr, xl=None), dict(nextra=1, xp=one_ptr, xl=neg_len), dict(nextra=1, xp=null_ptr, xl=one_len)]
    cases = {"lfi_segment_stats": (plain, common + [dict(out=None), dict(out=ok + 4)]),
             "lfi_segment_stats_guard": (guarded, common + [dict(rec=None), dict(rec=ok + 4), dict(blame=None), dict(blame=ok + 4)])}
    for entry, (call, bad) in cases.items():
        for kw in bad:
            rc = call(**kw)
            msg = L.lfi_last_error()
            assert rc != 0, (entry, kw)
            assert msg and entry.encode() + b":" in msg, (entry, kw, msg)
    # an empty call succeeds without a device: nothing to launch
    assert L.lfi_segment_stats(None, 0, None, 0, 0, None, None, ok, ok, None) == 0


def test_host_only_queries():
    L = _lib.lib()
    CH = L.lfi_segment_stats_chunk()
    assert CH >= 256 and CH % 4 == 0
    xl = (ctypes.c_long * 2)(CH + 1, 0)
    # 8-byte slots: one prefix entry per array and one for the total, then LFI_SEG_SLOTS per chunk the call can need
    chunks = (10 * CH + CH - 1) // CH + 3 + 2
    assert L.lfi_segment_stats_work_floats(10 * CH, 3, 2, xl) == 2 * (3 + 2 + 1 + _lib.SEG_SLOTS * chunks)
    assert L.lfi_segment_stats_work_floats(0, 0, 0, None) == 2
    assert L.lfi_segment_stats_work_floats(-1, 0, 0, None) < 0 and L.lfi_segment_stats_work_floats(4, 1, 9, xl) < 0
