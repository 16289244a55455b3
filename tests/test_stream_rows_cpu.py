"""CPU: per-row reseeding of a streaming sampling session without a device - the C entry point's argument checks (no launch) and the
model API's surface."""
import ctypes
from argparse import Namespace

import pytest

from helpers import Fixture
from lets_face_it_amd import _lib


def _reset_rows(B=4, rows=(1,), count=2, hist=3, dim=4, Ks=2, H=8, lead_last=1, ld=None):
    L = _lib.lib()
    n = max(count, 1)
    win, seed = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    lds = (ctypes.c_long * n)()
    hs, ds, lead = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
    for i in range(min(count, n)):
        win[i], seed[i], hs[i], ds[i] = 0x1000 * (i + 1), 0x20000 * (i + 1), hist, dim
        lead[i] = lead_last if i == count - 1 else 0
        lds[i] = 10 * dim if ld is None else ld
    ra = (ctypes.c_int * max(len(rows), 1))(*rows)
    rc = L.lfi_stream_reset_rows(B, len(rows), ra, count, win, seed, lds, hs, ds, lead, 0x5000, None, Ks, H, None, None, None)
    return rc, L.lfi_last_error()


def test_stream_reset_rows_reports_argument_errors_without_launching():
    for kwargs, text in ((dict(B=0), b"batch 0"), (dict(rows=()), b"0 rows"), (dict(rows=(4,)), b"is 4, outside the batch"),
                         (dict(rows=(0, -1)), b"is -1, outside the batch"), (dict(rows=(2, 0, 2)), b"row 2 is listed twice"),
                         (dict(rows=(0, 1, 2, 3, 1)), b"5 rows"), (dict(count=9), b"9 windows"), (dict(hist=0), b"hist 0"),
                         (dict(dim=-1), b"dim -1"), (dict(Ks=0), b"Ks = 0"), (dict(H=-2), b"H = -2"),
                         (dict(lead_last=2), b"lead_zero 2"), (dict(ld=5), b"seed row stride 5")):
        rc, msg = _reset_rows(**kwargs)
        assert rc == -1 and text in msg, (kwargs, msg)


def test_stream_reset_rows_is_bound_and_declared():
    assert "lfi_stream_reset_rows" in _lib.EXPORTS
    assert _lib.lib().lfi_stream_reset_rows.argtypes is not None


def test_sample_stream_has_reset_rows_and_open_stream_still_refuses_cpu_tensors():
    from lets_face_it_amd import engine
    from lets_face_it_amd.glow.models import SeqGlow
    assert callable(getattr(engine.SampleStream, "reset_rows", None))
    fx = Fixture("tiny")
    m = SeqGlow(Namespace(**fx.hp))
    seed = {k: v[:, :fx.start].float().contiguous() for k, v in fx.group("infer/data/").items()}
    with pytest.raises(RuntimeError, match="GPU only"):
        m.open_stream(seed)


def test_index_list_refusals_word_for_word():
    """The one check of `rows` (reset_rows / save_rows / load_rows: distinct, not empty) and of load_rows' `entries` (one per row,
    repeats allowed): every refusal a caller can receive, with its full text."""
    import torch
    from lets_face_it_amd.stream import _index_list

    def rows(v, B=4):
        return _index_list("rows", v, B, "the session's batch")

    def entries(v, n, saved=3):
        return _index_list("entries", v, saved, "the saved rows", count=n, distinct=False)

    assert rows([2, 0]) == [2, 0] and rows((3,)) == [3] and rows(torch.tensor([1, 3])) == [1, 3] and rows(torch.tensor(2)) == [2]
    assert rows(torch.tensor([0, 1], dtype=torch.int16)) == [0, 1] and rows(range(4)) == [0, 1, 2, 3]
    assert entries([1, 1, 2], 3) == [1, 1, 2] and entries(torch.tensor([2, 2]), 2) == [2, 2] and entries(range(2), 2) == [0, 1]
    text = "expected a sequence of ints or a 1-D CPU integer tensor, got "
    for call, message in (
            (lambda: rows([]), "rows: empty list"),
            (lambda: rows(torch.zeros(0, dtype=torch.long)), "rows: empty list"),
            (lambda: rows([0, 4, -1]), "rows: [4, -1] outside the session's batch (0 .. 3)"),
            (lambda: rows([2, 0, 2, 1, 1]), "rows: [1, 2] listed more than once"),
            (lambda: rows([0, 7, 0]), "rows: [7] outside the session's batch (0 .. 3)"),   # the range before the repeats
            (lambda: rows(3), "rows: " + text + "3"),
            (lambda: rows([0, 1.0]), "rows: " + text + "[0, 1.0]"),
            (lambda: rows(torch.tensor([0.0, 1.0])), "rows: " + text + "(2,) torch.float32 on cpu"),
            (lambda: rows(torch.tensor([True, False])), "rows: " + text + "(2,) torch.bool on cpu"),
            (lambda: rows(torch.zeros(2, 2, dtype=torch.long)), "rows: " + text + "(2, 2) torch.int64 on cpu"),
            (lambda: entries([0], 2), "entries: 1 listed for 2 rows"),
            (lambda: entries([], 1), "entries: 0 listed for 1 rows"),
            (lambda: entries([0, 3], 2), "entries: [3] outside the saved rows (0 .. 2)"),
            (lambda: entries([0, 5, 1], 2), "entries: 3 listed for 2 rows"),               # the count before the range
            (lambda: entries(range(4), 4), "entries: [3] outside the saved rows (0 .. 2)"),
            (lambda: entries("ab", 2), "entries: " + text + "'ab'"),
            (lambda: entries(torch.tensor([0.5]), 1), "entries: " + text + "(1,) torch.float32 on cpu")):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == message
