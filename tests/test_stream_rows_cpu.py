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
