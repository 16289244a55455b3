"""CPU: moving live rows between streaming sampling sessions without a device - the record layout (lfi_stream_row_floats), the C
entry points' argument checks (no launch), the binding, the model API's surface and StreamRows' host round trip."""
import ctypes
import io

import torch

from lets_face_it_amd import _lib


def _tables(count, hist, dim):
    n = max(count, 1)
    win, hs, ds = (ctypes.c_void_p * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
    for i in range(min(count, n)):
        win[i], hs[i], ds[i] = 0x1000 * (i + 1), hist, dim
    return win, hs, ds


def _save_rows(B=4, rows=(1,), count=2, hist=3, dim=4, Ks=2, H=8, ld=None, h=0x5000, out=0x9000, lstm=False, nb=False):
    L = _lib.lib()
    win, hs, ds = _tables(count, hist, dim)
    R = count * hist * dim + Ks * H * (2 if lstm else 1) + (1 if nb else 0)
    ra = (ctypes.c_int * max(len(rows), 1))(*rows)
    rc = L.lfi_stream_save_rows(B, len(rows), ra, count, win, hs, ds, h, 0x6000 if lstm else None, Ks, H, 0x7000 if nb else None, 0,
                                out, R if ld is None else ld, None)
    return rc, L.lfi_last_error()


def _load_rows(B=4, rows=(1,), entries=None, nentries=3, count=2, hist=3, dim=4, Ks=2, H=8, ld=None, h=0x5000, src=0x9000, lstm=False,
               nb=False):
    L = _lib.lib()
    win, hs, ds = _tables(count, hist, dim)
    R = count * hist * dim + Ks * H * (2 if lstm else 1) + (1 if nb else 0)
    entries = tuple(range(len(rows))) if entries is None else entries
    ra = (ctypes.c_int * max(len(rows), 1))(*rows)
    ea = (ctypes.c_int * max(len(entries), 1))(*entries)
    rc = L.lfi_stream_load_rows(B, len(rows), ra, ea, nentries, count, win, hs, ds, h, 0x6000 if lstm else None, Ks, H,
                                0x7000 if nb else None, src, R if ld is None else ld, None, None)
    return rc, L.lfi_last_error()


def test_stream_row_floats_is_the_sum_of_the_record():
    L = _lib.lib()
    hist = (ctypes.c_int * 4)(24, 24, 24, 6)
    dim = (ctypes.c_int * 4)(50, 27, 27, 50)
    wins = 24 * 50 + 24 * 27 + 24 * 27 + 6 * 50
    Ks, H = 16, 512
    assert L.lfi_stream_row_floats(4, hist, dim, Ks, H, 0, 0) == wins + Ks * H
    assert L.lfi_stream_row_floats(4, hist, dim, Ks, H, 1, 0) == wins + 2 * Ks * H
    assert L.lfi_stream_row_floats(4, hist, dim, Ks, H, 0, 1) == wins + Ks * H + 1
    assert L.lfi_stream_row_floats(4, hist, dim, Ks, H, 1, 1) == wins + 2 * Ks * H + 1
    assert L.lfi_stream_row_floats(1, hist, dim, 2, 8, 0, 0) == 24 * 50 + 16
    assert L.lfi_stream_row_floats(0, None, None, 2, 8, 1, 1) == 33
    for args, text in (((9, hist, dim, Ks, H, 0, 0), b"9 windows"), ((4, hist, dim, 0, H, 0, 0), b"Ks = 0"),
                       ((4, hist, dim, Ks, -1, 0, 0), b"H = -1"), ((2, None, dim, Ks, H, 0, 0), b"null window table")):
        assert L.lfi_stream_row_floats(*args) == -1 and text in L.lfi_last_error(), args
    hist[2] = 0
    assert L.lfi_stream_row_floats(4, hist, dim, Ks, H, 0, 0) == -1 and b"window 2: hist 0" in L.lfi_last_error()


def test_stream_save_rows_reports_argument_errors_without_launching():
    for kwargs, text in ((dict(B=0), b"batch 0"), (dict(rows=()), b"0 rows"), (dict(rows=(4,)), b"is 4, outside the batch"),
                         (dict(rows=(0, -1)), b"is -1, outside the batch"), (dict(rows=(2, 0, 2)), b"row 2 is listed twice"),
                         (dict(rows=(0, 1, 2, 3, 1)), b"5 rows"), (dict(count=9), b"9 windows"), (dict(hist=0), b"hist 0"),
                         (dict(dim=-1), b"dim -1"), (dict(Ks=0), b"Ks = 0"), (dict(H=-2), b"H = -2"),
                         (dict(ld=39), b"record stride 39 below the record's 40"),
                         (dict(ld=56, lstm=True, nb=True), b"record stride 56 below the record's 57"),
                         (dict(h=None), b"null h"), (dict(out=None), b"null out")):
        rc, msg = _save_rows(**kwargs)
        assert rc == -1 and b"lfi_stream_save_rows" in msg and text in msg, (kwargs, msg)


def test_stream_load_rows_reports_argument_errors_without_launching():
    for kwargs, text in ((dict(B=0), b"batch 0"), (dict(rows=()), b"0 rows"), (dict(rows=(4,)), b"is 4, outside the batch"),
                         (dict(rows=(0, -1)), b"is -1, outside the batch"), (dict(rows=(2, 0, 2)), b"row 2 is listed twice"),
                         (dict(rows=(0, 1, 2, 3, 1)), b"5 rows"), (dict(count=9), b"9 windows"), (dict(hist=0), b"hist 0"),
                         (dict(dim=-1), b"dim -1"), (dict(Ks=0), b"Ks = 0"), (dict(H=-2), b"H = -2"),
                         (dict(ld=39), b"record stride 39 below the record's 40"),
                         (dict(ld=56, lstm=True, nb=True), b"record stride 56 below the record's 57"),
                         (dict(h=None), b"null h"), (dict(src=None), b"null in"),
                         (dict(rows=(0, 1), entries=(0, 3)), b"is 3, outside the saved entries"),
                         (dict(rows=(0, 1), entries=(-1, 0)), b"is -1, outside the saved entries"),
                         (dict(nentries=0), b"0 saved entries")):
        rc, msg = _load_rows(**kwargs)
        assert rc == -1 and b"lfi_stream_load_rows" in msg and text in msg, (kwargs, msg)


def test_stream_load_rows_accepts_a_repeated_entry():
    """A branch lists one entry for several rows. The entries are checked before the record stride: a call with a repeated entry and
    too short a stride is refused for the stride, so the repeat passed (no launch either way)."""
    rc, msg = _load_rows(rows=(0, 1, 2), entries=(1, 1, 1), ld=39)
    assert rc == -1 and b"record stride 39" in msg, msg
    rc, msg = _load_rows(rows=(0, 1, 2), entries=(1, 3, 1), ld=39)
    assert rc == -1 and b"outside the saved entries" in msg, msg


def test_stream_state_entry_points_are_bound_and_declared():
    L = _lib.lib()
    for name in ("lfi_stream_row_floats", "lfi_stream_save_rows", "lfi_stream_load_rows"):
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    from lets_face_it_amd import engine
    assert callable(getattr(engine.SampleStream, "save_rows", None))
    assert callable(getattr(engine.SampleStream, "load_rows", None))


def test_stream_rows_survive_the_host_round_trip():
    from lets_face_it_amd.engine import StreamRows
    sig = (6, 8, 2, "lstm", True, (("p2_face", 3, 6), ("p1_speech", 3, 4)), 2, 3 * 6 + 3 * 4 + 3 * 6 + 2 * 2 * 8 + 1)
    data = torch.randn(5, sig[-1], generator=torch.Generator().manual_seed(1))
    rows = StreamRows(data, sig)
    assert len(rows) == 5 and rows.signature == sig
    d = rows.cpu().state_dict()
    assert sum(torch.is_tensor(v) for v in d.values()) == 1
    f = io.BytesIO()
    torch.save(d, f)
    f.seek(0)
    back = StreamRows.from_state_dict(torch.load(f))
    assert back.signature == sig and len(back) == 5
    assert back.data.dtype == torch.float32 and torch.equal(back.data, data)
    pick = back.select([4, 0, 4])
    assert pick.signature == sig and torch.equal(pick.data, data[[4, 0, 4]])
