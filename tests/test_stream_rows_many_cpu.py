"""CPU: per-row roles over a chunk of frames (SampleStream.step_rows_many) without a device - the two entry points of the C ABI
(lfi_stream_chunk_roles_in, the window launch in; lfi_flow_step_rows_seq, the rows chain frame by frame): declared, exported and bound,
their argument errors before any launch; the planner that splits a round between the chunk forward chain and the rows chain; and the
refusals of step_rows_many()'s arguments before anything touches a device."""
import os

import pytest
import torch

import host_dispatch_expected as E
from lets_face_it_amd import _lib
from lets_face_it_amd.stream import plan_rows_many
from test_stream_chunk_cpu import _declaration, _gpu, _stub_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lfi_stream_chunk_roles_in", "lfi_flow_step_rows_seq")


def test_both_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    L = _lib.lib()
    for name in NEW:
        _declaration(text, name)
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is _lib.C.c_int
    # the generated chunk's window launch with the role words added in front of the guard
    tail = "unsigned* guard_bits, void* stream"
    assert _declaration(text, "lfi_stream_chunk_roles_in") == _declaration(text, "lfi_stream_chunk_gen_in").replace(
        tail, "const int* roles, " + tail)
    gen_in = L.lfi_stream_chunk_gen_in.argtypes
    assert L.lfi_stream_chunk_roles_in.argtypes == gen_in[:-2] + [_lib.C.c_void_p] + gen_in[-2:]
    # the rows chain of a run of frames: the one-frame call's list, word for word
    assert _declaration(text, "lfi_flow_step_rows_seq") == _declaration(text, "lfi_flow_step_rows_from")
    assert L.lfi_flow_step_rows_seq.argtypes == L.lfi_flow_step_rows_from.argtypes
    # the existing entry points keep their argument counts
    assert len(L.lfi_stream_chunk_gen_in.argtypes) == 15 and len(L.lfi_stream_chunk_gen_out.argtypes) == 15
    assert len(L.lfi_flow_step_rows_from.argtypes) == 23 and len(L.lfi_stream_advance_rows.argtypes) == 15
    assert len(L.lfi_flow_score_seq_chunk.argtypes) == 21


def _tables(dim=4, hist=4, lead=0):
    c = _lib.C
    return (c.c_void_p * 1)(0x4000), (c.c_int * 1)(hist), (c.c_int * 1)(dim), (c.c_int * 1)(lead)


def test_roles_in_refuses_null_tables_before_any_launch():
    L = _lib.lib()
    c = _lib.C
    one_p, hist, dim, lead = _tables()
    null_p = (c.c_void_p * 1)()
    fake = c.c_void_p(0x8000)
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, None, None, None, None, None, None, 0, None, 4, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    # a null window / sequence inside the tables, a null source table, null noise
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, one_p, one_p, null_p, hist, dim, lead, 0, fake, 4, fake, None, None) == -1
    assert b"null pointer (window 0)" in L.lfi_last_error()
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, null_p, one_p, one_p, hist, dim, lead, 0, fake, 4, fake, None, None) == -1
    assert b"null pointer (window 0)" in L.lfi_last_error()
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, one_p, None, one_p, hist, dim, lead, 0, fake, 4, fake, None, None) == -1
    assert b"null pointer (source table / noise)" in L.lfi_last_error()
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, one_p, one_p, one_p, hist, dim, lead, 0, None, 4, fake, None, None) == -1
    assert b"null pointer (source table / noise)" in L.lfi_last_error()
    # null roles
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, one_p, one_p, one_p, hist, dim, lead, 0, fake, 4, None, None, None) == -1
    assert b"null pointer (roles)" in L.lfi_last_error()
    # unlike gen_in, the generated window needs its source: the given faces of the rows that observe
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 1, one_p, null_p, one_p, hist, dim, lead, 0, fake, 4, fake, None, None) == -1
    assert b"null pointer (source 0)" in L.lfi_last_error()
    two_p, half = (c.c_void_p * 2)(0x4000, 0x5000), (c.c_void_p * 2)(0x4000, None)
    two_h, two_d, two_l = (c.c_int * 2)(4, 4), (c.c_int * 2)(4, 4), (c.c_int * 2)(0, 1)
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 2, two_p, half, two_p, two_h, two_d, two_l, 1, fake, 4, fake, None, None) == -1
    assert b"null pointer (source 1)" in L.lfi_last_error()
    # and a conditioning window (not gen_win) its own
    other = (c.c_void_p * 2)(None, 0x5000)
    assert L.lfi_stream_chunk_roles_in(2, 3, 4, 2, two_p, other, two_p, two_h, two_d, two_l, 1, fake, 4, fake, None, None) == -1
    assert b"null pointer (source 0)" in L.lfi_last_error()


def test_roles_in_refuses_bad_shapes_before_any_launch():
    L = _lib.lib()
    c = _lib.C
    one_p, hist, dim, lead = _tables()
    fake = c.c_void_p(0x8000)

    def roles_in(B=2, n=3, start=4, count=1, gen_win=0, C=4):
        return L.lfi_stream_chunk_roles_in(B, n, start, count, one_p, one_p, one_p, hist, dim, lead, gen_win, fake, C, fake, None, None)

    for bad in (dict(n=0), dict(B=0), dict(count=9), dict(start=3), dict(gen_win=-1), dict(gen_win=1)):
        assert roles_in(**bad) == -1, bad
        assert b"lfi_stream_chunk_roles_in" in L.lfi_last_error(), bad
    assert roles_in(C=5) == -1                        # dim[gen_win] != C
    assert b"dim 4" in L.lfi_last_error() and b"C = 5" in L.lfi_last_error()
    assert roles_in(C=0) == -1
    # the prev_p1_face window's leading row does not count against the history: hist - lead <= start
    p, h5, d, l1 = _tables(hist=5, lead=1)
    assert L.lfi_stream_chunk_roles_in(2, 3, 3, 1, p, p, p, h5, d, l1, 0, fake, 4, fake, None, None) == -1


def test_the_rows_chain_of_a_run_refuses_no_frames_and_null_roles_and_the_one_frame_call_two_frames():
    L = _lib.lib()
    c = _lib.C
    by_name = dict(E.FLOW_DIMS)
    fake = c.c_void_p(0x8000)
    for name in ("headline gemm_precision 0x0", "headline gemm_precision 0x9"):
        d = _lib.FlowDims(*by_name[name])
        ref, p = c.byref(d), _lib.FlowParams()
        cst = fake if d.lstm else None

        def call(fn, nframes, observed=fake, seq_len=64):
            # every buffer there (never touched: the checks come first), hist1 = 1, start = 8
            return fn(ref, c.byref(p), fake, fake, 1 << 20, 1, fake, fake, fake, seq_len, 8, nframes, 1, fake, cst, None, None, fake, fake,
                      fake, observed, fake, None)

        assert call(L.lfi_flow_step_rows_seq, 0) == -1
        assert b"lfi_flow_step_rows_seq: 0 frames" in L.lfi_last_error()
        assert call(L.lfi_flow_step_rows_seq, -1) == -1
        assert call(L.lfi_flow_step_rows_seq, 2, observed=None) == -1
        assert b"lfi_flow_step_rows_seq: null pointer" in L.lfi_last_error()
        assert call(L.lfi_flow_step_rows_seq, 4, seq_len=11) == -1            # frames 8 .. 11 of an 11-frame sequence
        assert b"bad frame range" in L.lfi_last_error()
        assert L.lfi_flow_step_rows_seq(ref, None, None, None, 0, 0, None, None, None, 0, 0, 2, 0, None, None, None, None, None, None,
                                        None, None, None, None) == -1
        # the one-frame call is still the one-frame call
        assert call(L.lfi_flow_step_rows_from, 2) == -1
        assert b"lfi_flow_step_rows_from: 2 frames (one frame per call)" in L.lfi_last_error()
        assert call(L.lfi_flow_step_rows_from, 0) == -1
        assert call(L.lfi_flow_step_rows_from, 1, observed=None) == -1
        assert b"lfi_flow_step_rows_from: null pointer" in L.lfi_last_error()


def test_the_planner():
    T, F = True, False
    flags = [T, T, F, T, F, F, T, T, T]
    assert plan_rows_many(flags, 2) == [("observe", 0, 2), ("rows", 2, 4), ("observe", 6, 3)]
    assert plan_rows_many(flags, 0) == [("rows", 0, 9)]
    assert plan_rows_many(flags, 3) == [("rows", 0, 6), ("observe", 6, 3)]
    assert plan_rows_many(flags, 1) == [("observe", 0, 2), ("rows", 2, 1), ("observe", 3, 1), ("rows", 4, 2), ("observe", 6, 3)]
    assert plan_rows_many([T] * 5, 2) == [("observe", 0, 5)]
    assert plan_rows_many([F] * 5, 2) == [("rows", 0, 5)]
    assert plan_rows_many([T] * 5, 0) == [("rows", 0, 5)]
    assert plan_rows_many([T], 2) == [("rows", 0, 1)] and plan_rows_many([F], 2) == [("rows", 0, 1)]
    assert plan_rows_many([T], 1) == [("observe", 0, 1)]
    assert plan_rows_many(torch.tensor(flags), 2) == plan_rows_many(flags, 2)
    # every frame once, in order, whatever the flags
    g = torch.Generator().manual_seed(0)
    for n in (1, 2, 7, 33):
        for min_run in (0, 1, 2, 4):
            fl = (torch.rand(n, generator=g) < 0.6).tolist()
            plan = plan_rows_many(fl, min_run)
            at = 0
            for kind, first, count in plan:
                assert kind in ("observe", "rows") and first == at and count >= 1
                if kind == "observe":
                    assert min_run > 0 and count >= min_run and all(fl[first:first + count])
                    assert (first == 0 or not fl[first - 1]) and (first + count == n or not fl[first + count])      # maximal
                at += count
            assert at == n
            assert all(a[0] != b[0] or a[0] == "observe" for a, b in zip(plan, plan[1:]))      # rows runs are merged


def test_the_observe_run_switch(monkeypatch):
    from lets_face_it_amd.stream import SampleStream
    monkeypatch.delenv("LFI_ROWS_MANY_OBSERVE_RUN", raising=False)
    assert SampleStream._rows_many_min_run() == 2
    monkeypatch.setenv("LFI_ROWS_MANY_OBSERVE_RUN", "0")
    assert SampleStream._rows_many_min_run() == 0
    monkeypatch.setenv("LFI_ROWS_MANY_OBSERVE_RUN", "5")
    assert SampleStream._rows_many_min_run() == 5
    monkeypatch.setenv("LFI_ROWS_MANY_OBSERVE_RUN", "-1")
    with pytest.raises(ValueError, match="LFI_ROWS_MANY_OBSERVE_RUN"):
        SampleStream._rows_many_min_run()


def test_step_rows_many_refuses_bad_arguments_before_touching_a_device():
    st = _stub_session()
    ok = {"p1_speech": _gpu(3, 4, 5), "p2_face": _gpu(3, 4, 16)}
    faces = _gpu(3, 4, 16)
    mask = [[True, False, True]] * 4
    for bad in (None, [ok["p1_speech"], ok["p2_face"]], ok["p1_speech"]):
        with pytest.raises(TypeError, match="frames must be a dict"):
            st.step_rows_many(bad, faces, mask)
    with pytest.raises(KeyError, match="p2_face"):
        st.step_rows_many({"p1_speech": ok["p1_speech"]}, faces, mask)
    # faces: n comes from them, in the wording of observe_many()
    with pytest.raises(ValueError, match=r"faces: expected contiguous float32 GPU tensor \(B=3, n>=1, 16\)"):
        st.step_rows_many(ok, torch.zeros(3, 4, 16), mask)                    # a CPU tensor
    with pytest.raises(ValueError, match=r"faces: expected contiguous float32 GPU tensor \(B=3, n>=1, 16\).*\(3, 16\)"):
        st.step_rows_many(ok, _gpu(3, 16), mask)                              # a wrong rank: one frame is step_rows()'s
    with pytest.raises(ValueError, match=r"faces: .*\(3, 0, 16\)"):
        st.step_rows_many(ok, _gpu(3, 0, 16), [])
    with pytest.raises(ValueError, match=r"faces: .*\(4, 4, 16\)"):
        st.step_rows_many(ok, _gpu(4, 4, 16), mask)                           # another batch
    with pytest.raises(ValueError, match=r"faces: .*float64"):
        st.step_rows_many(ok, _gpu(3, 4, 16, dtype=torch.float64), mask)
    with pytest.raises(ValueError, match="faces"):
        st.step_rows_many(ok, None, mask)
    # the frames, against the faces' n
    with pytest.raises(ValueError, match=r"p1_speech: expected contiguous float32 GPU tensor \(B=3, n=4, 5\).*\(3, 5\)"):
        st.step_rows_many(dict(ok, p1_speech=_gpu(3, 5)), faces, mask)
    with pytest.raises(ValueError, match=r"p2_face: expected contiguous float32 GPU tensor \(B=3, n=4, 16\).*\(3, 5, 16\)"):
        st.step_rows_many(dict(ok, p2_face=_gpu(3, 5, 16)), faces, mask)      # a wrong n in one modality
    with pytest.raises(ValueError, match=r"p1_speech: .*\(4, 4, 5\)"):
        st.step_rows_many(dict(ok, p1_speech=_gpu(4, 4, 5)), faces, mask)
    with pytest.raises(ValueError, match=r"p1_speech: .*float16"):
        st.step_rows_many(dict(ok, p1_speech=_gpu(3, 4, 5, dtype=torch.float16)), faces, mask)
    with pytest.raises(ValueError, match=r"p1_speech: .* on cpu"):
        st.step_rows_many(dict(ok, p1_speech=torch.zeros(3, 4, 5)), faces, mask)
    with pytest.raises(ValueError, match="p2_face: expected contiguous"):
        st.step_rows_many(dict(ok, p2_face=_gpu(3, 16, 4).transpose(1, 2)), faces, mask)
    # noise: (n, B, C) = (4, 3, 16), frame-major, in the wording of step_many()
    with pytest.raises(ValueError, match=r"noise: expected contiguous float32 GPU tensor \(n=4, B=3, 16\).*frame-major.*\(3, 4, 16\)"):
        st.step_rows_many(ok, faces, mask, _gpu(3, 4, 16))                    # (B, n, C): the orientation of `out`, not of the noise
    with pytest.raises(ValueError, match=r"noise: .*\(5, 3, 16\)"):
        st.step_rows_many(ok, faces, mask, _gpu(5, 3, 16))
    with pytest.raises(ValueError, match=r"noise: .*\(4, 3, 15\)"):
        st.step_rows_many(ok, faces, mask, _gpu(4, 3, 15))
    with pytest.raises(ValueError, match=r"noise: .*\(3, 16\)"):
        st.step_rows_many(ok, faces, mask, _gpu(3, 16))
    with pytest.raises(ValueError, match=r"noise: .*float64"):
        st.step_rows_many(ok, faces, mask, _gpu(4, 3, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"noise: .* on cpu"):
        st.step_rows_many(ok, faces, mask, torch.zeros(4, 3, 16))
    with pytest.raises(ValueError, match="noise: expected contiguous"):
        st.step_rows_many(ok, faces, mask, _gpu(3, 4, 16).transpose(0, 1))
    # observed: host data, (n, B) = (4, 3), frame-major
    with pytest.raises(ValueError, match=r"observed: on cuda:0.*step_rows\(\) is the call for device-resident masks"):
        st.step_rows_many(ok, faces, _gpu(4, 3, dtype=torch.bool))
    for bad in (torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.uint8), torch.zeros(4, 3, dtype=torch.int64)):
        with pytest.raises(TypeError, match="observed: expected an .n, B. CPU torch.bool tensor"):
            st.step_rows_many(ok, faces, bad)
    for bad in (torch.zeros(3, 4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), torch.zeros(5, 3, dtype=torch.bool),
                torch.zeros(4, 3, 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"observed: expected \(n, B\) = \(4, 3\)"):
            st.step_rows_many(ok, faces, bad)
    for bad in ([[True, False, True]] * 3, [[True, False, True], [True, False], [True] * 3, [False] * 3], [[True] * 4] * 3, []):
        with pytest.raises(ValueError, match=r"observed: expected \(n, B\) = \(4, 3\)"):
            st.step_rows_many(ok, faces, bad)                                 # too few frames, ragged, (B, n)
    for bad in ([[1, 0, 1]] * 4, [[True, None, False]] * 4, [[True, False, 0.0]] * 4):
        with pytest.raises(TypeError, match="observed: expected an .n, B. CPU torch.bool tensor"):
            st.step_rows_many(ok, faces, bad)                                 # non-bool entries
    for bad in (None, 1, [True, False, True, True]):
        with pytest.raises(TypeError, match="observed"):
            st.step_rows_many(ok, faces, bad)
    # a session whose parameters changed since the open, and a closed one
    st.eng.param_version = 1
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_rows_many(ok, faces, mask)
    st.eng.param_version = 0
    st.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        st.step_rows_many(ok, faces, mask)
