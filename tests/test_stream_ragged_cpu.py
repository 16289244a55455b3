"""CPU: ragged chunks (SampleStream.observe_many with lengths) without a device - the C ABI's new entry points beside the unchanged
dense ones, their argument errors before any launch, the refusals of the lengths argument before anything touches a device, and the
register budget of the new chain kernel."""
import os
import re
import subprocess
import sys

import pytest
import torch

import host_dispatch_expected as E
from lets_face_it_amd import _lib
from test_stream_chunk_cpu import _declaration, _gpu, _stub_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("lfi_flow_score_seq_chunk_rows", "lfi_flow_score_seq_chunk"), ("lfi_stream_chunk_in_rows", "lfi_stream_chunk_in"),
         ("lfi_stream_chunk_out_rows", "lfi_stream_chunk_out"))


def test_ragged_entry_points_are_declared_bound_and_the_dense_ones_plus_lengths():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    L = _lib.lib()
    for rows, dense in PAIRS:
        assert rows in _lib.EXPORTS and dense in _lib.EXPORTS
        want = _declaration(text, dense)
        assert want.endswith(", void* stream")
        assert _declaration(text, rows) == want[:-len(", void* stream")] + ", const int* lengths, void* stream"
        a, b = getattr(L, rows).argtypes, getattr(L, dense).argtypes
        assert list(a) == list(b[:-1]) + [_lib.C.c_void_p, b[-1]] and getattr(L, rows).restype is getattr(L, dense).restype
    # the dense chunk chain is still lfi_flow_score_seq_from's declaration with the work area's name swapped
    assert _declaration(text, "lfi_flow_score_seq_chunk") == \
        _declaration(text, "lfi_flow_score_seq_from").replace("float* score_work", "float* chunk_work")


def test_ragged_null_arguments_are_an_argument_error_and_the_pinned_size_queries_are_unchanged():
    L = _lib.lib()
    c = _lib.C
    by_name = dict(E.FLOW_DIMS)
    rows = {name: E.EXPECTED[0]["flow"][i] for i, (name, _) in enumerate(E.FLOW_DIMS)}
    for name in ("headline gemm_precision 0x0", "headline gemm_precision 0x5", "headline gemm_precision 0x9"):
        d = _lib.FlowDims(*by_name[name])
        ref = c.byref(d)
        assert L.lfi_flow_score_seq_chunk_rows(ref, None, None, None, 0, 0, None, None, 0, 0, 0, 0, None, None, None, None, None, None,
                                               None, None, None, None) == -1
        p = _lib.FlowParams()
        assert L.lfi_flow_score_seq_chunk_rows(ref, c.byref(p), None, None, 0, 1, None, None, 2, 1, 1, 0, None, None, None, None, None,
                                               None, None, None, None, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        # the dense call's argument errors are what they were
        assert L.lfi_flow_score_seq_chunk(ref, c.byref(p), None, None, 0, 1, None, None, 2, 1, 1, 0, None, None, None, None, None,
                                          None, None, None, None) == -1
        assert b"lfi_flow_score_seq_chunk: null pointer" in L.lfi_last_error()
        got = [L.lfi_flow_prep_floats(ref), L.lfi_flow_sample_work_floats(ref), L.lfi_flow_sample_nll_work_floats(ref)]
        want = [rows[name][E.FLOW_QUERIES.index(q)] for q in ("prep_floats", "sample_work_floats", "sample_nll_work_floats")]
        assert got == want, (name, got, want)


def test_ragged_window_launches_refuse_null_tables_and_null_lengths_before_any_launch():
    L = _lib.lib()
    c = _lib.C
    one_p, one_i = (c.c_void_p * 1)(0x4000), (c.c_int * 1)(4)
    zero_i, null_p = (c.c_int * 1)(0), (c.c_void_p * 1)()
    lengths = c.c_void_p(0x8000)
    assert L.lfi_stream_chunk_in_rows(2, 3, 4, 1, None, None, None, None, None, None, None, lengths, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_out_rows(2, 3, 4, 1, None, None, None, None, None, None, lengths, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_in_rows(2, 3, 4, 1, one_p, null_p, one_p, one_i, one_i, zero_i, None, lengths, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_out_rows(2, 3, 4, 1, one_p, null_p, one_i, one_i, zero_i, None, lengths, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    # complete tables, no lengths
    assert L.lfi_stream_chunk_in_rows(2, 3, 4, 1, one_p, one_p, one_p, one_i, one_i, zero_i, None, None, None) == -1
    assert b"lfi_stream_chunk_in_rows: null pointer (lengths)" in L.lfi_last_error()
    assert L.lfi_stream_chunk_out_rows(2, 3, 4, 1, one_p, one_p, one_i, one_i, zero_i, None, None, None) == -1
    assert b"lfi_stream_chunk_out_rows: null pointer (lengths)" in L.lfi_last_error()
    for bad in ((2, 0, 4, 1), (0, 3, 4, 1), (2, 3, 4, 9), (2, 3, 3, 1)):        # no frames, no batch, too many windows, hist > start
        assert L.lfi_stream_chunk_in_rows(*bad, one_p, one_p, one_p, one_i, one_i, zero_i, None, lengths, None) == -1, bad
        assert L.lfi_stream_chunk_out_rows(*bad, one_p, one_p, one_i, one_i, zero_i, None, lengths, None) == -1, bad
        # ... as the dense launches refuse them
        assert L.lfi_stream_chunk_in(*bad, one_p, one_p, one_p, one_i, one_i, zero_i, None, None) == -1, bad
        assert L.lfi_stream_chunk_out(*bad, one_p, one_p, one_i, one_i, zero_i, None, None) == -1, bad


def test_lengths_are_refused_before_anything_touches_a_device():
    st = _stub_session()
    ok = {"p1_speech": _gpu(3, 4, 5), "p2_face": _gpu(3, 4, 16)}
    faces = _gpu(3, 4, 16)
    refused = (ValueError, TypeError)
    with pytest.raises(refused, match=r"lengths: 2 listed for 3 rows"):
        st.observe_many(ok, faces, lengths=[1, 2])
    with pytest.raises(refused, match=r"lengths: 4 listed for 3 rows"):
        st.observe_many(ok, faces, lengths=torch.tensor([1, 2, 3, 4]))
    with pytest.raises(refused, match=r"lengths: \[-1\] outside the chunk's frames \(0 \.\. 4\)"):
        st.observe_many(ok, faces, lengths=[4, -1, 0])
    with pytest.raises(refused, match=r"lengths: \[5\] outside the chunk's frames \(0 \.\. 4\)"):
        st.observe_many(ok, faces, lengths=torch.tensor([0, 5, 4]))
    with pytest.raises(refused, match="lengths: expected a sequence of ints"):
        st.observe_many(ok, faces, lengths=[True, False, True])
    with pytest.raises(refused, match="lengths: expected a sequence of ints.*torch.bool"):
        st.observe_many(ok, faces, lengths=torch.tensor([True, False, True]))
    with pytest.raises(refused, match="lengths: expected a sequence of ints"):
        st.observe_many(ok, faces, lengths=[1.0, 2.0, 3.0])
    with pytest.raises(refused, match="lengths: expected a sequence of ints.*float32"):
        st.observe_many(ok, faces, lengths=torch.tensor([1.0, 2.0, 3.0]))
    with pytest.raises(refused, match=r"lengths: expected a sequence of ints.*\(3, 1\)"):
        st.observe_many(ok, faces, lengths=torch.tensor([[1], [2], [3]]))
    with pytest.raises(refused, match="lengths: expected a sequence of ints.*cuda:0"):
        st.observe_many(ok, faces, lengths=_gpu(3, dtype=torch.int32))
    with pytest.raises(refused, match="lengths: expected a sequence of ints"):
        st.observe_many(ok, faces, lengths=3)
    # the other arguments are checked as before, with lengths given
    with pytest.raises(ValueError, match=r"p2_face: expected contiguous float32 GPU tensor \(B=3, n=4, 16\).*\(3, 5, 16\)"):
        st.observe_many(dict(ok, p2_face=_gpu(3, 5, 16)), faces, lengths=[1, 2, 3])
    with pytest.raises(TypeError, match="return_z"):
        st.observe_many(ok, faces, return_z=1, lengths=[1, 2, 3])


def test_good_lengths_and_none_go_on_to_the_launches(monkeypatch):
    """What passes the checks reaches the first thing behind them (the stub has no engine: _chunk_cap is made to say so) - with
    lengths=None as without the keyword, the dense call's path."""
    from lets_face_it_amd.stream import SampleStream

    class Reached(Exception):
        pass

    def cap(self):
        raise Reached()
    monkeypatch.setattr(SampleStream, "_chunk_cap", cap)
    st = _stub_session()
    ok = {"p1_speech": _gpu(3, 4, 5), "p2_face": _gpu(3, 4, 16)}
    faces = _gpu(3, 4, 16)
    for kw in ({}, {"lengths": None}, {"lengths": [4, 0, 2]}, {"lengths": (0, 0, 0)}, {"lengths": torch.tensor([1, 4, 0])},
               {"lengths": torch.tensor([1, 4, 0], dtype=torch.int32)}, {"return_z": True, "lengths": range(3)}):
        with pytest.raises(Reached):
            st.observe_many(ok, faces, **kw)
    assert st._check_lengths(torch.tensor([1, 4, 0]), 4) == [1, 4, 0] and st._check_lengths(range(3), 4) == [0, 1, 2]


def test_the_ragged_chain_kernels_stay_out_of_scratch():
    """As test_the_sequence_chain_kernels_stay_out_of_scratch for the dense chunk chain: the row-length variant of the frame loop
    (GRU exact, GRU fp16 pieces, LSTM) keeps its masks out of the vector registers' way. Compiles the unit for gfx950; no device."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "lets_face_it_amd", "csrc", "lfi_flow_chunk_rows.hip"), "flow_fwd_seq_rows_chain_kernel"],
                         capture_output=True, text=True, check=True).stdout
    rows = [line for line in out.splitlines() if "flow_fwd_seq_rows_chain_kernel" in line]
    assert len(rows) == 3, out
    for line in rows:
        m = re.search(r"vgpr\s+(\d+)\s+agpr\s+(\d+)\s+spill\s+(\d+)\s+scratch\s+(\d+)", line)
        assert m, line
        vgpr, agpr, spill, scratch = (int(v) for v in m.groups())
        assert spill == 0 and scratch == 0 and vgpr + agpr <= 256, line
