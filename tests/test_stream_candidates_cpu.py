"""CPU: N candidates per frame of streaming sessions (SampleStream.step_candidates / commit / step_best_of) without a device - the C
ABI's new entry points beside the unchanged size queries, and the refusals of the new calls' arguments and the pending rule before
anything touches a device."""
import os
import re
from argparse import Namespace

import pytest
import torch

import host_dispatch_expected as E
from lets_face_it_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("headline gemm_precision 0x0", "headline gemm_precision 0x5", "headline gemm_precision 0x9")


def _declaration(text, name):
    m = re.search(r"\b(?:int|long)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split())


def test_candidate_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    sampler = _declaration(text, "lfi_flow_sample_seq_nll")
    new = _declaration(text, "lfi_flow_sample_cand_from")
    # lfi_flow_sample_seq_nll's list (one frame per call), then the candidates' count, outputs and work area in front of the stream
    assert new == sampler.replace("void* stream", "int ncand, float* cand_frames, float* cand_nll, float* cand_h, float* cand_c, "
                                                  "float* cand_work, void* stream")
    assert _declaration(text, "lfi_flow_sample_cand_work_floats") == "const lfi_flow_dims* d, int ncand"
    commit = _declaration(text, "lfi_stream_commit_cand")
    assert commit == ("int B, int ncand, int C, int Ks, int H, const int* choice, const float* cand_frames, const float* cand_nll, "
                      "const float* cand_h, const float* cand_c, float* face_win, int hist, float* h, float* cstate, float* out_frame, "
                      "float* out_nll, int* out_choice, unsigned* guard_bits, void* stream")
    for name in ("lfi_flow_sample_cand_from", "lfi_flow_sample_cand_work_floats", "lfi_stream_commit_cand"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    vp, i = _lib.C.c_void_p, _lib.C.c_int
    nll_args = L.lfi_flow_sample_seq_nll.argtypes
    assert L.lfi_flow_sample_cand_from.argtypes == nll_args[:-1] + [i, vp, vp, vp, vp, vp] + nll_args[-1:]
    assert L.lfi_flow_sample_cand_work_floats.argtypes == L.lfi_flow_sample_nll_work_floats.argtypes + [i]
    assert L.lfi_flow_sample_cand_work_floats.restype == _lib.C.c_long
    assert L.lfi_stream_commit_cand.argtypes == [i] * 5 + [vp] * 6 + [i] + [vp] * 7


def test_candidate_null_arguments_are_an_argument_error_and_the_pinned_size_queries_are_unchanged():
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    rows = {name: E.EXPECTED[0]["flow"][i] for i, (name, _) in enumerate(E.FLOW_DIMS)}
    for name in HEADLINE:
        d = _lib.FlowDims(*by_name[name])
        ref = _lib.C.byref(d)
        # every pointer null: an argument error, reported before any launch
        assert L.lfi_flow_sample_cand_from(ref, None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, None, None, None, None, None, None,
                                           None, 0, None, None, None, None, None, None) == -1
        p = _lib.FlowParams()
        # partly null: dims and params there, one frame and four candidates asked for, every buffer missing
        assert L.lfi_flow_sample_cand_from(ref, _lib.C.byref(p), None, None, 0, 0, None, None, None, 1, 0, 1, 0, None, None, None, None,
                                           None, None, None, 4, None, None, None, None, None, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        got = [L.lfi_flow_prep_floats(ref), L.lfi_flow_sample_work_floats(ref), L.lfi_flow_sample_nll_work_floats(ref)]
        want = [rows[name][E.FLOW_QUERIES.index(q)] for q in ("prep_floats", "sample_work_floats", "sample_nll_work_floats")]
        assert got == want, (name, got, want)
        # the candidate work area: positive at the headline dims, growing with the candidates
        sizes = [L.lfi_flow_sample_cand_work_floats(ref, n) for n in (1, 2, 3, 8, 17, 256)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert L.lfi_flow_sample_cand_work_floats(ref, 0) == 0
    assert L.lfi_flow_sample_cand_work_floats(None, 4) == 0
    # the commit: all null, and sizes without buffers
    assert L.lfi_stream_commit_cand(0, 0, 0, 0, 0, None, None, None, None, None, None, 0, None, None, None, None, None, None, None) == -1
    assert L.lfi_stream_commit_cand(5, 3, 6, 2, 7, None, None, None, None, None, None, 2, None, None, None, None, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()


def _stub_session(B=3, C=16):
    """A SampleStream with just what the candidate calls look at before their first launch (no engine behind it)."""
    from lets_face_it_amd.stream import SampleStream
    st = SampleStream.__new__(SampleStream)
    st.eng = Namespace(spec=Namespace(C=C), param_version=0)
    st.closed, st.param_version, st._bound = False, 0, None
    st.B, st.mods, st.device = B, [], torch.device("cuda", 0)
    return st


def test_step_candidates_refuses_bad_arguments_before_touching_a_device():
    st = _stub_session()
    for call in (st.step_candidates, st.step_best_of):
        for bad in (2.0, "4", None, True, torch.tensor(4)):
            with pytest.raises(TypeError, match="ncand: expected an int"):
                call({}, bad)
        for bad in (0, -1, 257):
            with pytest.raises(ValueError, match=r"ncand: -?\d+ outside 1 \.\. 256"):
                call({}, bad)
        with pytest.raises(TypeError, match="frame must be a dict"):
            call(None, 4)
        # the noise: (B, ncand, C) contiguous float32 on the session's device
        for bad in (torch.zeros(3, 4, 16), torch.zeros(3, 16), torch.zeros(4, 3, 16), torch.zeros(3, 4, 15), [0.0], 1.0):
            with pytest.raises(ValueError, match=r"noise: expected contiguous float32 GPU tensor \(B=3, ncand=4, 16\)"):
                call({}, 4, bad)
    st.eng.param_version = 1
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_candidates({}, 4)
    st.eng.param_version = 0
    st.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        st.step_candidates({}, 4)
    with pytest.raises(RuntimeError, match="closed"):
        st.commit()


def test_commit_refuses_bad_choices_and_a_session_without_candidates():
    st = _stub_session()
    with pytest.raises(RuntimeError, match="without pending candidates"):
        st.commit()
    with pytest.raises(RuntimeError, match="without pending candidates"):
        st.commit([0, 0, 0])
    st._pending = 4
    # host data in the wording of _index_list: B entries, each one of the row's candidates; repeats are fine
    with pytest.raises(ValueError, match="choice: 2 listed for 3 rows"):
        st.commit([0, 1])
    with pytest.raises(ValueError, match=r"choice: \[4\] outside the row's candidates \(0 \.\. 3\)"):
        st.commit([0, 4, 1])
    with pytest.raises(ValueError, match=r"choice: \[-1\] outside the row's candidates"):
        st.commit(torch.tensor([0, -1, 1]))
    with pytest.raises(ValueError, match="choice: expected a sequence of ints or a 1-D CPU integer tensor"):
        st.commit(torch.zeros(3))
    with pytest.raises(ValueError, match="choice: expected a sequence of ints or a 1-D CPU integer tensor"):
        st.commit([0.5, 1, 2])
    with pytest.raises(ValueError, match="choice: expected a sequence of ints or a 1-D CPU integer tensor"):
        st.commit(torch.zeros(3, 1, dtype=torch.int32))
    assert st._pending == 4
    st.eng.param_version = 1
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.commit()


def test_pending_candidates_refuse_every_other_call_before_touching_a_device():
    st = _stub_session()
    st._pending = 5
    face, seed = torch.zeros(3, 16), {"p1_face": torch.zeros(3, 4, 16)}
    calls = (lambda: st.step({}), lambda: st.observe({}, face), lambda: st.step_rows({}, face, [True, False, True]),
             lambda: st.step_candidates({}, 5), lambda: st.step_best_of({}, 5), lambda: st.step_many({}),
             lambda: st.observe_many({}, torch.zeros(3, 2, 16)), lambda: st.step_rows_many({}, torch.zeros(3, 2, 16), [[True] * 3] * 2),
             lambda: st.save_rows([0]), lambda: st.load_rows([0], None), lambda: st.reset_rows([0], seed))
    for call in calls:
        with pytest.raises(RuntimeError, match=r"5 candidates per row are pending \(step_candidates\): commit\(\)"):
            call()
    assert st._pending == 5
