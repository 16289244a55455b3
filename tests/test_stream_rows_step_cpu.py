"""CPU: the per-row step of streaming sessions (SampleStream.step_rows) without a device - the C ABI's new entry points beside the
unchanged size queries, and the refusals of step_rows()'s arguments before anything touches a device."""
import os
import re
from argparse import Namespace

import pytest
import torch

import host_dispatch_expected as E
from lets_face_it_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(text, name):
    m = re.search(r"\b(?:int|long)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split())


def test_step_rows_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    sampler = _declaration(text, "lfi_flow_sample_seq_nll")
    new = _declaration(text, "lfi_flow_step_rows_from")
    # lfi_flow_sample_seq_nll's list, then the role words and the second work area in front of the stream
    assert new == sampler.replace("void* stream", "const int* observed, float* rows_work, void* stream")
    assert _declaration(text, "lfi_flow_step_rows_work_floats") == "const lfi_flow_dims* d"
    advance = _declaration(text, "lfi_stream_advance")
    rows = _declaration(text, "lfi_stream_advance_rows")
    assert rows == advance.replace("const float* noise", "int face_win, const float* noise") \
                          .replace("unsigned* guard_bits", "const unsigned char* observed, int* role, unsigned* guard_bits")
    for name in ("lfi_flow_step_rows_from", "lfi_flow_step_rows_work_floats", "lfi_stream_advance_rows"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    vp, i = _lib.C.c_void_p, _lib.C.c_int
    nll_args = L.lfi_flow_sample_seq_nll.argtypes
    assert L.lfi_flow_step_rows_from.argtypes == nll_args[:-1] + [vp, vp] + nll_args[-1:]
    assert L.lfi_flow_step_rows_work_floats.argtypes == L.lfi_flow_sample_nll_work_floats.argtypes
    adv = L.lfi_stream_advance.argtypes
    assert L.lfi_stream_advance_rows.argtypes == adv[:6] + [i] + adv[6:10] + [vp, vp] + adv[10:]


def test_step_rows_null_arguments_are_an_argument_error_and_the_pinned_size_queries_are_unchanged():
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    rows = {name: E.EXPECTED[0]["flow"][i] for i, (name, _) in enumerate(E.FLOW_DIMS)}
    for name in ("headline gemm_precision 0x0", "headline gemm_precision 0x5", "headline gemm_precision 0x9"):
        d = _lib.FlowDims(*by_name[name])
        ref = _lib.C.byref(d)
        assert L.lfi_flow_step_rows_work_floats(ref) > 0
        # every pointer null: an argument error, reported before any launch
        assert L.lfi_flow_step_rows_from(ref, None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, None, None, None, None, None, None,
                                         None, None, None, None) == -1
        p = _lib.FlowParams()
        # partly null: dims and params there, one frame asked for, every buffer missing
        assert L.lfi_flow_step_rows_from(ref, _lib.C.byref(p), None, None, 0, 0, None, None, None, 1, 0, 1, 0, None, None, None, None,
                                         None, None, None, None, None, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        got = [L.lfi_flow_prep_floats(ref), L.lfi_flow_sample_work_floats(ref), L.lfi_flow_sample_nll_work_floats(ref)]
        want = [rows[name][E.FLOW_QUERIES.index(q)] for q in ("prep_floats", "sample_work_floats", "sample_nll_work_floats")]
        assert got == want, (name, got, want)
    assert L.lfi_flow_step_rows_work_floats(None) == 0
    # the advance: all null, and a window table without the mask
    assert L.lfi_stream_advance_rows(4, 0, None, None, None, None, 0, None, None, 0, None, None, None, None, None) == -1
    assert L.lfi_stream_advance_rows(4, 1, None, None, None, None, 0, None, None, 8, None, None, None, None, None) == -1
    assert b"null" in L.lfi_last_error()


def _stub_session(B=3, C=16):
    """A SampleStream with just what step_rows() looks at before its first launch (no engine behind it)."""
    from lets_face_it_amd.stream import SampleStream
    st = SampleStream.__new__(SampleStream)
    st.eng = Namespace(spec=Namespace(C=C), param_version=0)
    st.closed, st.param_version, st._bound = False, 0, None
    st.B, st.mods, st.device = B, [], torch.device("cuda", 0)
    return st


def test_step_rows_refuses_bad_arguments_before_touching_a_device():
    st = _stub_session()
    face = torch.zeros(3, 16)
    mask = [True, False, True]
    # the role mask: length, dtype, device
    for bad in ([True, False], torch.zeros(4, dtype=torch.bool), torch.zeros(3, 1, dtype=torch.bool), []):
        with pytest.raises(ValueError, match=r"observed: expected 3 entries \(B,\)"):
            st.step_rows({}, face, bad)
    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), [1, 0, 1], [True, None, False],
                None, 1):
        with pytest.raises(TypeError, match="observed: expected a torch.bool tensor or a sequence of bools"):
            st.step_rows({}, face, bad)
    with pytest.raises(ValueError, match="observed: on meta, the session on cuda:0"):
        st.step_rows({}, face, torch.zeros(3, dtype=torch.bool, device="meta"))
    # the face and the noise, in the wording of step() / observe()
    with pytest.raises(ValueError, match=r"face: expected contiguous float32 GPU tensor \(B=3, 16\)"):
        st.step_rows({}, face, mask)                                  # a CPU tensor
    with pytest.raises(ValueError, match=r"face: expected contiguous float32 GPU tensor \(B=3, 16\).*\(3, 15\)"):
        st.step_rows({}, torch.zeros(3, 15), torch.tensor(mask))      # a wrong shape
    with pytest.raises(ValueError, match="face"):
        st.step_rows({}, None, mask)
    with pytest.raises(TypeError, match="frame must be a dict"):
        st.step_rows(None, face, mask)
    # a closed session, and one whose parameters changed since the open
    st.eng.param_version = 1
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_rows({}, face, mask)
    st.eng.param_version = 0
    st.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        st.step_rows({}, face, mask)
