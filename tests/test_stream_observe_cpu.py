"""CPU: the teacher-forced step of streaming sessions (SampleStream.observe) without a device - the C ABI's new entry points beside the
unchanged size queries, the yardstick of the mixed-session GPU tests (in the fp64 oracle a forward and a reverse flow step of the same
frame leave the same recurrent state), and the refusals of observe()'s arguments before anything touches a device."""
import os
import re
from argparse import Namespace

import pytest
import torch

import host_dispatch_expected as E
from helpers import Fixture
from lets_face_it_amd import _lib
from oracle import seqglow_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(text, name):
    m = re.search(r"\b(?:int|long)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split())


def test_score_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    sampler = _declaration(text, "lfi_flow_sample_seq_nll")
    new = _declaration(text, "lfi_flow_score_seq_from")
    # lfi_flow_sample_seq_nll's order without `noise`; score_work, z, nll where it has nll, nll_work
    assert new == sampler.replace("const float* noise, ", "").replace("float* nll, float* nll_work, ", "float* score_work, float* z, float* nll, ")
    assert _declaration(text, "lfi_flow_score_work_floats") == "const lfi_flow_dims* d"
    for name in ("lfi_flow_score_seq_from", "lfi_flow_score_work_floats"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    vp = _lib.C.c_void_p
    nll_args = L.lfi_flow_sample_seq_nll.argtypes
    assert L.lfi_flow_score_seq_from.argtypes == nll_args[:7] + nll_args[8:-3] + [vp] * 4
    assert L.lfi_flow_score_work_floats.argtypes == L.lfi_flow_sample_nll_work_floats.argtypes


def test_score_null_arguments_are_an_argument_error_and_the_pinned_size_queries_are_unchanged():
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    rows = {name: E.EXPECTED[0]["flow"][i] for i, (name, _) in enumerate(E.FLOW_DIMS)}
    for name in ("headline gemm_precision 0x0", "headline gemm_precision 0x5", "headline gemm_precision 0x9"):
        d = _lib.FlowDims(*by_name[name])
        ref = _lib.C.byref(d)
        assert L.lfi_flow_score_work_floats(ref) > 0
        # every pointer null: an argument error, reported before any launch
        assert L.lfi_flow_score_seq_from(ref, None, None, None, 0, 0, None, None, 0, 0, 0, 0, None, None, None, None, None, None, None,
                                         None, None) == -1
        p = _lib.FlowParams()
        assert L.lfi_flow_score_seq_from(ref, _lib.C.byref(p), None, None, 0, 0, None, None, 1, 0, 1, 0, None, None, None, None, None,
                                         None, None, None, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        got = [L.lfi_flow_prep_floats(ref), L.lfi_flow_sample_work_floats(ref), L.lfi_flow_sample_nll_work_floats(ref)]
        want = [rows[name][E.FLOW_QUERIES.index(q)] for q in ("prep_floats", "sample_work_floats", "sample_nll_work_floats")]
        assert got == want, (name, got, want)
    assert L.lfi_flow_score_work_floats(None) == 0


@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_oracle_forward_and_reverse_steps_leave_the_same_recurrent_state(name):
    """The yardstick of the mixed-session tests: flow_forward on frame x and flow_reverse on the z that yields x carry the same h / c in
    every flow step (the recurrent cell's input is the pass-through half and the conditioning, identical in both directions)."""
    fx = Fixture(name)
    hp, sd = fx.hp, fx.state_dict()
    C = sd["glow.flow.layers.0.actnorm.bias"].numel()
    width = sd["glow.flow.layers.0.f.cond_transform.0.weight"].shape[1]
    B = 5
    gen = torch.Generator().manual_seed(7)
    state_f, state_r = oracle._new_state(hp), oracle._new_state(hp)
    worst = 0.0
    for n in range(4):
        x = torch.randn(B, C, dtype=torch.float64, generator=gen)
        cond = torch.randn(B, width, dtype=torch.float64, generator=gen)
        z, _, _ = oracle.flow_forward(hp, sd, x, cond, state_f)
        x2, _ = oracle.flow_reverse(hp, sd, z, cond, state_r)
        assert float((x2 - x).abs().max()) < 1e-9
        for sf, sr in zip(state_f, state_r):
            for a, b in zip(sf, sr):
                assert (a is None) == (b is None)
                if a is not None:
                    worst = max(worst, float((a - b).abs().max()))
    assert state_f[0][0] is not None and (state_f[0][1] is not None) == (hp["Glow"]["rnn_type"] == "lstm")
    print("%s: oracle forward vs reverse recurrent state over 4 frames: max abs diff %.2e" % (name, worst))
    assert worst < 1e-10


def _stub_session(B=3, C=16):
    """A SampleStream with just what observe() looks at before its first launch (no engine behind it)."""
    from lets_face_it_amd.stream import SampleStream
    st = SampleStream.__new__(SampleStream)
    st.eng = Namespace(spec=Namespace(C=C), param_version=0)
    st.closed, st.param_version, st._bound = False, 0, None
    st.B, st.mods, st.device = B, [], torch.device("cuda", 0)
    return st


def test_observe_refuses_bad_arguments_before_touching_a_device():
    st = _stub_session()
    face = torch.zeros(3, 16)
    with pytest.raises(ValueError, match=r"face: expected contiguous float32 GPU tensor \(B=3, 16\)"):
        st.observe({}, face)                                      # a CPU tensor
    with pytest.raises(ValueError, match=r"face: expected contiguous float32 GPU tensor \(B=3, 16\).*\(3, 15\)"):
        st.observe({}, torch.zeros(3, 15))                        # a wrong shape
    with pytest.raises(ValueError, match="face"):
        st.observe({}, None)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(TypeError, match="return_z"):
            st.observe({}, face, return_z=bad)
    with pytest.raises(TypeError, match="frame must be a dict"):
        st.observe(None, face)
    st.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        st.observe({}, face)
