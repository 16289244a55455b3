"""CPU: N candidate rollouts over a chunk of streaming sessions (SampleStream.rollout_candidates / commit / discard / rollout_best_of)
without a device - the C ABI's new entry points beside the unchanged size queries, the register budget of the fused front end's parent
mode, and the refusals of the new calls' arguments and the pending rule before anything touches a device."""
import os
import re
import subprocess
import sys
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


def test_rollout_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    sampler = _declaration(text, "lfi_flow_sample_seq_nll")
    # lfi_flow_sample_seq_nll's list, then the candidates' count in front of the stream
    assert _declaration(text, "lfi_flow_sample_cand_seq") == sampler.replace("void* stream", "int ncand, void* stream")
    assert _declaration(text, "lfi_flow_sample_cand_seq_work_floats") == _declaration(text, "lfi_flow_sample_cand_work_floats")
    assert _declaration(text, "lfi_stream_cand_seq_in") == (
        "int B, int ncand, int n, int start, int C, int Ks, int H, const float* parent_seq, float* cand_seq, const float* h, "
        "const float* cstate, float* cand_h, float* cand_c, int first_frame, const float* noise, unsigned* guard_bits, void* stream")
    # lfi_stream_commit_cand's list with the rollout's frames: n and start behind ncand, the candidates' sequences where that has
    # their frames, the frame counter in front of the outputs
    one = _declaration(text, "lfi_stream_commit_cand")
    want = one.replace("int ncand, int C", "int ncand, int n, int start, int C").replace("cand_frames", "cand_seq") \
              .replace("float* out_frame", "float* frame_nb, float* out")
    assert _declaration(text, "lfi_stream_commit_cand_seq") == want
    names = ("lfi_flow_sample_cand_seq", "lfi_flow_sample_cand_seq_work_floats", "lfi_stream_cand_seq_in", "lfi_stream_commit_cand_seq")
    for name in names:
        assert name in _lib.EXPORTS
    L = _lib.lib()
    vp, i = _lib.C.c_void_p, _lib.C.c_int
    nll_args = L.lfi_flow_sample_seq_nll.argtypes
    assert L.lfi_flow_sample_cand_seq.argtypes == nll_args[:-1] + [i] + nll_args[-1:]
    assert L.lfi_flow_sample_cand_seq_work_floats.argtypes == L.lfi_flow_sample_cand_work_floats.argtypes
    assert L.lfi_flow_sample_cand_seq_work_floats.restype == _lib.C.c_long
    assert L.lfi_stream_cand_seq_in.argtypes == [i] * 7 + [vp] * 6 + [i] + [vp] * 3
    assert L.lfi_stream_commit_cand_seq.argtypes == [i] * 7 + [vp] * 6 + [i] + [vp] * 8


def test_rollout_null_arguments_are_an_argument_error_and_the_pinned_size_queries_are_unchanged():
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    rows = {name: E.EXPECTED[0]["flow"][i] for i, (name, _) in enumerate(E.FLOW_DIMS)}
    for name in HEADLINE:
        d = _lib.FlowDims(*by_name[name])
        ref = _lib.C.byref(d)
        # every pointer null: an argument error, reported before any launch
        assert L.lfi_flow_sample_cand_seq(None, None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, None, None, None, None, None, None,
                                          None, 0, None) == -1
        assert L.lfi_flow_sample_cand_seq(ref, None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, None, None, None, None, None, None,
                                          None, 4, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        p = _lib.FlowParams()
        # partly null: dims and params there, two frames and four candidates asked for, every buffer missing
        assert L.lfi_flow_sample_cand_seq(ref, _lib.C.byref(p), None, None, 0, 0, None, None, None, 2, 0, 2, 0, None, None, None, None,
                                          None, None, None, 4, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        # no candidates
        assert L.lfi_flow_sample_cand_seq(ref, _lib.C.byref(p), None, None, 0, 0, None, None, None, 2, 0, 2, 0, None, None, None, None,
                                          None, None, None, 0, None) == -1
        assert b"candidates" in L.lfi_last_error()
        got = [L.lfi_flow_prep_floats(ref), L.lfi_flow_sample_work_floats(ref), L.lfi_flow_sample_nll_work_floats(ref),
               L.lfi_flow_sample_cand_work_floats(ref, 8)]
        want = [rows[name][E.FLOW_QUERIES.index(q)] for q in ("prep_floats", "sample_work_floats", "sample_nll_work_floats")]
        assert got[:3] == want, (name, got, want)
        # the rollout work area: the sampler's for the virtual rows and one frame of their pre-activations; growing with the candidates
        sizes = [L.lfi_flow_sample_cand_seq_work_floats(ref, n) for n in (1, 2, 3, 8, 17, 256)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] >= want[1] + d.B * d.Ks * d.D
        v8 = _lib.FlowDims(*by_name[name])
        v8.B = 8 * d.B
        assert sizes[3] >= L.lfi_flow_sample_work_floats(_lib.C.byref(v8)) + 8 * d.B * d.Ks * d.D
        assert L.lfi_flow_sample_cand_seq_work_floats(ref, 0) == 0 and L.lfi_flow_sample_cand_seq_work_floats(ref, -3) == 0
        assert L.lfi_flow_sample_cand_seq_work_floats(ref, (1 << 22) // d.B + 1) == 0       # beyond the virtual rows of one call
    assert L.lfi_flow_sample_cand_seq_work_floats(None, 4) == 0
    # the two window launches: all null, and sizes without buffers
    assert L.lfi_stream_cand_seq_in(0, 0, 0, 0, 0, 0, 0, None, None, None, None, None, None, 0, None, None, None) == -1
    assert L.lfi_stream_cand_seq_in(5, 3, 2, 4, 6, 2, 7, None, None, None, None, None, None, 1, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_commit_cand_seq(0, 0, 0, 0, 0, 0, 0, None, None, None, None, None, None, 0, None, None, None, None, None, None,
                                        None, None) == -1
    assert L.lfi_stream_commit_cand_seq(5, 3, 2, 4, 6, 2, 7, None, None, None, None, None, None, 2, None, None, None, None, None, None,
                                        None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    # a faces window longer than the candidates' sequences
    assert L.lfi_stream_commit_cand_seq(5, 3, 2, 4, 6, 2, 7, None, None, None, None, None, None, 7, None, None, None, None, None, None,
                                        None, None) == -1
    assert b"hist = 7" in L.lfi_last_error()


def test_the_parent_mode_of_the_fused_front_end_stays_inside_the_register_file():
    """sc_cond_kernel keeps one workgroup of 512 threads per CU: 256 VGPRs a lane. Its parent instantiations (the row index of the one
    pre_static load divided by ncand) must not cost more than the instantiations they stand beside - no spills in the form that
    runs by default, no more than its twin in the in-register-split form. tools/kernel_resources.py compiles the unit for gfx950;
    no device is needed."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "lets_face_it_amd", "csrc", "lfi_sample.hip"), "sc_cond_kernel"],
                         capture_output=True, text=True, check=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.search(r"sc_cond_kernel<(\d), (true|false), (\d), (true|false)>\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+spill\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            seen[(int(m.group(1)), m.group(2) == "true", int(m.group(3)), m.group(4) == "true")] = tuple(int(v) for v in m.groups()[4:])
    assert len(seen) == 9, out
    for ngt in (3, 4):
        vgpr, agpr, spill, scratch = seen[(ngt, True, 4, True)]
        assert spill == 0 and scratch == 0 and vgpr + agpr <= 256, (ngt, seen)
        assert seen[(ngt, False, 4, True)][2] <= seen[(ngt, False, 4, False)][2], (ngt, seen)


class _OnGpu(torch.Tensor):
    """A host tensor that says it lives on cuda:0: what the argument checks look at, with no device behind it."""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 0))


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


def _stub_session(B=3, C=16):
    """A SampleStream with just what the rollout calls look at before their first launch (no engine behind it)."""
    from lets_face_it_amd.stream import SampleStream
    st = SampleStream.__new__(SampleStream)
    st.eng = Namespace(spec=Namespace(C=C, rnn_type="gru", H=32, Ks=4, D=64, ldf=128), param_version=0)
    st.closed, st.param_version, st._bound = False, 0, None
    st.B, st.device = B, torch.device("cuda", 0)
    st.mods = [Namespace(name="p1_speech", in_dim=5)]
    return st


def test_rollout_candidates_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    st = _stub_session()
    ok = {"p1_speech": _gpu(3, 4, 5)}
    for call in (st.rollout_candidates, st.rollout_best_of):
        for bad in (2.0, "4", None, True, torch.tensor(4)):
            with pytest.raises(TypeError, match="ncand: expected an int"):
                call(ok, bad)
        for bad in (0, -1, 257):
            with pytest.raises(ValueError, match=r"ncand: -?\d+ outside 1 \.\. 256"):
                call(ok, bad)
        with pytest.raises(TypeError, match="frames must be a dict"):
            call(None, 4)
        with pytest.raises(KeyError, match="p1_speech"):
            call({}, 4)
        with pytest.raises(ValueError, match=r"p1_speech: expected contiguous float32 GPU tensor \(B=3, n>=1, 5\)"):
            call({"p1_speech": torch.zeros(3, 4, 5)}, 4)                      # a CPU tensor
        # the noise: (n, B, ncand, C) contiguous float32 on the session's device, n the frames'
        for bad in (torch.zeros(4, 3, 4, 16), _gpu(4, 3, 16), _gpu(3, 4, 4, 16), _gpu(4, 3, 5, 16), _gpu(4, 3, 4, 15), _gpu(5, 3, 4, 16),
                    _gpu(4, 3, 4, 16, dtype=torch.float64), [0.0], 1.0):
            with pytest.raises(ValueError, match=r"noise: expected contiguous float32 GPU tensor \(n=4, B=3, ncand=4, 16\)"):
                call(ok, 4, bad)
    # one round only: the frames one round takes for B * ncand virtual rows, which LFI_OBSERVE_CHUNK_FRAMES caps too
    monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "3")
    with pytest.raises(ValueError, match=r"frames: 4 frames of 5 candidates for each of 3 rows are more than the one round a rollout is "
                                         r"\(at most 3 frames\)"):
        st.rollout_candidates(ok, 5, _gpu(4, 3, 5, 16))
    monkeypatch.delenv("LFI_OBSERVE_CHUNK_FRAMES")
    caps = [st._rollout_cap(n) for n in (1, 2, 16, 256)]
    assert caps[0] == st._chunk_cap() and all(a >= b for a, b in zip(caps, caps[1:])) and caps[-1] >= 8, caps
    # a model without conditioning windows takes its frame count from the noise
    st.mods = []
    with pytest.raises(ValueError, match=r"noise: a model without conditioning windows .* \(n, B=3, ncand=4, 16\)"):
        st.rollout_candidates({}, 4)
    # more virtual rows than one call takes
    st.B = 40000
    with pytest.raises(ValueError, match=r"ncand: 256 candidates for each of 40000 rows are 10240000 virtual rows, .* \(at most 4194304\)"):
        st.rollout_candidates({}, 256, _gpu(1, 40000, 256, 16))
    st.B = 3
    st.eng.param_version = 1
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.rollout_candidates({}, 4)
    st.eng.param_version = 0
    st.closed = True
    for call in (lambda: st.rollout_candidates({}, 4), st.discard, st.commit):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def _pending_rollouts(ncand, n):
    return Namespace(kind="rollouts", ncand=ncand, n=n)


def test_discard_wants_pending_rollouts_and_commit_checks_their_choice():
    st = _stub_session()
    with pytest.raises(RuntimeError, match=r"discard\(\) without pending rollouts \(rollout_candidates comes first\)"):
        st.discard()
    # one-frame candidates have moved the windows already: commit() or reset()
    st._pending = 4
    with pytest.raises(RuntimeError, match=r"discard\(\) with 4 one-frame candidates per row pending \(step_candidates\).*commit\(\) one "
                                           r"of them, or reset\(\)"):
        st.discard()
    assert st._pending == 4
    st._pending = _pending_rollouts(4, 3)
    with pytest.raises(ValueError, match="choice: 2 listed for 3 rows"):
        st.commit([0, 1])
    with pytest.raises(ValueError, match=r"choice: \[4\] outside the row's candidates \(0 \.\. 3\)"):
        st.commit([0, 4, 1])
    with pytest.raises(ValueError, match="choice: expected a sequence of ints or a 1-D CPU integer tensor"):
        st.commit(torch.zeros(3))
    with pytest.raises(ValueError, match=r"choice: expected 3 entries \(B,\) of int32 / int64"):
        st.commit(_gpu(3))
    assert st._pending.ncand == 4
    st.discard()                                    # no launch: the rollouts are dropped, nothing else moves
    assert st._pending is None
    st._pending = _pending_rollouts(4, 3)
    st.eng.param_version = 1
    for call in (st.commit, st.discard):
        with pytest.raises(RuntimeError, match="parameters changed"):
            call()


def test_pending_rollouts_refuse_every_other_call_before_touching_a_device():
    st = _stub_session()
    st._pending = _pending_rollouts(5, 3)
    face, seed = torch.zeros(3, 16), {"p1_face": torch.zeros(3, 4, 16)}
    calls = (lambda: st.step({}), lambda: st.observe({}, face), lambda: st.step_rows({}, face, [True, False, True]),
             lambda: st.step_candidates({}, 5), lambda: st.step_best_of({}, 5), lambda: st.step_many({}),
             lambda: st.observe_many({}, torch.zeros(3, 2, 16)), lambda: st.step_rows_many({}, torch.zeros(3, 2, 16), [[True] * 3] * 2),
             lambda: st.rollout_candidates({}, 5), lambda: st.rollout_best_of({}, 5),
             lambda: st.save_rows([0]), lambda: st.load_rows([0], None), lambda: st.reset_rows([0], seed))
    for call in calls:
        with pytest.raises(RuntimeError, match=r"5 candidate rollouts of 3 frames per row are pending \(rollout_candidates\): commit\(\) "
                                               r"one of them, discard\(\) them, or reset\(\)"):
            call()
    assert st._pending.ncand == 5
    # pending one-frame candidates refuse the new calls in their own words, as before
    st._pending = 5
    for call in (lambda: st.rollout_candidates({}, 5), lambda: st.rollout_best_of({}, 5)):
        with pytest.raises(RuntimeError, match=r"5 candidates per row are pending \(step_candidates\): commit\(\)"):
            call()
