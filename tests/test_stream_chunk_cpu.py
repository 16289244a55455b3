"""CPU: a chunk of recorded frames per call (SampleStream.observe_many) without a device - the C ABI's new entry points (the chunk chain
with its two size queries, the two window launches) beside the unchanged pinned size queries, their argument errors before any launch,
and the refusals of observe_many()'s arguments before anything touches a device."""
import os
import re
from argparse import Namespace

import pytest
import torch

import host_dispatch_expected as E
from lets_face_it_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lfi_flow_score_seq_chunk", "lfi_flow_score_chunk_work_floats", "lfi_flow_score_chunk_ok", "lfi_stream_chunk_in",
       "lfi_stream_chunk_out")


def _declaration(text, name):
    m = re.search(r"\b(?:int|long)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split())


def test_chunk_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    L = _lib.lib()
    for name in NEW:
        _declaration(text, name)
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    # lfi_flow_score_seq_from's declaration with the work area's name swapped
    per_frame = _declaration(text, "lfi_flow_score_seq_from")
    assert "float* score_work" in per_frame
    assert _declaration(text, "lfi_flow_score_seq_chunk") == per_frame.replace("float* score_work", "float* chunk_work")
    assert L.lfi_flow_score_seq_chunk.argtypes == L.lfi_flow_score_seq_from.argtypes
    assert _declaration(text, "lfi_flow_score_chunk_work_floats") == "const lfi_flow_dims* d, const lfi_p1enc* p1, int hist1"
    assert _declaration(text, "lfi_flow_score_chunk_ok") == "const lfi_flow_dims* d"


def test_chunk_null_arguments_are_an_argument_error_and_the_pinned_size_queries_are_unchanged():
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    rows = {name: E.EXPECTED[0]["flow"][i] for i, (name, _) in enumerate(E.FLOW_DIMS)}
    for name in ("headline gemm_precision 0x0", "headline gemm_precision 0x5", "headline gemm_precision 0x9"):
        d = _lib.FlowDims(*by_name[name])
        ref = _lib.C.byref(d)
        # every pointer null: an argument error, reported before any launch
        assert L.lfi_flow_score_seq_chunk(ref, None, None, None, 0, 0, None, None, 0, 0, 0, 0, None, None, None, None, None, None, None,
                                          None, None) == -1
        p = _lib.FlowParams()
        assert L.lfi_flow_score_seq_chunk(ref, _lib.C.byref(p), None, None, 0, 1, None, None, 2, 1, 1, 0, None, None, None, None, None,
                                          None, None, None, None) == -1
        assert b"null pointer" in L.lfi_last_error()
        got = [L.lfi_flow_prep_floats(ref), L.lfi_flow_sample_work_floats(ref), L.lfi_flow_sample_nll_work_floats(ref)]
        want = [rows[name][E.FLOW_QUERIES.index(q)] for q in ("prep_floats", "sample_work_floats", "sample_nll_work_floats")]
        assert got == want, (name, got, want)


def test_chunk_work_size_is_positive_and_grows_with_the_frames():
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    args = list(by_name["headline gemm_precision 0x9"])
    for kind, hid in ((0, 0), (1, 24), (2, 24), (3, 24)):
        p1 = _lib.P1Enc()
        p1.kind, p1.hid = kind, hid
        last = 0
        for n in (1, 2, 3, 16, 64, 250):
            d = _lib.FlowDims(*args)
            d.N = n
            w = L.lfi_flow_score_chunk_work_floats(_lib.C.byref(d), _lib.C.byref(p1), 8)
            assert w > 0 and w >= last, (kind, n, w, last)
            last = w
    d = _lib.FlowDims(*args)
    assert L.lfi_flow_score_chunk_work_floats(None, None, 8) == 0
    assert L.lfi_flow_score_chunk_ok(None) == 0
    assert L.lfi_flow_score_chunk_work_floats(_lib.C.byref(d), None, 8) > 0      # (no p1 descriptor: a raw window)


def test_window_launches_refuse_null_tables_before_any_launch():
    L = _lib.lib()
    c = _lib.C
    one_p, one_i = (c.c_void_p * 1)(0x4000), (c.c_int * 1)(4)
    zero_i = (c.c_int * 1)(0)
    assert L.lfi_stream_chunk_in(2, 3, 4, 1, None, None, None, None, None, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_out(2, 3, 4, 1, None, None, None, None, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    null_p = (c.c_void_p * 1)()
    assert L.lfi_stream_chunk_in(2, 3, 4, 1, one_p, null_p, one_p, one_i, one_i, zero_i, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_out(2, 3, 4, 1, one_p, null_p, one_i, one_i, zero_i, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    for bad in ((2, 0, 4, 1), (0, 3, 4, 1), (2, 3, 4, 9), (2, 3, 3, 1)):        # no frames, no batch, too many windows, hist > start
        assert L.lfi_stream_chunk_in(*bad, one_p, one_p, one_p, one_i, one_i, zero_i, None, None) == -1, bad
        assert L.lfi_stream_chunk_out(*bad, one_p, one_p, one_i, one_i, zero_i, None, None) == -1, bad


def test_chunk_ok_follows_the_shape_and_the_two_switches(monkeypatch):
    """1 for the register-resident cells' shapes (final_model's among them), 0 beyond them and under either switch: there the session
    falls back to lfi_flow_score_seq_from."""
    L = _lib.lib()
    by_name = dict(E.FLOW_DIMS)
    for key in ("LFI_SAMPLE_CHAIN", "LFI_FLOW_GENERIC"):
        monkeypatch.delenv(key, raising=False)
    fields = [f[0] for f in _lib.FlowDims._fields_]
    for name in ("headline gemm_precision 0x0", "headline gemm_precision 0x5", "headline gemm_precision 0x9"):
        d = _lib.FlowDims(*by_name[name])
        ref = _lib.C.byref(d)
        assert L.lfi_flow_score_chunk_ok(ref) == 1, name
        for key, value in (("LFI_SAMPLE_CHAIN", "0"), ("LFI_FLOW_GENERIC", "1")):
            with monkeypatch.context() as mp:
                mp.setenv(key, value)
                assert L.lfi_flow_score_chunk_ok(ref) == 0, (name, key)
        assert L.lfi_flow_score_chunk_ok(ref) == 1
        for field, value in (("C", 130), ("H", 144)):
            assert field in fields
            wide = _lib.FlowDims(*by_name[name])
            setattr(wide, field, value)
            assert L.lfi_flow_score_chunk_ok(_lib.C.byref(wide)) == 0, (name, field)


def test_the_sequence_chain_kernels_stay_out_of_scratch():
    """The frame loop of flow_fwd_seq_chain_kernel stays inside the register file only because two empty asm statements keep the
    compiler from hoisting per-frame loads and addresses out of it (lfi_flow_cells.h): a toolchain that finds another way to spill
    shows here, not as a slower chain. tools/kernel_resources.py compiles the unit for gfx950; no device is needed."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "lets_face_it_amd", "csrc", "lfi_flow_chunk.hip"), "flow_fwd_seq_chain_kernel"],
                         capture_output=True, text=True, check=True).stdout
    rows = [line for line in out.splitlines() if "flow_fwd_seq_chain_kernel" in line]
    assert len(rows) == 3, out
    for line in rows:
        m = re.search(r"vgpr\s+(\d+)\s+agpr\s+(\d+)\s+spill\s+(\d+)\s+scratch\s+(\d+)", line)
        assert m, line
        vgpr, agpr, spill, scratch = (int(v) for v in m.groups())
        assert spill == 0 and scratch == 0 and vgpr + agpr <= 256, line


class _OnGpu(torch.Tensor):
    """A host tensor that says it lives on cuda:0: what the argument checks look at, with no device behind it."""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 0))


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


def _stub_session(B=3, C=16):
    """A SampleStream with just what observe_many() looks at before its first launch (no engine behind it)."""
    from lets_face_it_amd.stream import SampleStream
    st = SampleStream.__new__(SampleStream)
    st.eng = Namespace(spec=Namespace(C=C), param_version=0)
    st.closed, st.param_version, st._bound = False, 0, None
    st.B, st.device = B, torch.device("cuda", 0)
    st.mods = [Namespace(name="p1_speech", in_dim=5), Namespace(name="p2_face", in_dim=16)]
    return st


def test_observe_many_refuses_bad_arguments_before_touching_a_device():
    st = _stub_session()
    ok = {"p1_speech": _gpu(3, 4, 5), "p2_face": _gpu(3, 4, 16)}
    faces = _gpu(3, 4, 16)
    with pytest.raises(ValueError, match=r"faces: expected contiguous float32 GPU tensor \(B=3, n>=1, 16\)"):
        st.observe_many(ok, torch.zeros(3, 4, 16))                            # a CPU tensor
    with pytest.raises(ValueError, match=r"faces: expected contiguous float32 GPU tensor \(B=3, n>=1, 16\).*\(3, 16\)"):
        st.observe_many(ok, _gpu(3, 16))                                      # a wrong rank: one frame is observe()'s
    with pytest.raises(ValueError, match=r"faces: .*\(3, 0, 16\)"):
        st.observe_many(ok, _gpu(3, 0, 16))                                   # no frames
    with pytest.raises(ValueError, match=r"faces: .*float64"):
        st.observe_many(ok, _gpu(3, 4, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="faces"):
        st.observe_many(ok, None)
    with pytest.raises(ValueError, match=r"p2_face: expected contiguous float32 GPU tensor \(B=3, n=4, 16\).*\(3, 5, 16\)"):
        st.observe_many(dict(ok, p2_face=_gpu(3, 5, 16)), faces)              # a wrong n in one modality
    with pytest.raises(ValueError, match=r"p1_speech: expected contiguous float32 GPU tensor \(B=3, n=4, 5\).*\(3, 4, 6\)"):
        st.observe_many(dict(ok, p1_speech=_gpu(3, 4, 6)), faces)
    with pytest.raises(ValueError, match=r"p1_speech: .*float16"):
        st.observe_many(dict(ok, p1_speech=_gpu(3, 4, 5, dtype=torch.float16)), faces)
    with pytest.raises(ValueError, match=r"p1_speech: .* on cpu"):
        st.observe_many(dict(ok, p1_speech=torch.zeros(3, 4, 5)), faces)      # on another device
    with pytest.raises(ValueError, match="p2_face: expected contiguous"):
        st.observe_many(dict(ok, p2_face=_gpu(3, 16, 4).transpose(1, 2)), faces)
    with pytest.raises(KeyError, match="p2_face"):
        st.observe_many({"p1_speech": ok["p1_speech"]}, faces)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(TypeError, match="return_z"):
            st.observe_many(ok, faces, return_z=bad)
    with pytest.raises(TypeError, match="frames must be a dict"):
        st.observe_many(None, faces)
    st.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        st.observe_many(ok, faces)
