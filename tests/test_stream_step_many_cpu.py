"""CPU: several generated frames per call (SampleStream.step_many) without a device - the two window launches of the C ABI
(lfi_stream_chunk_gen_in / lfi_stream_chunk_gen_out): declared, exported and bound, their argument errors before any launch - and the
refusals of step_many()'s arguments before anything touches a device."""
import os

import pytest
import torch

from lets_face_it_amd import _lib
from test_stream_chunk_cpu import _declaration, _gpu, _stub_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lfi_stream_chunk_gen_in", "lfi_stream_chunk_gen_out")


def test_gen_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    L = _lib.lib()
    for name in NEW:
        _declaration(text, name)
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is _lib.C.c_int
    # the observed chunk's declarations with the generated window's arguments added
    tail_in = "unsigned* guard_bits, void* stream"
    assert _declaration(text, "lfi_stream_chunk_gen_in") == _declaration(text, "lfi_stream_chunk_in").replace(
        tail_in, "int gen_win, const float* noise , int C, " + tail_in)
    assert _declaration(text, "lfi_stream_chunk_gen_out") == _declaration(text, "lfi_stream_chunk_out").replace(
        "float* frame_nb, void* stream", "int gen_win, float* out , long ld_out, float* frame_nb, unsigned* guard_bits, void* stream")
    assert len(L.lfi_stream_chunk_gen_in.argtypes) == len(L.lfi_stream_chunk_in.argtypes) + 3
    assert len(L.lfi_stream_chunk_gen_out.argtypes) == len(L.lfi_stream_chunk_out.argtypes) + 4
    # the existing entry points keep their signatures
    assert len(L.lfi_stream_chunk_in.argtypes) == 12 and len(L.lfi_stream_chunk_out.argtypes) == 11


def _tables(dim=4, hist=4, lead=0):
    c = _lib.C
    return (c.c_void_p * 1)(0x4000), (c.c_int * 1)(hist), (c.c_int * 1)(dim), (c.c_int * 1)(lead)


def test_gen_launches_refuse_null_tables_before_any_launch():
    L = _lib.lib()
    c = _lib.C
    one_p, hist, dim, lead = _tables()
    null_p = (c.c_void_p * 1)()
    fake = c.c_void_p(0x8000)
    assert L.lfi_stream_chunk_gen_in(2, 3, 4, 1, None, None, None, None, None, None, 0, None, 4, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_gen_out(2, 3, 4, 1, None, None, None, None, None, 0, None, 12, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    # a null window / sequence inside the tables, a null source table, null noise, null out
    assert L.lfi_stream_chunk_gen_in(2, 3, 4, 1, one_p, null_p, null_p, hist, dim, lead, 0, fake, 4, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_gen_out(2, 3, 4, 1, null_p, one_p, hist, dim, lead, 0, fake, 12, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_gen_in(2, 3, 4, 1, one_p, None, one_p, hist, dim, lead, 0, fake, 4, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_gen_in(2, 3, 4, 1, one_p, null_p, one_p, hist, dim, lead, 0, None, 4, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_stream_chunk_gen_out(2, 3, 4, 1, one_p, one_p, hist, dim, lead, 0, None, 12, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    # a conditioning window (not gen_win) needs its source
    two_p, two_null = (c.c_void_p * 2)(0x4000, 0x5000), (c.c_void_p * 2)()
    two_h, two_d, two_l = (c.c_int * 2)(4, 4), (c.c_int * 2)(4, 4), (c.c_int * 2)(0, 1)
    assert L.lfi_stream_chunk_gen_in(2, 3, 4, 2, two_p, two_null, two_p, two_h, two_d, two_l, 1, fake, 4, None, None) == -1
    assert b"null pointer (source 0)" in L.lfi_last_error()


def test_gen_launches_refuse_bad_shapes_before_any_launch():
    L = _lib.lib()
    c = _lib.C
    one_p, hist, dim, lead = _tables()
    fake = c.c_void_p(0x8000)

    def gen_in(B=2, n=3, start=4, count=1, gen_win=0, C=4):
        return L.lfi_stream_chunk_gen_in(B, n, start, count, one_p, one_p, one_p, hist, dim, lead, gen_win, fake, C, None, None)

    def gen_out(B=2, n=3, start=4, count=1, gen_win=0, ld_out=12):
        return L.lfi_stream_chunk_gen_out(B, n, start, count, one_p, one_p, hist, dim, lead, gen_win, fake, ld_out, None, None, None)

    for bad in (dict(n=0), dict(B=0), dict(count=9), dict(start=3), dict(gen_win=-1), dict(gen_win=1)):
        assert gen_in(**bad) == -1, bad
        assert L.lfi_last_error(), bad
        assert gen_out(**bad) == -1, bad
    assert gen_in(C=5) == -1                          # dim[gen_win] != C
    assert b"dim 4" in L.lfi_last_error() and b"C = 5" in L.lfi_last_error()
    assert gen_in(C=0) == -1
    assert gen_out(ld_out=11) == -1                   # ld_out < n * C
    assert b"row pitch 11" in L.lfi_last_error()
    # the prev_p1_face window's leading row does not count against the history: hist - lead <= start
    p, h5, d, l1 = _tables(hist=5, lead=1)
    assert L.lfi_stream_chunk_gen_in(2, 3, 3, 1, p, p, p, h5, d, l1, 0, fake, 4, None, None) == -1
    assert L.lfi_stream_chunk_gen_out(2, 3, 3, 1, p, p, h5, d, l1, 0, fake, 12, None, None, None) == -1


def test_step_many_refuses_bad_arguments_before_touching_a_device():
    st = _stub_session()
    ok = {"p1_speech": _gpu(3, 4, 5), "p2_face": _gpu(3, 4, 16)}
    for bad in (None, [ok["p1_speech"], ok["p2_face"]], ok["p1_speech"]):
        with pytest.raises(TypeError, match="frames must be a dict"):
            st.step_many(bad)
    with pytest.raises(KeyError, match="p2_face"):
        st.step_many({"p1_speech": ok["p1_speech"]})
    with pytest.raises(ValueError, match=r"p1_speech: expected contiguous float32 GPU tensor \(B=3, n>=1, 5\).*\(3, 5\)"):
        st.step_many(dict(ok, p1_speech=_gpu(3, 5)))                          # a wrong rank: one frame is step()'s
    with pytest.raises(ValueError, match=r"p1_speech: .*\(3, 0, 5\)"):
        st.step_many(dict(ok, p1_speech=_gpu(3, 0, 5)))                       # no frames
    with pytest.raises(ValueError, match=r"p1_speech: .*float16"):
        st.step_many(dict(ok, p1_speech=_gpu(3, 4, 5, dtype=torch.float16)))
    with pytest.raises(ValueError, match=r"p1_speech: .* on cpu"):
        st.step_many(dict(ok, p1_speech=torch.zeros(3, 4, 5)))                # on another device
    with pytest.raises(ValueError, match="p2_face: expected contiguous"):
        st.step_many(dict(ok, p2_face=_gpu(3, 16, 4).transpose(1, 2)))
    with pytest.raises(ValueError, match=r"p2_face: expected contiguous float32 GPU tensor \(B=3, n=4, 16\).*\(3, 5, 16\)"):
        st.step_many(dict(ok, p2_face=_gpu(3, 5, 16)))                        # n differs between modalities
    with pytest.raises(ValueError, match=r"p1_speech: .*\(4, 4, 5\)"):
        st.step_many(dict(ok, p1_speech=_gpu(4, 4, 5)))                       # another batch
    # noise: (n, B, C) = (4, 3, 16), frame-major
    with pytest.raises(ValueError, match=r"noise: expected contiguous float32 GPU tensor \(n=4, B=3, 16\).*frame-major.*\(3, 4, 16\)"):
        st.step_many(ok, _gpu(3, 4, 16))                                      # (B, n, C): the orientation of `out`, not of the noise
    with pytest.raises(ValueError, match=r"noise: .*\(5, 3, 16\)"):
        st.step_many(ok, _gpu(5, 3, 16))                                      # another n
    with pytest.raises(ValueError, match=r"noise: .*\(4, 3, 15\)"):
        st.step_many(ok, _gpu(4, 3, 15))
    with pytest.raises(ValueError, match=r"noise: .*\(3, 16\)"):
        st.step_many(ok, _gpu(3, 16))                                         # one frame's: step()'s
    with pytest.raises(ValueError, match=r"noise: .*float64"):
        st.step_many(ok, _gpu(4, 3, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"noise: .* on cpu"):
        st.step_many(ok, torch.zeros(4, 3, 16))
    with pytest.raises(ValueError, match="noise: expected contiguous"):
        st.step_many(ok, _gpu(3, 4, 16).transpose(0, 1))                      # the right shape, strided
    with pytest.raises(ValueError, match="noise"):
        st.step_many(ok, "draw")
    st.eng.param_version = 1
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_many(ok)
    st.eng.param_version = 0
    st.closed = True
    with pytest.raises(RuntimeError, match="closed"):
        st.step_many(ok)
