"""CPU: the streaming sampling surface without a device - the C entry point's argument checks (no launch), the model API's
refusals, and the engine's parameter version."""
import ctypes
from argparse import Namespace

import pytest
import torch

from helpers import Fixture
from lets_face_it_amd import _lib


def _advance(B=2, count=1, hist=3, dim=4, noise=True, C=4):
    L = _lib.lib()
    n = max(count, 1)
    win, src = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    hs, ds = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    for i in range(min(count, n)):
        win[i], src[i], hs[i], ds[i] = 0x1000, 0x2000, hist, dim
    nz = 0x3000 if noise else None
    return L.lfi_stream_advance(B, count, win, src, hs, ds, nz, 0x4000 if noise else None, C, None, None, None), L.lfi_last_error()


def test_stream_advance_reports_argument_errors_without_launching():
    for kwargs, text in ((dict(B=0), b"batch 0"), (dict(count=9), b"9 windows"), (dict(noise=False), b"null noise"),
                         (dict(hist=0), b"window 0: hist 0"), (dict(dim=-1), b"dim -1"), (dict(C=0), b"C = 0")):
        rc, msg = _advance(**kwargs)
        assert rc == -1 and text in msg, (kwargs, msg)


def test_stream_advance_is_bound_and_declared():
    assert "lfi_stream_advance" in _lib.EXPORTS
    assert _lib.lib().lfi_stream_advance.argtypes is not None


def test_open_stream_refuses_cpu_tensors_and_a_missing_seed():
    from lets_face_it_amd.glow.models import SeqGlow
    fx = Fixture("tiny")
    m = SeqGlow(Namespace(**fx.hp))
    seed = {k: v[:, :fx.start].float().contiguous() for k, v in fx.group("infer/data/").items()}
    with pytest.raises(RuntimeError, match="GPU only"):
        m.open_stream(seed)
    with pytest.raises(KeyError, match="p1_face"):
        m.open_stream({k: v for k, v in seed.items() if k != "p1_face"})
    with pytest.raises(KeyError, match="p1_face"):
        m.open_stream(None)


def test_parameter_loads_move_the_engine_parameter_version():
    """A bound module's load_state_dict bumps its engine's parameter version (what an open SampleStream checks); an unbound one
    has nothing to bump."""
    from lets_face_it_amd import engine
    from lets_face_it_amd.glow.models import SeqGlow
    fx = Fixture("tiny")
    m = SeqGlow(Namespace(**fx.hp))
    m.load_state_dict(fx.state_dict(torch.float32))      # no engine yet
    eng = object.__new__(engine.GlowEngine)
    eng.param_version = 0
    m.engine = eng
    try:
        m.load_state_dict(fx.state_dict(torch.float32))
        assert eng.param_version == 1
        eng.bump_param_version()
        assert eng.param_version == 2
    finally:
        m.engine = None
