"""CPU: the likelihood the samplers report (return_nll) without a device - the yardstick of the GPU tests (the fp64 oracle's
teacher-forced pass over the reference's generated frames recovers the noise they were made from), the C ABI's new entry point
beside the unchanged old ones, and the refusals of a non-bool return_nll before anything touches a device."""
import os
import re
from argparse import Namespace

import pytest
import torch

from helpers import FIXTURES, Fixture
from lets_face_it_amd import _lib
from sample_nll_expected import fixture_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_forward_over_generated_frames_recovers_the_noise(name):
    """The expected values of the GPU tests are the oracle's NLL of infer/out: that pass must see the z the sampler was given."""
    fx = Fixture(name)
    z, nll = fixture_expected(fx)
    noise = fx.get("infer/noise")
    assert z.dtype == torch.float64 and tuple(z.shape) == tuple(noise.shape) and tuple(nll.shape) == tuple(noise.shape[:2])
    err = float((z - noise).abs().max())
    print("%s: oracle forward over infer/out: max |z - noise| %.2e; NLL in [%.2f, %.2f] bits" % (name, err, float(nll.min()), float(nll.max())))
    assert err < 1e-10
    assert torch.isfinite(nll).all()


def _declaration(text, name):
    m = re.search(r"\b(?:int|long)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split())


def test_nll_entry_points_are_declared_and_bound_and_the_old_one_is_unchanged():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    old = _declaration(text, "lfi_flow_sample_seq_from")
    assert old == ("const lfi_flow_dims* d, const lfi_flow_params* p, const float* prep, const float* wct, long E, int hist1, "
                   "float* pre_static, const float* noise, float* faces, int seq_len, int start, int nframes, int first_frame, "
                   "float* h, float* cstate, const lfi_p1enc* p1, float* p1work, float* work, void* stream")
    new = _declaration(text, "lfi_flow_sample_seq_nll")
    assert new == old[:-len("void* stream")] + "float* nll, float* nll_work, void* stream"
    assert _declaration(text, "lfi_flow_sample_nll_work_floats") == "const lfi_flow_dims* d"
    for name in ("lfi_flow_sample_seq_nll", "lfi_flow_sample_nll_work_floats"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    assert L.lfi_flow_sample_seq_nll.argtypes == L.lfi_flow_sample_seq_from.argtypes[:-1] + [_lib.C.c_void_p] * 3
    d = _lib.FlowDims(37, 1, 50, 128, 512, 16, 1, 0, 1e-4, 0)
    assert L.lfi_flow_sample_nll_work_floats(_lib.C.byref(d)) >= 2 * 37
    # null arguments are an argument error, reported before any launch
    assert L.lfi_flow_sample_seq_nll(_lib.C.byref(d), None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, None, None, None, None,
                                     None, None, None, None) == -1


def test_a_non_bool_return_nll_is_refused_before_any_device_work():
    from lets_face_it_amd.glow.models import SeqGlow
    from lets_face_it_amd.stream import SampleStream
    fx = Fixture("tiny")
    m = SeqGlow(Namespace(**fx.hp))
    data = {k: v.float().contiguous() for k, v in fx.group("infer/data/").items()}     # CPU tensors: a bool flag gets to "GPU only"
    seq_len = int(fx.get("infer/seq_len"))
    seed = {k: v[:, :fx.start].contiguous() for k, v in data.items()}
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(TypeError, match="return_nll"):
            m.inference(seq_len, data, return_nll=bad)
        with pytest.raises(TypeError, match="return_nll"):
            m.open_stream(seed, return_nll=bad)
        with pytest.raises(TypeError, match="return_nll"):
            SampleStream(None, seed, None, return_nll=bad)      # what step() returns is fixed where the session is made
    for ok in (True, False):
        with pytest.raises(RuntimeError, match="GPU only"):
            m.inference(seq_len, data, return_nll=ok)
        with pytest.raises(RuntimeError, match="GPU only"):
            m.open_stream(seed, return_nll=ok)
    assert m.engine is None
