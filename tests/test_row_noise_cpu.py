"""CPU: the per-row keyed sampling noise (lfi_row_noise) without a device - the numpy restatement of the generator
(tests/row_noise_reference.py) against the Random123 known-answer vectors, planted defects and moments; the two C entry points'
argument checks (no launch), their declarations and their binding; the one shared Philox definition."""
import os
import re

import numpy as np
import pytest

import row_noise_reference as R
from lets_face_it_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_philox_matches_the_random123_known_answers():
    for counter, key, want in KAT:
        got = " ".join("%08x" % int(v) for v in R.philox4x32(counter, key))
        assert got == want, (counter, key, got)
    # vectorised over counters: the three at once give the three answers
    c = [np.array([k[0][j] for k in KAT]) for j in range(4)]
    key = [np.array([k[1][j] for k in KAT]) for j in range(2)]
    out = R.philox4x32(c, key)
    for i, (_, _, want) in enumerate(KAT):
        assert " ".join("%08x" % int(v[i]) for v in out) == want


def test_the_generator_is_the_definition_spelled_out_for_one_element():
    """Key K, position p, candidate k, channel c by hand: counter (c >> 2, lo32(p), hi32(p), k), key (lo32(K), hi32(K)), channel c
    takes g[c & 3]."""
    K, p, k, c, eps = (7 << 32) + 11, (3 << 32) + 0xfffffffe, 2, 6, 0.8
    o = [int(v) for v in R.philox4x32((c >> 2, p & 0xffffffff, p >> 32, k), (K & 0xffffffff, K >> 32))]
    u = [(v >> 9) * 2.0 ** -23 + 2.0 ** -24 for v in o]
    assert all(0.0 < v < 1.0 and float(np.float32(v)) == v for v in u)        # exact in fp32, never 0 or 1
    want = float(np.float32(eps)) * np.sqrt(-2.0 * np.log(u[2])) * np.cos(2.0 * np.pi * u[3])       # c & 3 = 2: the cosine of (u2, u3)
    z = R.row_noise([5, K], [0, p - 1], n=3, ncand=3, eps=eps, C=7)
    assert z.shape == (3, 2, 3, 7)
    assert z[1, 1, k, c] == pytest.approx(want, rel=0, abs=1e-15)
    # the position crosses the 32-bit word; ncand = 0 is one candidate, number 0
    assert np.array_equal(R.row_noise([K], [p - 1], 3, 0, eps, 7)[:, :, 0], z[:, 1:, 0])
    # a row's values do not depend on the other rows, the batch size or the row index
    assert np.array_equal(R.row_noise([K], [p - 1], 3, 3, eps, 7)[:, 0], z[:, 1])
    # frame i of a call at p is frame 0 of a call at p + i
    assert np.array_equal(R.row_noise([K], [p + 1], 1, 3, eps, 7)[0], z[2:, 1][0:1].reshape(1, 3, 7))
    assert np.abs(z).max() <= R.G_MAX * eps


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_moves_the_output(defect):
    args = dict(keys=[5 + (9 << 40), 1], pos=[(1 << 32) + 1, 7 << 33], n=2, ncand=3, eps=1.0, C=6)
    good, bad = R.row_noise(**args), R.row_noise(defect=defect, **args)
    assert good.shape == bad.shape
    assert np.abs(good - bad).max() > 1e-3, defect
    # ... in every row the defect can reach: all of them here (both keys have two non-zero, different words; both positions a high word)
    assert all(np.abs(good[:, r] - bad[:, r]).max() > 1e-3 for r in range(2)), defect


def test_moments_over_2_to_the_20_draws_of_one_key():
    """Five-sigma bounds, deterministic: the key was picked once (the first tried) so that the reference passes."""
    z = R.row_noise([20261021], [0], n=4096, ncand=0, eps=1.0, C=256).reshape(-1)
    N = z.size
    assert N == 1 << 20
    mean, var = float(z.mean()), float(z.var())
    assert abs(mean) <= 5.0 / np.sqrt(N), mean
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N), var
    assert np.abs(z).max() <= R.G_MAX


def test_the_error_bound_is_a_few_fp32_ulps_and_follows_eps():
    b = R.row_noise_bound([3, 4], [0, 1 << 40], n=2, ncand=2, eps=1.0, C=9)
    z = R.row_noise([3, 4], [0, 1 << 40], n=2, ncand=2, eps=1.0, C=9)
    assert b.shape == z.shape == (2, 2, 2, 9)
    assert (b > 0).all() and (b <= 16 * 2.0 ** -23 * np.maximum(np.abs(z), 1e-3) + 1e-12).all()
    assert np.allclose(R.row_noise_bound([3, 4], [0, 1 << 40], 2, 2, 0.5, 9), 0.5 * b, rtol=0.2, atol=0)


# ---- the library
def _declaration(text, name):
    m = re.search(r"\b(?:int|long)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split())


def test_row_noise_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    assert _declaration(text, "lfi_row_noise") == (
        "unsigned long long* rng , int B, int n, int ncand, int C, float eps, float* out, long stride_frame, long stride_row, "
        "long stride_cand, int advance, void* stream")
    assert _declaration(text, "lfi_row_rng_advance") == "unsigned long long* rng, int B, long delta, const int* lens , void* stream"
    L = _lib.lib()
    vp, i, l, f = _lib.C.c_void_p, _lib.C.c_int, _lib.C.c_long, _lib.C.c_float
    for name in ("lfi_row_noise", "lfi_row_rng_advance"):
        assert name in _lib.EXPORTS
    assert L.lfi_row_noise.argtypes == [vp, i, i, i, i, f, vp, l, l, l, i, vp]
    assert L.lfi_row_rng_advance.argtypes == [vp, i, l, vp, vp]
    # the one Philox definition lives in the shared header, and the Makefile knows both units depend on it
    csrc = os.path.join(ROOT, "lets_face_it_amd", "csrc")
    for unit in ("lfi_data.hip", "lfi_noise.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "lfi_philox.h"' in src and "0xD2511F53" not in src, unit
    assert open(os.path.join(csrc, "lfi_philox.h")).read().count("void philox4x32_10(") == 1
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"lfi_data\.o.*lfi_noise\.o.*:.*lfi_philox\.h", mk) and "lfi_noise.hip" in mk
    assert "-ffast-math" not in mk and "fast-math" not in open(os.path.join(csrc, "lfi_noise.hip")).read().replace("no fast-math", "")


def test_row_noise_reports_argument_errors_without_a_device():
    L = _lib.lib()
    rng, out = 0x10000, 0x20000

    def noise(rng=rng, B=2, n=1, ncand=0, C=4, out=out, sf=8, sr=4, sc=0, advance=0):
        return L.lfi_row_noise(rng, B, n, ncand, C, 1.0, out, sf, sr, sc, advance, None), L.lfi_last_error()

    for kwargs, text in ((dict(rng=None), b"null"), (dict(out=None), b"null"), (dict(rng=None, n=0, advance=2), b"null"),
                         (dict(B=-1), b"negative"), (dict(n=-1), b"negative"), (dict(ncand=-1), b"negative"), (dict(C=-3), b"negative"),
                         (dict(advance=-1), b"negative"), (dict(sf=-1), b"negative stride"), (dict(sr=-4), b"negative stride"),
                         (dict(sc=-4), b"negative stride"), (dict(ncand=257), b"257 candidates"), (dict(rng=rng + 4), b"misaligned"),
                         (dict(out=out + 2), b"not a float address")):
        rc, msg = noise(**kwargs)
        assert rc == -1 and b"lfi_row_noise" in msg and text in msg, (kwargs, msg)
    # nothing to do is not an error, and launches nothing: no rows; no frames and no advance
    assert noise(rng=None, out=None, B=0)[0] == 0
    assert noise(rng=None, out=None, n=0, advance=0)[0] == 0

    def advance(rng=rng, B=2, delta=1, lens=None):
        return L.lfi_row_rng_advance(rng, B, delta, lens, None), L.lfi_last_error()

    for kwargs, text in ((dict(rng=None), b"null"), (dict(rng=None, delta=0, lens=0x3000), b"null"), (dict(B=-2), b"negative"),
                         (dict(delta=-1), b"negative"), (dict(rng=rng + 4), b"misaligned")):
        rc, msg = advance(**kwargs)
        assert rc == -1 and b"lfi_row_rng_advance" in msg and text in msg, (kwargs, msg)
    assert advance(rng=None, B=0)[0] == 0 and advance(rng=None, delta=0)[0] == 0
