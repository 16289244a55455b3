"""GPU: the keyed sampling-noise kernel (lfi_row_noise / lfi_row_rng_advance, csrc/lfi_noise.hip) through the C ABI against the numpy
restatement of the generator (tests/row_noise_reference.py): every element inside the reference's own error bound, in the four
dense layouts (B, C), (B, ncand, C), (n, B, C), (n, B, ncand, C) and a padded one, at an unaligned address between guard bands;
the same (key, position, candidate) gives the same bits in every layout, batch size and row; the position advance rides in the
launch and is exact."""
import numpy as np
import pytest
import torch

import row_noise_reference as R
from helpers import report
from lets_face_it_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats either side of the addressed span
SENTINEL = 12345.5
KEYS = (0, 1, 1 << 32, (1 << 63) - 1)
POSITIONS = (0, (1 << 32) - 2)  # with n = 4 the second crosses the 32-bit word
EPS = 0.8


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rng(keys, pos, device):
    return torch.tensor([[k, p] for k, p in zip(keys, pos)], dtype=torch.int64, device=device).reshape(len(keys), 2)


def _strides(layout, B, K, C):
    """(stride_frame, stride_row, stride_cand) in floats: the dense layout of (n, B, K, C) - which is (B, C), (B, ncand, C), (n, B, C)
    and (n, B, ncand, C) - or one with every stride larger than dense."""
    if layout == "dense":
        return B * K * C, K * C, C
    sc = C + 3
    sr = K * sc + 5
    return B * sr + 7, sr, sc


def _launch(device, keys, pos, n, ncand, C, layout, eps=EPS, advance=0):
    """One lfi_row_noise call into a buffer that starts one float behind an allocation boundary, guard bands either side -> (values
    (n, B, K, C) float32 on the host, the rng words after the launch). Checks that nothing but the addressed elements was written."""
    B, K = len(keys), max(ncand, 1)
    sf, sr, sc = _strides(layout, B, K, C)
    span = (n - 1) * sf + (B - 1) * sr + (K - 1) * sc + C if n else 0
    buf = torch.full((1 + GUARD + span + GUARD,), SENTINEL, dtype=torch.float32, device=device)
    rng = _rng(keys, pos, device)
    out_ptr = buf.data_ptr() + 4 * (1 + GUARD)
    assert out_ptr % 16 == 4                # no alignment to lean on
    if layout == "dense" and ncand == 0:
        sc = 0                              # (B, C) and (n, B, C): no candidate axis
    _lib.check(_lib.lib().lfi_row_noise(rng.data_ptr(), B, n, ncand, C, eps, out_ptr, sf, sr, sc, advance, _stream()), "lfi_row_noise")
    host = buf.cpu().numpy()
    body = host[1 + GUARD:1 + GUARD + span]
    idx = (np.arange(n)[:, None, None, None] * sf + np.arange(B)[None, :, None, None] * sr
           + np.arange(K)[None, None, :, None] * _strides(layout, B, K, C)[2] + np.arange(C)[None, None, None, :])
    touched = np.zeros(span, dtype=bool)
    touched[idx.reshape(-1)] = True
    assert touched.sum() == n * B * K * C                                    # (the layouts address every element once)
    assert (host[:1 + GUARD] == SENTINEL).all() and (host[1 + GUARD + span:] == SENTINEL).all(), "guard band written"
    assert (body[~touched] == SENTINEL).all(), "an element outside the addressed ones was written"
    return body[idx] if n else np.zeros((0, B, K, C), np.float32), rng.cpu()


def _check(z, keys, pos, n, ncand, C, eps=EPS):
    """Every element within 2 x the reference's error model, finite, |z| <= 5.78 eps -> max measured / allowed."""
    ref = R.row_noise(keys, pos, n, ncand, eps, C)
    allowed = 2.0 * R.row_noise_bound(keys, pos, n, ncand, eps, C)
    assert z.shape == ref.shape and z.dtype == np.float32
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.78 * eps
    ratio = np.abs(z.astype(np.float64) - ref) / allowed
    assert ratio.max() <= 1.0, (keys, pos, n, ncand, C, float(ratio.max()))
    return float(ratio.max())


def _remember(seen, z, keys, pos, n):
    """The bits of every (key, position, candidate) seen so far: whoever draws it again - another layout, batch size or row - must
    draw the same bits."""
    for r, (k, p) in enumerate(zip(keys, pos)):
        for i in range(n):
            for c in range(z.shape[2]):
                bits = z[i, r, c].view(np.uint32)
                first = seen.setdefault((k, p + i, c), bits)
                assert np.array_equal(first, bits), (k, p + i, c, r, len(keys))
    return seen


@pytest.mark.parametrize("C", (1, 3, 4, 6, 56, 57))
def test_kernel_matches_the_reference_in_every_layout(C, gpu_device):
    seen, worst, cases = {}, 0.0, 0
    # B = 5: every key and both positions somewhere, then the same pairs in other rows; B = 1: every pair on its own
    five = [((0, 1, 1 << 32, (1 << 63) - 1, 1), (0, (1 << 32) - 2, (1 << 32) - 2, 0, 0)),
            ((1, (1 << 63) - 1, 0, 1, 1 << 32), (0, 0, 0, (1 << 32) - 2, (1 << 32) - 2))]
    ones = [((k,), (p,)) for k in KEYS for p in POSITIONS]
    for keys, pos in five + ones:
        for n in (1, 4):
            for ncand in (0, 1, 3):
                for layout in ("dense", "padded"):
                    z, rng = _launch(gpu_device, keys, pos, n, ncand, C, layout)
                    assert torch.equal(rng, _rng(keys, pos, "cpu"))                 # advance = 0: nothing moves
                    worst = max(worst, _check(z, keys, pos, n, ncand, C))
                    _remember(seen, z, keys, pos, n)
                    cases += 1
    assert cases == (2 + 8) * 2 * 3 * 2
    report("lfi_row_noise C=%d: %d cases (B 1 / 5, n 1 / 4, ncand 0 / 1 / 3, dense and padded), max measured / allowed error %.3f"
           % (C, cases, worst))


def test_more_items_than_threads_more_rows_than_a_block_and_eps_one(gpu_device):
    """The rollout shape (n, ncand) = (8, 8) at C = 57 is 960 Philox calls for a row's 256 threads; 300 rows are 300 workgroups;
    eps = 1 and a tiny eps."""
    keys, pos = (5, (1 << 63) - 1, 1 << 32), (7, (1 << 32) - 3, (1 << 33) + 1)
    seen = {}
    for layout in ("dense", "padded"):
        z, _ = _launch(gpu_device, keys, pos, 8, 8, 57, layout, eps=1.0)
        worst = _check(z, keys, pos, 8, 8, 57, eps=1.0)
        _remember(seen, z, keys, pos, 8)
    report("lfi_row_noise (n, ncand, C) = (8, 8, 57), eps 1: max measured / allowed error %.3f" % worst)
    keys = tuple(range(1000, 1300))
    pos = tuple((r * 7919) % 50 for r in range(300))
    z, _ = _launch(gpu_device, keys, pos, 2, 0, 3, "dense")
    report("lfi_row_noise B = 300: max measured / allowed error %.3f" % _check(z, keys, pos, 2, 0, 3))
    z, _ = _launch(gpu_device, (9,), (0,), 4, 3, 6, "dense", eps=1e-3)
    _check(z, (9,), (0,), 4, 3, 6, eps=1e-3)


def test_advance_rides_in_the_launch_and_is_exact(gpu_device):
    keys = (0, 1, 1 << 32, (1 << 63) - 1, 77)
    pos = (0, (1 << 32) - 2, (1 << 40) + 5, (1 << 62) + 1, 3)
    n = 4
    base, _ = _launch(gpu_device, keys, pos, n, 3, 6, "dense")
    for advance in (0, 1, n):
        z, rng = _launch(gpu_device, keys, pos, n, 3, 6, "padded", advance=advance)
        assert np.array_equal(z.view(np.uint32), base.view(np.uint32))             # the draws are those of the positions before the move
        assert torch.equal(rng, _rng(keys, [p + advance for p in pos], "cpu")), advance
    # advance only: positions move, nothing is written (the guard bands and an empty span are checked in _launch)
    z, rng = _launch(gpu_device, keys, pos, 0, 0, 6, "dense", advance=3)
    assert z.size == 0 and torch.equal(rng, _rng(keys, [p + 3 for p in pos], "cpu"))
    # the next call draws what a call at the moved positions draws
    moved, _ = _launch(gpu_device, keys, [p + 3 for p in pos], 1, 0, 6, "dense")
    again, _ = _launch(gpu_device, keys, pos, n, 0, 6, "dense")
    assert np.array_equal(again[3].view(np.uint32), moved[0].view(np.uint32))


def test_row_rng_advance_with_and_without_lengths(gpu_device):
    L = _lib.lib()
    keys = (0, 1, 1 << 32, (1 << 63) - 1, 77)
    pos = (0, (1 << 32) - 2, (1 << 40) + 5, (1 << 62) + 1, 3)
    rng = _rng(keys, pos, gpu_device)
    _lib.check(L.lfi_row_rng_advance(rng.data_ptr(), 5, 6, None, _stream()), "lfi_row_rng_advance")
    assert torch.equal(rng.cpu(), _rng(keys, [p + 6 for p in pos], "cpu"))
    lens = torch.tensor([2, 0, 5, 1, 0], dtype=torch.int32, device=gpu_device)
    _lib.check(L.lfi_row_rng_advance(rng.data_ptr(), 5, 99, lens.data_ptr(), _stream()), "lfi_row_rng_advance")     # (lens wins over delta)
    assert torch.equal(rng.cpu(), _rng(keys, [p + 6 + v for p, v in zip(pos, (2, 0, 5, 1, 0))], "cpu"))
    # more rows than one block
    big = torch.zeros(600, 2, dtype=torch.int64, device=gpu_device)
    big[:, 0] = torch.arange(600, device=gpu_device)
    lens = (torch.arange(600, device=gpu_device) % 7).to(torch.int32)
    _lib.check(L.lfi_row_rng_advance(big.data_ptr(), 600, 0, lens.data_ptr(), _stream()), "lfi_row_rng_advance")
    _lib.check(L.lfi_row_rng_advance(big.data_ptr(), 600, 2, None, _stream()), "lfi_row_rng_advance")
    want = torch.stack([torch.arange(600), torch.arange(600) % 7 + 2], 1)
    assert torch.equal(big.cpu(), want)
