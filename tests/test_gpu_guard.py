"""GPU: the non-finite step guard, from the decide kernel behind lfi_grad_guard through the guarded optimiser and averaging kernels,
the engine, the eager and the captured training step, the negative-example branch and checkpoints. Reference: tests/guard_expected.py
(torch.optim + clip + the EMA lerp with the poisoned steps not taken). A step is poisoned through its BATCH - one element of p1_face
at a modelled frame set to NaN or +Inf - and every test first asserts that the record reports the skip."""
import copy
import math
import struct
from argparse import Namespace

import pytest
import torch

from ema_expected import worst_ratio
from guard_expected import GATE, GuardedRun, mismatches
from helpers import Fixture, report
from test_gpu_optimizers import CASES

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
BAND = 64             # 8-byte slots (record, work buffer) or floats (optimiser buffers) of guard band around each buffer
SENTINEL = 12345.0
SENTINEL_BITS = struct.unpack("<q", struct.pack("<d", SENTINEL))[0]
KINDS = {"nan": (NAN,), "+inf": (INF,), "-inf": (-INF,), "inf-pair": (INF, -INF)}


def _L():
    from lets_face_it_amd import _lib
    return _lib, _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ 1. the decide kernel through the C ABI
class _DecideArena:
    """record | work (1024 doubles) | sumsq, each between bands of sentinels, in one 8-byte-slot buffer."""

    def __init__(self, device, seed):
        _lib, _ = _L()
        self.S = _lib.GUARD_SLOTS
        self.rec0, self.work0 = BAND, 2 * BAND + self.S
        self.ss0 = self.work0 + 1024 + BAND
        self.whole = torch.full((self.ss0 + 1 + BAND,), SENTINEL_BITS, dtype=torch.int64, device=device)
        self.whole[self.rec0:self.rec0 + self.S] = torch.tensor(seed, dtype=torch.int64)
        self.whole[self.work0:self.work0 + 1024] = 0
        self.before = self.whole.clone()

    def ptr(self, slot):
        return self.whole.data_ptr() + 8 * slot

    def rec(self):
        return self.whole[self.rec0:self.rec0 + self.S].cpu()

    def sumsq_bits(self):
        return int(self.whole[self.ss0])

    def outside_untouched(self):
        mask = torch.ones_like(self.whole, dtype=torch.bool)
        for lo, n in ((self.rec0, self.S), (self.work0, 1024), (self.ss0, 1)):
            mask[lo:lo + n] = False
        return bool((self.whole[mask] == self.before[mask]).all())


def _seed(skipped=5, consecutive=2, applied=7, max_norm=1.0, mom=0, avg=0):
    _lib, _ = _L()
    s = [0] * _lib.GUARD_SLOTS
    s[_lib.GUARD_SKIPPED], s[_lib.GUARD_CONSECUTIVE], s[_lib.GUARD_APPLIED] = skipped, consecutive, applied
    s[_lib.GUARD_MAX_NORM] = struct.unpack("<q", struct.pack("<d", max_norm))[0]
    s[_lib.GUARD_STEP_FLOATS] = struct.unpack("<q", struct.pack("<ff", 0.25, 0.5))[0]
    s[_lib.GUARD_MOMENTUM_LIVE], s[_lib.GUARD_AVERAGE_LIVE] = mom, avg
    return s


def _f64(bits):
    return struct.unpack("<d", struct.pack("<q", int(bits)))[0]


def _floats(bits):
    return struct.unpack("<ff", struct.pack("<q", int(bits)))


def _positions(n):
    """element 0, element n - 1, one in stage 1's 8-way-unrolled body and one in its remainder loop, where they exist: with
    min(1024, ceil(n / 256)) blocks of 256 the unrolled body covers [0, 8 * stride) once n > 7 * stride - of the sizes here only
    2^21 + 5 (stride 2^18: body [0, 2^21), remainder the last five) - and everything else is the remainder loop."""
    stride = min(1024, (n + 255) // 256) * 256
    body = [12345 + 3 * stride] if n > 7 * stride else []
    return sorted({0, n - 1, n // 2, max(0, n - 3)} | set(body))


@pytest.mark.parametrize("n", [1, 3, 1027, 2 ** 20 + 5, 2 ** 21 + 5])
def test_decide_kernel_through_the_c_abi(n, gpu_device):
    _lib, L = _L()
    gen = torch.Generator().manual_seed(n % 1009)
    clean = (torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 4 - 2)).to(gpu_device)
    host = (0.125, 1.5)

    def decide(g, arena, t_host, gmul=1.0, flags=3, beta1=0.9, beta2=0.99):
        rc = L.lfi_grad_guard(g.data_ptr(), n, arena.ptr(arena.ss0), arena.ptr(arena.work0), arena.ptr(arena.rec0), gmul, flags, beta1,
                              beta2, host[0], host[1], t_host, _st())
        assert rc == 0, L.lfi_last_error()
        torch.cuda.synchronize()
        assert arena.outside_untouched(), "the decide launch wrote outside the record, the work buffer and sumsq"
        return arena.rec()

    # clean input: sumsq bit-equal to lfi_grad_sumsq's, the step is taken with the host's floats while t_host == applied + 1
    ref = torch.zeros(1 + 1024, dtype=torch.float64, device=gpu_device)
    assert L.lfi_grad_sumsq(clean.data_ptr(), n, ref.data_ptr(), ref.data_ptr() + 8, _st()) == 0
    a = _DecideArena(gpu_device, _seed(mom=0, avg=3))
    rec = decide(clean, a, t_host=8, gmul=-0.5)
    torch.cuda.synchronize()
    assert a.sumsq_bits() == int(ref[:1].view(torch.int64)[0]), "sumsq differs from lfi_grad_sumsq's"
    norm = math.sqrt(float(ref[0])) * 0.5
    assert (int(rec[_lib.GUARD_APPLY]), int(rec[_lib.GUARD_SKIPPED]), int(rec[_lib.GUARD_CONSECUTIVE]), int(rec[_lib.GUARD_APPLIED])) == (1, 5, 0, 8)
    assert abs(_f64(rec[_lib.GUARD_LAST_NORM]) - norm) <= 2.0 ** -52 * norm      # (one rounding of the root)
    assert _f64(rec[_lib.GUARD_MAX_NORM]) == max(1.0, _f64(rec[_lib.GUARD_LAST_NORM]))
    assert _floats(rec[_lib.GUARD_STEP_FLOATS]) == host
    assert (int(rec[_lib.GUARD_MOMENTUM_LIVE]), int(rec[_lib.GUARD_AVERAGE_LIVE])) == (2, 3), "live flags: (before, after) per slot"
    # a second decide sees the momentum buffer the first step's kernel wrote; flags 0 never makes anything live
    rec = decide(clean, a, t_host=9)
    assert int(rec[_lib.GUARD_MOMENTUM_LIVE]) == 3 and int(rec[_lib.GUARD_APPLIED]) == 9
    b = _DecideArena(gpu_device, _seed())
    rec = decide(clean, b, t_host=8, flags=0)
    assert (int(rec[_lib.GUARD_MOMENTUM_LIVE]), int(rec[_lib.GUARD_AVERAGE_LIVE])) == (0, 0)

    # the host is ahead (it counted skipped steps it has not heard of): floats re-based on the device to t = applied + 1
    c = _DecideArena(gpu_device, _seed())
    rec = decide(clean, c, t_host=11)
    b1, b2 = float(torch.tensor(0.9, dtype=torch.float32)), float(torch.tensor(0.99, dtype=torch.float32))
    want = (host[0] * (1 - b1 ** 11) / (1 - b1 ** 8), 1.0 / math.sqrt(1 - b2 ** 8))
    got = _floats(rec[_lib.GUARD_STEP_FLOATS])
    assert int(rec[_lib.GUARD_APPLIED]) == 8
    assert all(abs(g - w) <= 2.0 ** -23 * abs(w) for g, w in zip(got, want)), (got, want)      # one fp32 rounding of an fp64 value

    # every element +-3e38: legal, taken, finite norm
    big = torch.full((n,), 3e38, device=gpu_device)
    big[::2] = -3e38
    d = _DecideArena(gpu_device, _seed())
    rec = decide(big, d, t_host=8)
    assert int(rec[_lib.GUARD_APPLY]) == 1 and int(rec[_lib.GUARD_APPLIED]) == 8
    assert math.isfinite(_f64(rec[_lib.GUARD_LAST_NORM])) and abs(_f64(rec[_lib.GUARD_LAST_NORM]) / (3e38 * math.sqrt(n)) - 1) < 1e-6

    # every poison kind at every position: skipped, counters moved by one, a non-finite norm, floats and max_norm as they were
    cases = 0
    for kind, values in KINDS.items():
        for pos in _positions(n):
            if len(values) > n:
                continue
            g = clean.clone()
            for k, v in enumerate(values):
                g[(pos + k * (n // 2)) % n if len(values) > 1 else pos] = v
            e = _DecideArena(gpu_device, _seed(mom=0, avg=0))
            rec = decide(g, e, t_host=8)
            what = "n=%d %s at %d" % (n, kind, pos)
            assert int(rec[_lib.GUARD_APPLY]) == 0, what
            assert (int(rec[_lib.GUARD_SKIPPED]), int(rec[_lib.GUARD_CONSECUTIVE]), int(rec[_lib.GUARD_APPLIED])) == (6, 3, 7), what
            assert not math.isfinite(_f64(rec[_lib.GUARD_LAST_NORM])), what
            assert _f64(rec[_lib.GUARD_MAX_NORM]) == 1.0 and _floats(rec[_lib.GUARD_STEP_FLOATS]) == (0.25, 0.5), what
            assert (int(rec[_lib.GUARD_MOMENTUM_LIVE]), int(rec[_lib.GUARD_AVERAGE_LIVE])) == (0, 0), what
            cases += 1
    report("lfi_grad_guard n=%d: sumsq bit-equal to lfi_grad_sumsq, +-3e38 taken, %d poisoned inputs skipped, nothing outside the "
           "record / work / sumsq written" % (n, cases))


def test_decide_reads_a_captured_steps_params_block(gpu_device):
    _lib, L = _L()
    g = torch.randn(1027, device=gpu_device)
    block = torch.zeros(4, dtype=torch.int64, device=gpu_device)
    assert L.lfi_set_step_params_t(block.data_ptr(), 11, 22, 0.125, 1.5, 8, _st()) == 0
    a, b = _DecideArena(gpu_device, _seed()), _DecideArena(gpu_device, _seed())
    assert L.lfi_grad_guard_dev(g.data_ptr(), 1027, a.ptr(a.ss0), a.ptr(a.work0), a.ptr(a.rec0), 1.0, 0, 0.9, 0.99, block.data_ptr(), _st()) == 0
    assert L.lfi_grad_guard(g.data_ptr(), 1027, b.ptr(b.ss0), b.ptr(b.work0), b.ptr(b.rec0), 1.0, 0, 0.9, 0.99, 0.125, 1.5, 8, _st()) == 0
    torch.cuda.synchronize()
    assert block.tolist()[:2] == [11, 22] and int(block[3]) == 8 and _floats(block[2]) == (0.125, 1.5)
    assert torch.equal(a.whole, b.whole) and a.outside_untouched()
    assert int(a.rec()[_lib.GUARD_APPLIED]) == 8 and _floats(a.rec()[_lib.GUARD_STEP_FLOATS]) == (0.125, 1.5)


# ------------------------------------------------------------------ 2. guarded optimiser and averaging kernels through the C ABI
N2 = 1027      # five workgroups, not a multiple of anything


class _OptArena:
    """p | g | m | v | aux | ema between bands of sentinels in one float buffer, plus a record and a finished sumsq."""
    NAMES = ("p", "g", "m", "v", "aux", "ema")

    def __init__(self, device, seed=3):
        _lib, L = _L()
        gen = torch.Generator().manual_seed(seed)
        span = (N2 + 3) // 4 * 4
        self.off = {k: BAND + i * (span + BAND) for i, k in enumerate(self.NAMES)}
        self.whole = torch.full((BAND + len(self.NAMES) * (span + BAND),), SENTINEL, device=device)
        for k in self.NAMES:
            x = torch.randn(N2, generator=gen)
            # (second moments / square averages positive, and large enough that the centered RMSprop's sq - gavg^2 stays positive:
            # a NaN would make every bit comparison below fail for the wrong reason)
            self.whole[self.off[k]:self.off[k] + N2] = (x.abs() + 25.0 if k == "v" else x.abs() if k == "aux" else x).to(device)
        self.sumsq = torch.zeros(1 + 1024, dtype=torch.float64, device=device)
        assert L.lfi_grad_sumsq(self.ptr("g"), N2, self.sumsq.data_ptr(), self.sumsq.data_ptr() + 8, _st()) == 0
        self.rec = torch.zeros(_lib.GUARD_SLOTS, dtype=torch.int64, device=device)

    def ptr(self, k):
        return self.whole.data_ptr() + 4 * self.off[k]

    def set_rec(self, apply, floats=(0.0, 0.0), mom=0, avg=0):
        _lib, _ = _L()
        s = [0] * _lib.GUARD_SLOTS
        s[_lib.GUARD_APPLY] = apply
        s[_lib.GUARD_STEP_FLOATS] = struct.unpack("<q", struct.pack("<ff", *floats))[0]
        s[_lib.GUARD_MOMENTUM_LIVE], s[_lib.GUARD_AVERAGE_LIVE] = mom, avg
        self.rec.copy_(torch.tensor(s, dtype=torch.int64))


def _opt_calls(name, kwargs, arena, first):
    """(unguarded call, guarded call, record settings) for one entry of test_gpu_optimizers.CASES; clip 0.05 bites, gmul 0.5."""
    from lets_face_it_amd.engine import GlowEngine
    _, L = _L()
    a, ss, rec, lr, clip, gmul = arena, arena.sumsq.data_ptr(), arena.rec.data_ptr(), 3e-3, 0.05, 0.5
    if name == "adam":
        b1, b2 = kwargs["betas"]
        wd, ams, t = float(kwargs.get("weight_decay", 0.0)), bool(kwargs.get("amsgrad", False)), 3
        aux = a.ptr("aux") if ams else None
        if wd or ams:
            plain = lambda: L.lfi_adam_clip_step_ex(a.ptr("p"), a.ptr("g"), a.ptr("m"), a.ptr("v"), aux, N2, ss, clip, gmul, lr, b1, b2,
                                                    kwargs["eps"], wd, t, None, _st())
        else:
            plain = lambda: L.lfi_adam_clip_step(a.ptr("p"), a.ptr("g"), a.ptr("m"), a.ptr("v"), N2, ss, clip, gmul, lr, b1, b2,
                                                 kwargs["eps"], t, _st())
        guarded = lambda: L.lfi_adam_clip_step_guard(a.ptr("p"), a.ptr("g"), a.ptr("m"), a.ptr("v"), aux, N2, ss, clip, gmul, b1, b2,
                                                     kwargs["eps"], wd, rec, _st())
        return plain, guarded, {"floats": GlowEngine.adam_step_floats(lr, b1, b2, t)}
    if name == "sgd":
        mom, damp = float(kwargs.get("momentum", 0.0)), float(kwargs.get("dampening", 0.0))
        wd, nest = float(kwargs.get("weight_decay", 0.0)), int(bool(kwargs.get("nesterov", False)))
        buf = a.ptr("m") if mom else None
        plain = lambda: L.lfi_sgd_clip_step(a.ptr("p"), a.ptr("g"), buf, N2, ss, clip, gmul, lr, mom, damp, wd, nest, 1 if first else 2, _st())
        guarded = lambda: L.lfi_sgd_clip_step_guard(a.ptr("p"), a.ptr("g"), buf, N2, ss, clip, gmul, lr, mom, damp, wd, nest, rec, _st())
        return plain, guarded, {"mom": 0 if first else 3}
    alpha, eps = float(kwargs.get("alpha", 0.99)), float(kwargs.get("eps", 1e-8))
    wd, mom = float(kwargs.get("weight_decay", 0.0)), float(kwargs.get("momentum", 0.0))
    buf, gavg = (a.ptr("m") if mom else None), (a.ptr("aux") if kwargs.get("centered") else None)
    plain = lambda: L.lfi_rmsprop_clip_step(a.ptr("p"), a.ptr("g"), a.ptr("v"), buf, gavg, N2, ss, clip, gmul, lr, alpha, eps, wd, mom, _st())
    guarded = lambda: L.lfi_rmsprop_clip_step_guard(a.ptr("p"), a.ptr("g"), a.ptr("v"), buf, gavg, N2, ss, clip, gmul, lr, alpha, eps, wd,
                                                    mom, rec, _st())
    return plain, guarded, {}


@pytest.mark.parametrize("name,kwargs", CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_guarded_optimiser_kernels_through_the_c_abi(name, kwargs, gpu_device):
    for first in ((True, False) if name == "sgd" else (False,)):
        a, b = _OptArena(gpu_device), _OptArena(gpu_device)
        assert torch.equal(a.whole, b.whole)
        before = a.whole.clone()
        plain, _, _ = _opt_calls(name, kwargs, a, first)
        _, guarded, rec = _opt_calls(name, kwargs, b, first)
        # apply == 0: nothing at all is written
        b.set_rec(0, rec.get("floats", (0.0, 0.0)), mom=rec.get("mom", 0))
        assert guarded() == 0
        torch.cuda.synchronize()
        assert torch.equal(b.whole, before), "a skipped step wrote"
        # apply == 1 with the host's floats: the unguarded entry point's bits, bands included
        b.set_rec(1, rec.get("floats", (0.0, 0.0)), mom=rec.get("mom", 0))
        assert plain() == 0 and guarded() == 0
        torch.cuda.synchronize()
        assert not torch.equal(a.whole, before), "the unguarded step did nothing"
        assert torch.equal(a.whole, b.whole), "%s %s first=%s: guarded and unguarded entry points differ" % (name, kwargs, first)
    report("guarded %s %s: bit-identical to the unguarded entry point when applied, nothing written when skipped" % (name, kwargs))


@pytest.mark.parametrize("eoff,poff", [(0, 0), (1, 0), (0, 3)])
def test_guarded_average_through_the_c_abi(eoff, poff, gpu_device):
    _, L = _L()
    a, b = _OptArena(gpu_device), _OptArena(gpu_device)
    before = a.whole.clone()
    ema_a, p_a, ema_b, p_b = a.ptr("ema") + 4 * eoff, a.ptr("p") + 4 * poff, b.ptr("ema") + 4 * eoff, b.ptr("p") + 4 * poff
    n = N2 - 3
    b.set_rec(0, avg=3)
    assert L.lfi_ema_update_guard(ema_b, p_b, n, 0.99, b.rec.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(b.whole, before), "a skipped update wrote"
    b.set_rec(1, avg=3)      # live: the lerp, lfi_ema_update's bits
    assert L.lfi_ema_update(ema_a, p_a, n, 0.99, _st()) == 0 and L.lfi_ema_update_guard(ema_b, p_b, n, 0.99, b.rec.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a.whole, b.whole) and not torch.equal(a.whole, before)
    b.set_rec(1, avg=2)      # bit 0 clear: no average yet - a copy of the parameters
    assert L.lfi_ema_update_guard(ema_b, p_b, n, 0.99, b.rec.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    e0, p0 = b.off["ema"] + eoff, b.off["p"] + poff
    assert torch.equal(b.whole[e0:e0 + n], b.whole[p0:p0 + n])
    want = a.whole.clone()
    want[e0:e0 + n] = a.whole[p0:p0 + n]
    assert torch.equal(b.whole, want), "the copy wrote outside the average"


def test_guard_entry_points_refuse_bad_arguments_and_launch_nothing(gpu_device):
    _, L = _L()
    a = _OptArena(gpu_device)
    a.set_rec(1, (1e-3, 1.0), mom=3, avg=3)
    work = torch.zeros(1 + 1024, dtype=torch.float64, device=gpu_device)
    before, rec_before = a.whole.clone(), a.rec.clone()
    p, g, m, v, e, ss, rec, odd = a.ptr("p"), a.ptr("g"), a.ptr("m"), a.ptr("v"), a.ptr("ema"), a.sumsq.data_ptr(), a.rec.data_ptr(), a.rec.data_ptr() + 4
    st = _st()
    bad = {
        "lfi_grad_guard": [lambda r=r: L.lfi_grad_guard(g, N2, work.data_ptr(), work.data_ptr() + 8, r, 1.0, 0, 0.9, 0.99, 1e-3, 1.0, 1, st) for r in (None, odd)]
        + [lambda: L.lfi_grad_guard(None, N2, work.data_ptr(), work.data_ptr() + 8, rec, 1.0, 0, 0.9, 0.99, 1e-3, 1.0, 1, st),
           lambda: L.lfi_grad_guard(g, N2, work.data_ptr(), work.data_ptr() + 8, rec, 1.0, 0, 0.9, 0.99, 1e-3, 1.0, 0, st),
           lambda: L.lfi_grad_guard(g, N2, work.data_ptr(), work.data_ptr() + 8, rec, 1.0, 4, 0.9, 0.99, 1e-3, 1.0, 1, st),
           lambda: L.lfi_grad_guard(g, N2, work.data_ptr(), work.data_ptr() + 8, rec, 1.0, 0, 1.0, 0.99, 1e-3, 1.0, 1, st),
           lambda: L.lfi_grad_guard(g, -1, work.data_ptr(), work.data_ptr() + 8, rec, 1.0, 0, 0.9, 0.99, 1e-3, 1.0, 1, st)],
        "lfi_grad_guard_dev": [lambda: L.lfi_grad_guard_dev(g, N2, work.data_ptr(), work.data_ptr() + 8, rec, 1.0, 0, 0.9, 0.99, None, st),
                               lambda: L.lfi_grad_guard_dev(g, N2, work.data_ptr(), work.data_ptr() + 8, None, 1.0, 0, 0.9, 0.99, rec, st)],
        "lfi_set_step_params_t": [lambda: L.lfi_set_step_params_t(None, 1, 2, 1e-3, 1.0, 1, st),
                                  lambda: L.lfi_set_step_params_t(rec, 1, 2, 1e-3, 1.0, 0, st)],
        "lfi_adam_clip_step_guard": [lambda r=r: L.lfi_adam_clip_step_guard(p, g, m, v, None, N2, ss, 1.0, 1.0, 0.9, 0.99, 1e-8, 0.0, r, st) for r in (None, odd)]
        + [lambda: L.lfi_adam_clip_step_guard(None, g, m, v, None, N2, ss, 1.0, 1.0, 0.9, 0.99, 1e-8, 0.0, rec, st),
           lambda: L.lfi_adam_clip_step_guard(p, g, m, v, None, N2, None, 1.0, 1.0, 0.9, 0.99, 1e-8, 0.0, rec, st),
           lambda: L.lfi_adam_clip_step_guard(p, g, m, v, None, N2, ss, 1.0, 1.0, 0.9, 0.99, 1e-8, -1.0, rec, st)],
        "lfi_sgd_clip_step_guard": [lambda r=r: L.lfi_sgd_clip_step_guard(p, g, m, N2, ss, 1.0, 1.0, 1e-3, 0.9, 0.0, 0.0, 0, r, st) for r in (None, odd)]
        + [lambda: L.lfi_sgd_clip_step_guard(p, g, None, N2, ss, 1.0, 1.0, 1e-3, 0.9, 0.0, 0.0, 0, rec, st),
           lambda: L.lfi_sgd_clip_step_guard(p, g, m, N2, ss, 1.0, 1.0, 1e-3, 0.9, 0.1, 0.0, 1, rec, st)],
        "lfi_rmsprop_clip_step_guard": [lambda r=r: L.lfi_rmsprop_clip_step_guard(p, g, v, None, None, N2, ss, 1.0, 1.0, 1e-3, 0.99, 1e-8, 0.0, 0.0, r, st) for r in (None, odd)]
        + [lambda: L.lfi_rmsprop_clip_step_guard(p, g, None, None, None, N2, ss, 1.0, 1.0, 1e-3, 0.99, 1e-8, 0.0, 0.0, rec, st),
           lambda: L.lfi_rmsprop_clip_step_guard(p, g, v, None, None, N2, ss, 1.0, 1.0, 1e-3, 0.99, 1e-8, 0.0, 0.5, rec, st)],
        "lfi_ema_update_guard": [lambda r=r: L.lfi_ema_update_guard(e, p, N2, 0.9, r, st) for r in (None, odd)]
        + [lambda: L.lfi_ema_update_guard(e, p, N2, 1.0, rec, st), lambda: L.lfi_ema_update_guard(e, e + 4, N2, 0.9, rec, st),
           lambda: L.lfi_ema_update_guard(None, p, N2, 0.9, rec, st)],
    }
    for entry, calls in bad.items():
        for i, call in enumerate(calls):
            rc = call()
            msg = L.lfi_last_error()
            assert rc != 0, (entry, i)
            assert msg and entry.encode() + b":" in msg, (entry, i, msg)
    torch.cuda.synchronize()
    assert torch.equal(a.whole, before) and torch.equal(a.rec, rec_before) and not work.any(), "a refused call wrote"


# ------------------------------------------------------------------ the training step
def _module(fx_name, gpu_device, name="adam", kwargs=None, guard=True, ema_decay=None, negative=False, masks=True):
    """The module of test_gpu_optimizers (fixture weights, injected masks, exact-f32 GEMMs) with Optim.skip_nonfinite."""
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    fx = Fixture(fx_name)
    hp = Namespace(**copy.deepcopy(fx.hp))
    hp.Train["use_negative_nll_loss"] = bool(negative)
    hp.gradient_clip_val = 5.0
    hp.Optim["name"] = name
    hp.Optim["args"][name] = dict(kwargs if kwargs is not None else {"betas": [0.9, 0.9999], "eps": 1e-8})
    if guard:
        hp.Optim["skip_nonfinite"] = True
    if ema_decay is not None:
        hp.Optim["ema_decay"] = ema_decay
    hp.engine_precision = "f32"
    lm = LetsFaceItGlow(hp)
    lm.seq_glow.load_state_dict(fx.state_dict(torch.float32))
    lm.to(gpu_device)
    lm.seq_glow.glow.set_actnorm_init(True)
    lm.train()
    lm.seq_glow.injected_masks = ({k: v.to(gpu_device) for k, v in fx.masks(torch.float32).items()} if fx.masks() else None) if masks else None
    return lm, {k: v.to(gpu_device) for k, v in fx.batch(torch.float32).items()}, fx


def _poisoned(batch, fx, value, row=1, chan=2):
    """One element of p1_face at a modelled frame (t >= start) of one row."""
    out = {k: v.clone() for k, v in batch.items()}
    out["p1_face"][row % out["p1_face"].shape[0], fx.start + 1, chan % fx.C] = value
    return out


def _record(eng):
    """The record as it is, WITHOUT GlowEngine.guard_state's reconciliation: the host goes on believing every step was taken."""
    _lib, _ = _L()
    r = eng.guard.cpu()
    return {"apply": int(r[_lib.GUARD_APPLY]), "skipped": int(r[_lib.GUARD_SKIPPED]), "applied": int(r[_lib.GUARD_APPLIED]),
            "mom": int(r[_lib.GUARD_MOMENTUM_LIVE]), "avg": int(r[_lib.GUARD_AVERAGE_LIVE]), "norm": _f64(r[_lib.GUARD_LAST_NORM])}


def _bufs(eng):
    return {"params": eng.params, "adam_m": eng.adam_m, "adam_v": eng.adam_v, "opt_aux": eng.__dict__.get("opt_aux"), "ema": eng.ema}


ORACLE_CASES = [next(c for c in CASES if c[0] == name) for name in ("sgd", "rmsprop", "adam")] + [("sgd", {"momentum": 0.8, "dampening": 0.1})]
POISONED_STEPS = (1, 3, 4)      # of six: the first step, and two in a row


@pytest.mark.parametrize("fx_name", ["tiny", "mid"])
@pytest.mark.parametrize("kind", ["nan", "+inf"])
@pytest.mark.parametrize("name,kwargs", ORACLE_CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(ORACLE_CASES)])
def test_fused_steps_against_the_oracle(fx_name, kind, name, kwargs, gpu_device):
    """The host is never told about a skip before the end (the record is read raw), so every step after the first skip runs with
    step floats re-based on the device."""
    decay, lr = 0.99, 3e-3
    lm, batch, fx = _module(fx_name, gpu_device, name, kwargs, ema_decay=decay)
    bad = _poisoned(batch, fx, KINDS[kind][0])
    eng = lm.seq_glow._ensure_engine(gpu_device)
    ref = GuardedRun(name, kwargs, lr, eng.params, clip=5.0, ema_decay=decay)
    worst_p, worst_ema, seen_skips = 0.0, 0.0, 0
    for step in range(1, 7):
        poisoned = step in POISONED_STEPS
        before = {k: (None if v is None else v.clone()) for k, v in _bufs(eng).items()}
        rec_before = _record(eng) if eng.guard is not None else {"mom": 0, "avg": 0, "skipped": 0, "applied": 0}
        lm.fused_training_step(bad if poisoned else batch, lr)
        rec = _record(eng)
        assert rec["apply"] == (0 if poisoned else 1), "step %d: poisoned=%s but the record says apply=%d (norm %r)" % (
            step, poisoned, rec["apply"], rec["norm"])
        took = ref.step(eng.grads)
        assert took == (not poisoned), "the engine's own gradient of step %d is %sfinite" % (step, "" if took else "non-")
        after = _bufs(eng)
        if poisoned:
            seen_skips += 1
            assert not math.isfinite(rec["norm"])
            for k, v in before.items():
                if v is not None:
                    assert torch.equal(after[k], v), "step %d (skipped) changed %s" % (step, k)
            # what did not exist before a skipped step still does not, as far as the device is concerned
            assert rec["mom"] >> 1 == rec_before["mom"] >> 1 and rec["avg"] >> 1 == rec_before["avg"] >> 1
        else:
            want = ref.result()
            d = (eng.params.cpu().double() - want["p"].double()).abs().max().item() / max(1.0, want["p"].abs().max().item())
            worst_p = max(worst_p, d)
            assert d < GATE, "step %d: parameters differ from the oracle by %.3e" % (step, d)
            if before["ema"] is None or rec_before["avg"] >> 1 == 0:
                assert torch.equal(eng.ema, eng.params), "the first average is a copy"
            else:
                worst_ema = max(worst_ema, worst_ratio(eng.ema, before["ema"], eng.params, decay))
            with torch.no_grad():      # one update per comparison: rounding does not compound into the next step
                ref.p.copy_(eng.params.cpu())
                ref.ema = eng.ema.cpu().clone()
        assert (rec["skipped"], rec["applied"]) == (seen_skips, step - seen_skips)
    assert worst_ema <= 1.0, worst_ema
    assert eng.step_count == 6, "the host has not been told yet"
    gs = eng.guard_state()
    assert (gs["skipped"], gs["consecutive"], gs["applied"]) == (3, 0, 3) and math.isfinite(gs["last_norm"]) and gs["max_norm"] > 0
    assert eng.step_count == 3 and eng.ema_updates == 3
    # (the state buffers are left out: they drift by design, only the parameters are re-synchronised per step)
    got = {"p": eng.params, "state": {"t": eng.step_count}, "ema": eng.ema, **gs}
    want = ref.result()
    want["state"] = {"t": want["state"]["t"]}
    assert mismatches(got, want) == []
    report("guarded fused %s %s on %s, steps 1, 3, 4 poisoned with %s: worst parameter difference per update %.2e (gate %.0e), worst "
           "average |err| / bound %.3f, skipped steps bit-unchanged, counters 3 / 0 / 3" % (name, kwargs, fx_name, kind, worst_p, GATE, worst_ema))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "step_graph"])
def test_guard_on_and_nothing_poisoned_is_the_unguarded_run(graph, gpu_device):
    runs = []
    for guard in (False, True):
        torch.manual_seed(7)
        lm, batch, _ = _module("tiny", gpu_device, guard=guard, ema_decay=0.99, masks=not graph)
        lm.step_graph = graph
        for i in range(4):
            lm.fused_training_step(batch, 1e-3 * (1 + i % 2))
        eng = lm.seq_glow.engine
        assert (eng.guard is not None) == guard
        graphs = [v for v in getattr(lm, "_step_graphs", {}).values() if isinstance(v, dict)]
        assert len(graphs) == (1 if graph else 0) and not getattr(lm, "_step_graphs", {}).get("broken")
        if guard:
            gs = eng.guard_state()
            assert (gs["skipped"], gs["applied"]) == (0, 4)
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.ema.clone(), eng.step_count, eng.ema_updates))
    for a, b, what in zip(runs[0], runs[1], ("params", "adam_m", "adam_v", "ema", "step_count", "ema_updates")):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b, what


def test_captured_step_skips_like_the_eager_step(gpu_device):
    """Eight steps, the sixth poisoned - a replay, the graph is captured at the third: the decide node reads t_host from the params
    block, steps 7 and 8 run on re-based floats in both modes (and with the other learning rate)."""
    fx = Fixture("tiny")
    gen = torch.Generator().manual_seed(5)
    base = fx.batch(torch.float32)
    batches = [{k: (v + 0.05 * i * torch.randn(v.shape, generator=gen)).to(gpu_device) for k, v in base.items()} for i in range(2)]
    runs = {}
    for graph in (False, True):
        torch.manual_seed(7)
        lm, _, _ = _module("tiny", gpu_device, ema_decay=0.99, masks=False)
        lm.step_graph = graph
        eng = lm.seq_glow._ensure_engine(gpu_device)
        for i in range(8):
            b = batches[i % 2]
            before = eng.params.clone()
            lm.fused_training_step(_poisoned(b, fx, NAN) if i == 5 else b, 1e-3 * (1 + i % 2))
            rec = _record(eng)
            assert rec["apply"] == (0 if i == 5 else 1), (graph, i, rec)
            assert torch.equal(eng.params, before) == (i == 5), (graph, i)
        graphs = [v for v in getattr(lm, "_step_graphs", {}).values() if isinstance(v, dict)]
        assert len(graphs) == (1 if graph else 0) and not getattr(lm, "_step_graphs", {}).get("broken")
        gs = eng.guard_state()
        assert (gs["skipped"], gs["consecutive"], gs["applied"], eng.step_count, eng.ema_updates) == (1, 0, 7, 7, 7)
        runs[graph] = (eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.ema.clone())
    for a, b, what in zip(runs[False], runs[True], ("params", "adam_m", "adam_v", "ema")):
        assert torch.equal(a, b), "%s differs between eager and replayed guarded steps" % what
    report("guarded steps under hipGraph replay vs eager launches, 8 steps, step 6 poisoned: parameters, moments and average bit-identical")


def test_poisoned_negative_step_keeps_the_mismatched_nll(gpu_device):
    lm, batch, fx = _module("tiny", gpu_device, negative=True)
    assert lm.missmatched_modalities
    lm._negative_branch = lambda: True
    eng = lm.seq_glow._ensure_engine(gpu_device)
    lm.fused_training_step(batch, 1e-3)
    kept = float(lm.last_missmatched_nll)
    assert math.isfinite(kept) and _record(eng)["apply"] == 1
    lm.fused_training_step(_poisoned(batch, fx, NAN, row=0), 1e-3)
    assert _record(eng)["apply"] == 0, "the poisoned negative step was not skipped"
    assert float(lm.last_missmatched_nll) == kept and lm._last_mm() == kept
    # without the guard the same step writes the NaN
    off, batch_off, _ = _module("tiny", gpu_device, negative=True, guard=False)
    off._negative_branch = lambda: True
    off.fused_training_step(_poisoned(batch_off, fx, NAN, row=0), 1e-3)
    assert math.isnan(float(off.last_missmatched_nll))


def test_resume_after_a_skip_continues_the_uninterrupted_run(gpu_device, tmp_path):
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    from lets_face_it_amd.trainer import Trainer
    lm, batch, fx = _module("tiny", gpu_device, ema_decay=0.9)
    bad = _poisoned(batch, fx, INF)
    for b in (batch, bad, batch):
        lm.fused_training_step(b, 3e-3)
    path = str(tmp_path / "guard.ckpt")
    Trainer(lm.hparams, device=gpu_device, checkpoint_dir="").save_checkpoint(lm, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["optimizer_state"]["guard"]["skipped"] == 1 and ckpt["optimizer_state"]["guard"]["applied"] == 2
    assert ckpt["optimizer_state"]["step_count"] == 2 and ckpt["optimizer_state"]["ema_updates"] == 2
    lm2 = LetsFaceItGlow(Namespace(**copy.deepcopy(vars(lm.hparams))))
    tr2 = Trainer(lm2.hparams, device=gpu_device, checkpoint_dir="")
    tr2.resume(lm2, path)
    assert tr2._guard_seen == 1
    lm2.train()
    lm2.seq_glow.injected_masks = lm.seq_glow.injected_masks
    for b in (bad, batch):
        lm.fused_training_step(b, 3e-3)
        lm2.fused_training_step(b, 3e-3)
    e1, e2 = lm.seq_glow.engine, lm2.seq_glow.engine
    assert e1.guard_state() == e2.guard_state() and e2.guard_state()["skipped"] == 2 and e2.guard_state()["applied"] == 3
    for k in ("params", "adam_m", "adam_v", "ema"):
        assert torch.equal(getattr(e1, k), getattr(e2, k)), k
    assert (e1.step_count, e1.ema_updates) == (e2.step_count, e2.ema_updates) == (3, 3)


def test_a_buffer_whose_every_update_was_skipped_is_no_average(gpu_device):
    lm, batch, fx = _module("tiny", gpu_device, ema_decay=0.9)
    lm.fused_training_step(_poisoned(batch, fx, NAN), 3e-3)
    eng = lm.seq_glow.engine
    assert _record(eng)["apply"] == 0
    with pytest.raises(RuntimeError, match="no averaged weights"):
        eng.swap_ema()
    state = eng.optimizer_state()
    assert state["ema"] is None and state["ema_updates"] == 0 and state["step_count"] == 0 and state["guard"]["skipped"] == 1
    lm.fused_training_step(batch, 3e-3)
    assert torch.equal(eng.ema, eng.params) and eng.guard_state()["applied"] == 1 and eng.ema_updates == 1
