"""CPU: the fp64 reference of the weight average (tests/ema_expected.py) against torch.optim.swa_utils, its power to detect wrong
updates, and the validation of the Optim["ema_decay"] hparam at construction."""
import copy
from argparse import Namespace

import numpy as np
import pytest
import torch

from ema_expected import ema_coefficient, ema_step, trajectory_worst_ratio
from helpers import Fixture


@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_helper_agrees_with_torch_averaged_model(decay):
    """Five updates of a small fp64 module, the first a copy. torch is given the decay as the C entry point sees it (rounded to
    fp32): 1 - decay is then exact in fp32 as well, so both sides use one coefficient and differ by fp64 rounding only."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).double()
    d32 = float(np.float32(decay))
    assert ema_coefficient(decay) == 1.0 - d32
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(d32))
    mine = None
    for step in range(5):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.3)
        avg.update_parameters(m)
        flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
        mine = ema_step(mine, flat, decay)
        if step == 0:
            assert torch.equal(mine, flat)
        theirs = torch.cat([p.detach().reshape(-1) for p in avg.module.parameters()])
        assert float((mine - theirs).abs().max()) <= 1e-15, step
    assert int(avg.n_averaged) == 5


def _run(update, decay, steps=5, n=257):
    """An fp32 run of `update(ema, p, k) -> ema` as the kernel would make it; returns (emas, params)."""
    g = torch.Generator().manual_seed(11)
    p = torch.randn(n, generator=g)
    emas, params, ema = [], [], None
    for k in range(steps):
        p = p + 0.1 * torch.randn(n, generator=g)
        ema = update(ema, p, k)
        emas.append(ema.clone())
        params.append(p.clone())
    return emas, params


@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_helper_detects_planted_errors(decay):
    a = torch.tensor(ema_coefficient(decay), dtype=torch.float32)

    def good(ema, p, k):
        return p.clone() if ema is None else ema + a * (p - ema)

    def exchanged(ema, p, k):        # a and 1 - a the wrong way round
        return p.clone() if ema is None else ema + (1 - a) * (p - ema)

    def first_not_a_copy(ema, p, k):   # starts from zeros instead of the parameters
        return a * p if ema is None else ema + a * (p - ema)

    def skipped(ema, p, k):          # update 3 does not happen
        return good(ema, p, k) if k != 3 else ema.clone()

    assert trajectory_worst_ratio(*_run(good, decay), decay) <= 1.0
    for planted in (exchanged, first_not_a_copy, skipped):
        assert trajectory_worst_ratio(*_run(planted, decay), decay) > 100.0, planted.__name__


def _hparams(**optim):
    hp = Namespace(**copy.deepcopy(Fixture("tiny").hp))
    hp.Optim.update(optim)
    return hp


@pytest.mark.parametrize("value", [1, 1.0, -0.1, "x", True, float("nan"), [0.9]])
def test_bad_ema_decay_raises_at_construction(value):
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    with pytest.raises(ValueError, match="ema_decay"):
        LetsFaceItGlow(_hparams(ema_decay=value))


def test_ema_decay_absent_none_or_zero_is_off_and_a_fraction_is_kept():
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    assert "ema_decay" not in Fixture("tiny").hp["Optim"]
    assert LetsFaceItGlow(_hparams()).ema_decay is None
    for off in (None, 0, 0.0):
        assert LetsFaceItGlow(_hparams(ema_decay=off)).ema_decay is None
    assert LetsFaceItGlow(_hparams(ema_decay=0.9999)).ema_decay == 0.9999
