"""What the running average of the weights (Polyak / EMA; lfi_ema_update, GlowEngine.ema_update) has to hold, in fp64, and how far
an fp32 update may be from it.

The update is the lerp of torch.optim.swa_utils.get_ema_multi_avg_fn(decay): ema += a (p - ema) with a = 1 - decay, and the first
update is a copy (AveragedModel while n_averaged == 0). The kernel takes `decay` as a float and forms a = (float)(1.0 - (double)decay)
on the host: the reference here rounds the same way, so it is compared on the coefficient the kernel really uses
(for decay = 0.9999 the float's 1 - decay is 1.00017e-4, not 1e-4)."""
import numpy as np
import torch


def ema_coefficient(decay):
    """a = 1 - decay as the C entry point forms it: decay rounded to fp32, the difference in double, rounded to fp32."""
    return float(np.float32(1.0 - float(np.float32(decay))))


def ema_step(ema, p, decay):
    """One update in fp64: a copy of p when there is no average yet (ema None), else ema + a (p - ema). Returns a new tensor."""
    p = torch.as_tensor(p).to(torch.float64)
    if ema is None:
        return p.clone()
    ema = torch.as_tensor(ema).to(torch.float64)
    return ema + ema_coefficient(decay) * (p - ema)


def ema_bound(ema, p):
    """Per-element bound of an fp32 update against ema_step on the same fp32 inputs: 5 * 2^-24 * max(|p|, |ema|).
    Three roundings of relative size 2^-24: the subtraction (|p - ema| <= 2 max), the product when it is not fused (a <= 1: <= 2 max)
    and the sum (the result lies between ema and p: <= max) - (2 + 2 + 1) * 2^-24 * max."""
    m = torch.maximum(torch.as_tensor(p).to(torch.float64).abs(), torch.as_tensor(ema).to(torch.float64).abs())
    return 5.0 * 2.0 ** -24 * m


def worst_ratio(got, ema_before, p, decay):
    """max over elements of |got - ema_step(ema_before, p)| / ema_bound: <= 1 passes. Elements whose bound is 0 (p = ema = 0) must be
    exact: they count as 0 when they are and inf when not."""
    want = ema_step(ema_before, p, decay)
    err = (torch.as_tensor(got).to(torch.float64) - want).abs()
    bound = ema_bound(ema_before, p).to(err.device)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def trajectory_worst_ratio(emas, params, decay):
    """The check the step tests make, over a whole run: emas[k] = the average after update k, params[k] = the parameters it was
    updated with. Update 0 must be a bit-exact copy (inf otherwise); every later one is held to ema_bound against ema_step of the
    PREVIOUS measured average, so that each comparison covers one update and rounding does not compound."""
    if not torch.equal(torch.as_tensor(emas[0]), torch.as_tensor(params[0])):
        return float("inf")
    return max([0.0] + [worst_ratio(emas[k], emas[k - 1], params[k], decay) for k in range(1, len(emas))])
