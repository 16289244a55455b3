"""What the non-finite step guard has to compute: torch.optim.{Adam, SGD, RMSprop} + global-norm clip + the EMA lerp, with
optimizer.step() and the EMA update simply NOT CALLED on a step whose gradient holds a NaN or an Inf (what torch.amp.GradScaler does
on an overflow). Parameters and state are fp32 tensors stepped by torch itself; the norm is summed in fp64, as lfi_grad_sumsq sums
it, so 3e38-sized gradients are finite and "the norm is finite" is "every element is finite".

`defect` plants one wrong behaviour at a time (tests/test_guard_cpu.py shows that `mismatches`, the comparison the GPU tests make,
catches each of them):
    "t_on_skip"          Adam's / RMSprop's step count advances on a skipped step
    "momentum_on_skip"   a skipped first step leaves a (zero) momentum buffer behind: the next step is no longer the first
    "ema_on_skip"        the average is updated (first time: created) on a skipped step
    "inf_is_finite"      only NaN counts as non-finite
    "big_is_nonfinite"   the norm is summed in fp32, where 3e38^2 overflows
"""
import math

import numpy as np
import torch

from ema_expected import ema_coefficient, worst_ratio

GATE = 2e-6      # per update, of max(1, max |p|): the gate of tests/test_gpu_optimizers.py
DEFECTS = ("t_on_skip", "momentum_on_skip", "ema_on_skip", "inf_is_finite", "big_is_nonfinite")
_CLS = {"adam": torch.optim.Adam, "sgd": torch.optim.SGD, "rmsprop": torch.optim.RMSprop}


class GuardedRun:
    """One run: p (fp32, a copy of p0), the torch optimiser's state, ema (fp32, None until the first taken step), the counters the
    device record keeps. step(grad) -> True when the step was taken."""

    def __init__(self, name, kwargs, lr, p0, clip=0.0, gmul=1.0, ema_decay=None, defect=None):
        assert defect is None or defect in DEFECTS, defect
        kw = dict(kwargs)
        if "betas" in kw:
            kw["betas"] = tuple(kw["betas"])
        self.p = torch.nn.Parameter(torch.as_tensor(p0).detach().to(torch.float32).cpu().clone())
        self.opt = _CLS[name]([self.p], lr=lr, foreach=False, **kw)
        self.clip, self.gmul, self.ema_decay, self.defect = float(clip), float(gmul), ema_decay, defect
        self.ema = None
        self.skipped = self.consecutive = self.applied = 0
        self.last_norm, self.max_norm = 0.0, 0.0

    def set_lr(self, lr):
        for group in self.opt.param_groups:
            group["lr"] = lr

    def _norm(self, g):
        if self.defect == "big_is_nonfinite":
            return float(torch.sqrt((g * g).sum())) * abs(self.gmul)
        return math.sqrt(float((g.double() * g.double()).sum())) * abs(self.gmul)

    def step(self, grad):
        g = torch.as_tensor(grad).detach().to(torch.float32).cpu().clone()
        norm = self._norm(g)
        self.last_norm = norm
        finite = (not math.isnan(norm)) if self.defect == "inf_is_finite" else math.isfinite(norm)
        if not finite:
            self.skipped += 1
            self.consecutive += 1
            state = self.opt.state[self.p]
            if self.defect == "t_on_skip" and "step" in state:
                state["step"] = state["step"] + 1
            if self.defect == "momentum_on_skip" and isinstance(self.opt, torch.optim.SGD) and state.get("momentum_buffer") is None:
                state["momentum_buffer"] = torch.zeros_like(self.p)
            if self.defect == "ema_on_skip" and self.ema_decay:
                self._average()
            return False
        self.applied += 1
        self.consecutive = 0
        self.max_norm = max(self.max_norm, norm)
        coef = np.float32(self.gmul)
        if self.clip > 0.0:
            c = self.clip / (norm + 1e-6)
            if c < 1.0:
                coef = coef * np.float32(c)
        self.p.grad = g * float(coef)
        self.opt.step()
        if self.ema_decay:
            self._average()
        return True

    def _average(self):
        p = self.p.detach()
        if self.ema is None:
            self.ema = p.clone()
        else:
            self.ema = self.ema + np.float32(ema_coefficient(self.ema_decay)) * (p - self.ema)

    def state(self):
        """The optimiser's state under the engine's buffer names (None = does not exist)."""
        st = self.opt.state[self.p]
        if isinstance(self.opt, torch.optim.Adam):
            return {"adam_m": st.get("exp_avg"), "adam_v": st.get("exp_avg_sq"), "opt_aux": st.get("max_exp_avg_sq"),
                    "t": int(st["step"]) if "step" in st else 0}
        if isinstance(self.opt, torch.optim.SGD):
            return {"adam_m": st.get("momentum_buffer"), "adam_v": None, "opt_aux": None, "t": self.applied}
        return {"adam_m": st.get("momentum_buffer"), "adam_v": st.get("square_avg"), "opt_aux": st.get("grad_avg"),
                "t": int(st["step"]) if "step" in st else 0}

    def result(self):
        return {"p": self.p.detach().clone(), "state": self.state(), "ema": None if self.ema is None else self.ema.clone(),
                "skipped": self.skipped, "consecutive": self.consecutive, "applied": self.applied,
                "last_norm": self.last_norm, "max_norm": self.max_norm}


def run(name, kwargs, lr, p0, grads, clip=0.0, gmul=1.0, ema_decay=None, defect=None):
    """The whole gradient sequence -> result()."""
    r = GuardedRun(name, kwargs, lr, p0, clip, gmul, ema_decay, defect)
    for g in grads:
        r.step(g)
    return r.result()


def mismatches(got, want):
    """What differs between two result() dicts (`got` may come from the engine), as a list of strings; empty = they agree.
    Parameters, state buffers and the average: GATE * max(1, max |want|), and NaN anywhere in `got` is a mismatch (the GPU tests
    hold the average to ema_expected's per-update bound on top of this). Counters and Adam's t: equal. A buffer that exists on one
    side only is a mismatch."""
    out = []

    def close(what, a, b):
        if (a is None) != (b is None):
            out.append("%s exists on one side only" % what)
        elif a is not None:
            a, b = torch.as_tensor(a).detach().cpu().double().reshape(-1), torch.as_tensor(b).detach().cpu().double().reshape(-1)
            d = (a - b).abs().max().item() if a.numel() else 0.0
            scale = max(1.0, b.abs().max().item() if b.numel() else 0.0)
            if not d / scale < GATE:      # (NaN fails)
                out.append("%s differs by %.3e of max(1, |want|)" % (what, d / scale))

    close("p", got["p"], want["p"])
    for k in ("adam_m", "adam_v", "opt_aux"):
        close(k, got["state"].get(k), want["state"].get(k))
    if got["state"].get("t") != want["state"].get("t"):
        out.append("t %r != %r" % (got["state"].get("t"), want["state"].get("t")))
    if (got["ema"] is None) != (want["ema"] is None):
        out.append("ema exists on one side only")
    elif got["ema"] is not None:
        close("ema", got["ema"], want["ema"])
    for k in ("skipped", "consecutive", "applied"):
        if got[k] != want[k]:
            out.append("%s %r != %r" % (k, got[k], want[k]))
    return out


__all__ = ["GuardedRun", "run", "mismatches", "worst_ratio", "GATE", "DEFECTS"]
