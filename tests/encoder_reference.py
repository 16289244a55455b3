"""One window-encoder modality as include/lfi.h states it, in plain torch (any dtype, any device): the definition the HIP kernels
behind lfi_encode_windows_fwd / _bwd / _scatter are compared with, an arithmetic model of their documented roundings, and the
comparison both the GPU tests and the planted-error test go through.

The recurrences are torch.nn.GRU's and torch.nn.LSTM's documented equations (gate blocks r, z, n and i, f, g, o; the gate order
oracle/seqglow_oracle.py's gru_cell / lstm_cell use):

    GRU   r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   n = tanh(gi_n + r * gh_n)   h' = (1 - z) * n + z * h
    LSTM  i, f, o = s(pre_i), s(pre_f), s(pre_o)    g = tanh(pre_g)   c' = f * c + i * g   h' = o * tanh(c')   (pre = gi + gh)

with gi = mask[w, s] * Xp[row(w, s)] + b_ih, gh = h W_hh^T + b_hh, h = c = 0 at the first history step. Window w = n * B + b reads
rows b * T + pos0 + n + s (s < hist, pos0 = start - hist + 1) of the projected input Xp (B * T x G; G = 3 hid, LSTM 4 hid).

A run is a dict of tensors: features (F x hid (1 + dup)), hseq (hist x F x hid), dgi / dgh (hist x F x G: gradients of the input-side /
hidden-side pre-activations, dgi before the dropout mask), dXp (B * T x G), dW_hh (G x hid), db_ih, db_hh (G), for the loss
(features * dcond[:, col : col + hid (1 + dup)]).sum().
"""
from collections import namedtuple

import torch

from helpers import rel_l2

Dims = namedtuple("Dims", "B T N start hist hid col dup")
QUANTITIES = ("features", "hseq", "dgi", "dgh", "dXp", "dW_hh", "db_ih", "db_hh")

# The bound of compare(): err(got) <= MODEL_FACTOR * err(model) + F32_FACTOR * err(fp32), all three against the exact (fp64) run.
MODEL_FACTOR = 3.0
F32_FACTOR = 8.0


def window_rows(dims, device=None):
    """(F x hist) row indices into Xp: window w = n * B + b, step s reads row b * T + pos0 + n + s."""
    pos0 = dims.start - dims.hist + 1
    assert pos0 >= 0 and dims.start + dims.N <= dims.T
    w = torch.arange(dims.N * dims.B, device=device)
    n, b = w // dims.B, w % dims.B
    return (b * dims.T + pos0 + n).unsqueeze(1) + torch.arange(dims.hist, device=device).unsqueeze(0)


def windows_forward(Xp, whh, b_ih, b_hh, mask, dims, lstm=False, taps=None, h0=None, mm=torch.matmul, sig=torch.sigmoid, tanh=torch.tanh):
    """-> (hseq [hist][F][hid], features [F][hid (1 + dup)]). mask: (F x hist) multipliers of the INPUT, or None.
    taps: a list that receives per step the pre-activation tensors (gi, gh) (LSTM: (pre, pre)), each with its gradient retained when
    it needs one: their .grad after backward() is dgi[s] / dgh[s].
    h0 (F x hid, default zero: the definition), mm, sig, tanh: the state the recurrence starts from, the product h W_hh^T and the gate
    non-linearities, for an arithmetic model or a planted defect built on this recurrence (tests/frame_reference.py); the defaults
    are the definition."""
    F, hid = dims.N * dims.B, dims.hid
    rows = window_rows(dims, Xp.device)
    h = Xp.new_zeros(F, hid) if h0 is None else h0
    c = Xp.new_zeros(F, hid)
    hs = []
    for s in range(dims.hist):
        x = Xp[rows[:, s]]
        if mask is not None:
            x = mask[:, s].to(Xp.dtype).unsqueeze(1) * x
        gi = x + b_ih
        gh = mm(h, whh.t()) + b_hh
        if lstm:
            pre = gi + gh
            if taps is not None:
                if pre.requires_grad:
                    pre.retain_grad()
                taps.append((pre, pre))
            i, f, g, o = pre[:, :hid], pre[:, hid:2 * hid], pre[:, 2 * hid:3 * hid], pre[:, 3 * hid:]
            c = sig(f) * c + sig(i) * tanh(g)
            h = sig(o) * tanh(c)
        else:
            if taps is not None:
                if gi.requires_grad:
                    gi.retain_grad()
                    gh.retain_grad()
                taps.append((gi, gh))
            r = sig(gi[:, :hid] + gh[:, :hid])
            z = sig(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
            n = tanh(gi[:, 2 * hid:] + r * gh[:, 2 * hid:])
            h = (1.0 - z) * n + z * h
        hs.append(h)
    return torch.stack(hs), (torch.cat([h, h], dim=1) if dims.dup else h)


def _dfeat(dcond, dims):
    return dcond[:, dims.col:dims.col + dims.hid * (1 + dims.dup)]


def run_autograd(inp, dims, dtype=torch.float64, lstm=False):
    """The reference run: windows_forward in `dtype` with autograd. fp64 is the exact reference, fp32 the second term of the bound.
    inp: dict Xp, whh, b_ih, b_hh, dcond, mask (or None)."""
    leaves = {k: inp[k].detach().to(dtype).clone().requires_grad_(True) for k in ("Xp", "whh", "b_ih", "b_hh")}
    mask = None if inp.get("mask") is None else inp["mask"].to(dtype)
    taps = []
    hseq, feats = windows_forward(leaves["Xp"], leaves["whh"], leaves["b_ih"], leaves["b_hh"], mask, dims, lstm, taps=taps)
    (feats * _dfeat(inp["dcond"].to(dtype), dims)).sum().backward()
    return {"features": feats.detach(), "hseq": hseq.detach(),
            "dgi": torch.stack([t[0].grad for t in taps]), "dgh": torch.stack([t[1].grad for t in taps]),
            "dXp": leaves["Xp"].grad, "dW_hh": leaves["whh"].grad, "db_ih": leaves["b_ih"].grad, "db_hh": leaves["b_hh"].grad}


# ---------------------------------------------------------------------------------------------- the arithmetic model
def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def _f16(x):
    return x.to(torch.float32).to(torch.float16).to(x.dtype)


def _split(x):
    """bf16 hi + lo of the fp32 value: hi = RNE(v), lo = RNE(v - hi)."""
    v = x.to(torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(x.dtype), lo.to(x.dtype)


def _prod3(a, b):
    """a @ b with both operands split: hi hi + hi lo + lo hi (the lo lo term, 2^-16 relative, is dropped)."""
    ah, al = _split(a)
    bh, bl = _split(b)
    return ah @ bh + ah @ bl + al @ bh


def _fast_sigmoid(x):
    """lfi_common.h's sigmoidf_: rcp(1 + exp2(-log2(e) x)), evaluated in fp32."""
    v = x.to(torch.float32)
    return (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * v))).to(x.dtype)


def _fast_tanh(x):
    """lfi_common.h's tanhf_: 1 - 2 rcp(1 + exp2(2 log2(e) x)) in fp32 - its error is an ulp of 1, not of the result."""
    v = x.to(torch.float32)
    return (1.0 - 2.0 * (1.0 / (1.0 + torch.exp2(2.8853900817779268 * v)))).to(x.dtype)


def dwhh_from_stashes(dgh, hseq):
    """dW_hh = dgh[1:]^T hseq[:-1] (lfi.h), in fp64."""
    G, hid = dgh.shape[-1], hseq.shape[-1]
    if dgh.shape[0] < 2:
        return torch.zeros(G, hid, dtype=torch.float64, device=dgh.device)
    return dgh[1:].double().reshape(-1, G).t() @ hseq[:-1].double().reshape(-1, hid)


def scatter_windows(dgi, mask, dims):
    """dXp[b T + p] = sum over the windows (n, s) that read row p of mask * dgi[s][n B + b]."""
    G = dgi.shape[-1]
    rows = window_rows(dims, dgi.device)
    out = torch.zeros(dims.B * dims.T, G, dtype=dgi.dtype, device=dgi.device)
    for s in range(dims.hist):
        term = dgi[s] if mask is None else mask[:, s].to(dgi.dtype).unsqueeze(1) * dgi[s]
        out.index_add_(0, rows[:, s], term)
    return out


def run_model(inp, dims, lstm=False, three_products=False, two_products=False, stash_f16=False, grads_bf16=False, bwd_exact=False,
              fast_gates=False):
    """The same recurrence in fp64 with a hand-written BPTT that applies ONLY the roundings the kernels document, each behind a flag:

    three_products  both operands of h W_hh^T and of dgh W_hh are split into bf16 hi + lo, summed as hi hi + hi lo + lo hi
                    (lfi_enc_desc.precision = 1; lfi_gemm_desc.precision = 1 on the unfused and LSTM loops)
    bwd_exact       with three_products: only the forward product is split, dgh W_hh is exact - the accumulator-layout backward
                    kernel "runs the exact-f32 ... kernel, whatever the engine's GEMM mode" (enc_plan_bwd in lfi_encoder_common.h)
    two_products    dgh W_hh takes the gate derivatives rounded to bf16 and the weights as hi + lo (lfi_enc_desc.bwd_two_products)
    stash_f16       r, z, n and W_hn h + b_hn are rounded to fp16 between forward and backward (lfi_enc_desc.stash_f16)
    grads_bf16      dgi and dgh are rounded to bf16 before the scatter and the dW_hh sum (lfi_encode_windows_grad_stash_bf16);
                    the bias gradients are summed from the unrounded values in the same pass (bsum in the fused kernels)
    fast_gates      sigmoid and tanh are lfi_common.h's default sigmoidf_ / tanhf_, fp32 expressions on exp2 and a reciprocal:
                    tanh = 1 - 2 / (1 + 2^(2 log2(e) x)) is good to an ulp of 1.0, i.e. absolutely, where libm's is good to an ulp
                    of the result - a few 1e-7 relative on |n| ~ 0.3, above what an fp32 run of the reference shows

    With every flag off this equals run_autograd(..., torch.float64)."""
    f64 = torch.float64
    Xp, whh, b_ih, b_hh = (inp[k].detach().to(f64) for k in ("Xp", "whh", "b_ih", "b_hh"))
    mask = None if inp.get("mask") is None else inp["mask"].to(f64)
    F, hid, hist = dims.N * dims.B, dims.hid, dims.hist
    rows = window_rows(dims, Xp.device)
    fwd_mm = _prod3 if three_products else torch.matmul
    sig, tanh = (_fast_sigmoid, _fast_tanh) if fast_gates else (torch.sigmoid, torch.tanh)
    if two_products:
        wh, wl = _split(whh)

        def bwd_mm(d, w):
            return _bf16(d) @ (wh + wl)
    elif three_products and not bwd_exact:
        bwd_mm = _prod3
    else:
        bwd_mm = torch.matmul
    h = Xp.new_zeros(F, hid)
    c = Xp.new_zeros(F, hid)
    hs, saved = [], []
    for s in range(hist):
        x = Xp[rows[:, s]]
        if mask is not None:
            x = mask[:, s].unsqueeze(1) * x
        gi = x + b_ih
        gh = fwd_mm(h, whh.t()) + b_hh
        if lstm:
            pre = gi + gh
            i, f, o = sig(pre[:, :hid]), sig(pre[:, hid:2 * hid]), sig(pre[:, 3 * hid:])
            g = tanh(pre[:, 2 * hid:3 * hid])
            cp, c = c, f * c + i * g
            h = o * tanh(c)
            saved.append((i, f, g, o, c, cp))
        else:
            r = sig(gi[:, :hid] + gh[:, :hid])
            z = sig(gi[:, hid:2 * hid] + gh[:, hid:2 * hid])
            ghn = gh[:, 2 * hid:]
            n = tanh(gi[:, 2 * hid:] + r * ghn)
            hp, h = h, (1.0 - z) * n + z * h
            saved.append(tuple(_f16(t) for t in (r, z, n, ghn)) + (hp,) if stash_f16 else (r, z, n, ghn, hp))
        hs.append(h)
    hseq = torch.stack(hs)
    feats = torch.cat([h, h], dim=1) if dims.dup else h
    d = _dfeat(inp["dcond"].to(f64), dims)
    dh = d[:, :hid] + d[:, hid:] if dims.dup else d.clone()
    dc = torch.zeros_like(dh)
    dgi, dgh = [None] * hist, [None] * hist
    for s in range(hist - 1, -1, -1):
        if lstm:
            i, f, g, o, c, cp = saved[s]
            tc = tanh(c)
            dc = dc + dh * o * (1.0 - tc * tc)
            dpre = torch.cat([dc * g * i * (1.0 - i), dc * cp * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], dim=1)
            dgi[s] = dgh[s] = dpre
            dc = dc * f
            dh = bwd_mm(dpre, whh)
        else:
            r, z, n, ghn, hp = saved[s]
            dan = dh * (1.0 - z) * (1.0 - n * n)
            daz = dh * (hp - n) * z * (1.0 - z)
            dar = dan * ghn * r * (1.0 - r)
            dgi[s] = torch.cat([dar, daz, dan], dim=1)
            dgh[s] = torch.cat([dar, daz, dan * r], dim=1)
            dh = dh * z + bwd_mm(dgh[s], whh)
    dgi, dgh = torch.stack(dgi), torch.stack(dgh)
    db_ih, db_hh = dgi.sum(dim=(0, 1)), dgh.sum(dim=(0, 1))
    if grads_bf16:
        dgi, dgh = _bf16(dgi), _bf16(dgh)
    return {"features": feats, "hseq": hseq, "dgi": dgi, "dgh": dgh, "dXp": scatter_windows(dgi, mask, dims),
            "dW_hh": dwhh_from_stashes(dgh, hseq), "db_ih": db_ih, "db_hh": db_hh}


# ---------------------------------------------------------------------------------------------- the comparison
def pieces(run, hid):
    """The separately measured parts of a run: features; hseq, dgi and dgh per history step; dXp; dW_hh per gate block; the biases."""
    out = [("features", run["features"])]
    for key in ("hseq", "dgi", "dgh"):
        out += [("%s[%d]" % (key, s), run[key][s]) for s in range(run[key].shape[0])]
    out.append(("dXp", run["dXp"]))
    out += [("dW_hh[%d]" % g, run["dW_hh"][g * hid:(g + 1) * hid]) for g in range(run["dW_hh"].shape[0] // hid)]
    out += [("db_ih", run["db_ih"]), ("db_hh", run["db_hh"])]
    return out


def compare(got, exact, model, fp32, hid):
    """-> rows (name, err, allowed, ok): err(got) <= MODEL_FACTOR * err(model) + F32_FACTOR * err(fp32), every error a rel_l2
    against `exact`. Both right-hand terms come from the reference alone. A part whose exact norm is 0 must be exactly 0."""
    rows = []
    for (name, g), (_, e), (_, m), (_, f) in zip(pieces(got, hid), pieces(exact, hid), pieces(model, hid), pieces(fp32, hid)):
        assert g.shape == e.shape, (name, tuple(g.shape), tuple(e.shape))
        err = rel_l2(g, e)
        allowed = MODEL_FACTOR * rel_l2(m, e) + F32_FACTOR * rel_l2(f, e)
        ok = bool(torch.isfinite(g).all()) and err <= allowed
        rows.append((name, err, allowed, ok))
    return rows


def failures(rows):
    return ["%s: %.3e > %.3e" % (n, e, a) for n, e, a, ok in rows if not ok]


def worst(rows):
    """(name, err, allowed) of the part closest to (or furthest past) its bound."""
    def ratio(r):
        return (r[1] / r[2]) if r[2] > 0 else (0.0 if r[1] == 0 else float("inf"))
    n, e, a, _ = max(rows, key=ratio)
    return n, e, a


def make_inputs(dims, lstm=False, masked=True, seed=0, ldcond=None, device="cpu"):
    """Inputs as the tilings test draws them: Xp and biases ~ 0.3 randn, W_hh ~ 0.06 randn, dcond ~ 0.3 randn,
    mask = Bernoulli(0.5) * 2 with at least one window fully masked. fp32 values (what the kernels are given)."""
    g = torch.Generator().manual_seed(seed)
    G = (4 if lstm else 3) * dims.hid
    F = dims.N * dims.B
    ldcond = ldcond or dims.col + dims.hid * (1 + dims.dup)

    def rnd(*s):
        return torch.randn(*s, generator=g) * 0.3
    inp = {"Xp": rnd(dims.B * dims.T, G), "whh": rnd(G, dims.hid) * 0.2, "b_ih": rnd(G), "b_hh": rnd(G), "dcond": rnd(F, ldcond)}
    mask = (torch.rand(F, dims.hist, generator=g) < 0.5).float() * 2
    mask[F // 2] = 0.0
    inp["mask"] = mask if masked else None
    return {k: (v.to(device) if v is not None else None) for k, v in inp.items()}
