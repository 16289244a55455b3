"""The teacher-forced flow of lfi_flow_seq_fwd / _bwd / lfi_flow_param_grads as include/lfi.h states it, in plain torch (any dtype, any
device): the definition the training walks and the thin weight-gradient products are compared with, an arithmetic model of their
documented roundings, and the comparison both the GPU tests and the planted-defect tests go through.

Written from glow/models.py / glow/modules.py as include/lfi.h cites them. Flow step k at timestep n, on the B rows x of that frame
(x = x0[:, start + n] for k = 0, the step below's output otherwise), with the recurrent state of step k carried from timestep n - 1
(zero at n = 0, init_rnn_hidden, glow/models.py:619):

    a  = (x + an_bias) * exp(an_logs)                         ActNorm2d, glow/modules.py:45-66; log-det C * sum(an_logs): the
                                                               reference scales it by x.size(1) == C
    y  = a @ W       W = P L U or the dense weight             InvertibleConv1x1, glow/modules.py:147-189; log-det C * log|det W|
    gi = gic[k][n] + z1 @ W_ih[:, :Ch]^T                       z1 = y[:, :Ch]; gic = W_ih[:, Ch:] c + b_ih is GIVEN (hoisted product)
    gh = h W_hh^T + b_hh                                       f_seq.forward, glow/models.py:204-214: GRUCell / LSTMCell equations
    GRU   r = s(gi_r + gh_r)  u = s(gi_z + gh_z)  n = tanh(gi_n + r * gh_n)  h' = (1 - u) n + u h
    LSTM  i, f, o = s(pre_i), s(pre_f), s(pre_o)  g = tanh(pre_g)  c' = f c + i g  h' = o tanh(c')   (pre = gi + gh)
    o  = (h' W_fl^T + b_fl) * exp(3 l_fl)                      LinearZeros, glow/modules.py:93-95
    affine    shift, scale = o[:, 0::2], sigmoid(o[:, 1::2] + 2).clamp(min = scale_eps)
              z2' = (z2 + shift) * scale, log-det sum(log scale)                         glow/models.py:332-341
    additive  z2' = z2 + o                                                               glow/models.py:330-331
    x_out = [z1 | z2']
    nll[n] = -(log-det + sum_c -0.5 (z_c^2 + log 2 pi)) / ln 2, z = x_out of the last step  glow/models.py:563-565

A run is a dict: z (N x B x C), nll (N x B), h (Ks x N x B x H), x_out (Ks x N x B x C), dgi / dgh (Ks x N x B x G: gradients of the
input-side pre-activation gi and of the hidden-side pre-activation W_hh h + b_hh, what the backward stash holds), dlin (gradient of
h' W_fl^T + b_fl), dx (Ks x N x B x C: gradient of the INPUT of step k; dx[0] is the frames' gradient) and grads, one tensor per
lfi_flow_grads array, for loss = gscale * sum(nll). grads["w_ih"][:, :, Ch:] is DEFINED as dgi[k]^T c[:, k D:(k + 1) D] for the given
c (F x Ks D), and grads["b_ih"] as the column sums of dgi: gic is a leaf here, as it is for the kernels.
"""
import math
from collections import namedtuple

import torch

from encoder_reference import (F32_FACTOR, MODEL_FACTOR, _bf16, _fast_sigmoid, _fast_tanh, _prod3, _split, failures,  # noqa: F401
                               worst)
from helpers import rel_l2

Dims = namedtuple("Dims", "B T N start C H D Ks affine lstm scale_eps")
LN2 = math.log(2.0)
LOG2PI = math.log(2.0 * math.pi)
MB = 16                     # rows per batch tile of the walks (lfi_flow_cells.h)
GRAD_KEYS = ("an_bias", "an_logs", "inv_l", "inv_u", "inv_logs", "inv_w", "w_ih", "w_hh", "b_ih", "b_hh", "w_fl", "b_fl", "l_fl")


def derived(d):
    """Ch, C2, Cout, NG, G, I as lfi.h derives them."""
    Ch = d.C // 2
    C2 = d.C - Ch
    NG = 4 if d.lstm else 3
    return Ch, C2, (2 * C2 if d.affine else C2), NG, NG * d.H, Ch + d.D


# ---- three seams the planted-defect tests replace (tests/test_flow_reference_cpu.py); the reference itself never changes them
def _carry(h, k, n):
    """The recurrent state step k hands from timestep n to n + 1."""
    return h


def _clamp_scale(s, eps):
    """sigmoid(. + 2).clamp(min=eps): no gradient through a clamped element."""
    return s.clamp(min=eps)


def _gru_candidate(gi_n, r, gh_n, b_n, tanh):
    """n = tanh(gi_n + r * gh_n), gh_n = W_hn h + b_hn: b_hn (b_n) sits INSIDE the product with r (torch.nn.GRUCell)."""
    return tanh(gi_n + r * gh_n)


class _FastSigmoid(torch.autograd.Function):
    """Value: sigmoidf_ of lfi_common.h. Derivative: s (1 - s) of that value - what the backward cells compute from the stash."""
    @staticmethod
    def forward(ctx, x):
        s = _fast_sigmoid(x)
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return g * s * (1.0 - s)


class _FastTanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        t = _fast_tanh(x)
        ctx.save_for_backward(t)
        return t

    @staticmethod
    def backward(ctx, g):
        t, = ctx.saved_tensors
        return g * (1.0 - t * t)


class _Product(torch.autograd.Function):
    """a (rows x K) @ w^T (w: J x K), forward and / or input gradient as three bf16 products. The weight gradient stays exact: the
    thin products are modelled on their own (_thin_products)."""
    @staticmethod
    def forward(ctx, a, w, fwd3, bwd3):
        ctx.save_for_backward(a, w)
        ctx.bwd3 = bwd3
        return _prod3(a, w.t()) if fwd3 else a @ w.t()

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        return (_prod3(g, w) if ctx.bwd3 else g @ w), g.t() @ a, None, None


def _invconv(par, k, dtype):
    """(W, log|det W|) of step k from the LU parameters or the dense weight."""
    if par.get("inv_w") is not None:
        w = par["inv_w"][k]
        return w, torch.slogdet(w)[1]
    C = par["inv_l"].shape[-1]
    lmask = torch.tril(torch.ones(C, C, dtype=dtype, device=par["inv_l"].device), -1)
    lm = par["inv_l"][k] * lmask + torch.eye(C, dtype=dtype, device=lmask.device)
    um = par["inv_u"][k] * lmask.t() + torch.diag(par["inv_sign"][k] * torch.exp(par["inv_logs"][k]))
    return par["inv_p"][k] @ (lm @ um), par["inv_logs"][k].sum()


def _run(inp, d, dtype, fast_gates=False, x3_fwd=False, x3_bwd=False, rows_bf16=False, two_products=False, three_products=False,
         w_fp32=False):
    Ch, C2, Cout, NG, G, I = derived(d)
    B, N, H, Ks, C = d.B, d.N, d.H, d.Ks, d.C
    F = N * B
    gscale = float(inp.get("gscale", 1.0))
    par = {}
    for key, v in inp["params"].items():
        if v is None:
            continue
        v = v.detach().to(dtype).clone()
        par[key] = v.requires_grad_(True) if key in GRAD_KEYS else v
    x0 = inp["x0"].detach().to(dtype).clone().requires_grad_(True)
    gic = inp["gic"].detach().to(dtype).clone().requires_grad_(True)
    assert x0.shape == (B, d.T, C) and gic.shape == (Ks, F, G) and 0 <= d.start and d.start + N <= d.T
    sig, tanh = (_FastSigmoid.apply, _FastTanh.apply) if fast_gates else (torch.sigmoid, torch.tanh)

    def mm(a, w, fwd3, bwd3):
        return _Product.apply(a, w, fwd3, bwd3) if (fwd3 or bwd3) else a @ w.t()

    Ws, lds = [], []
    for k in range(Ks):
        W, ld = _invconv(par, k, dtype)
        if w_fp32:      # the value is the fp32 product's, the gradient passes
            par32 = {key: (None if v is None else v.detach().to(torch.float32)) for key, v in par.items() if key.startswith("inv_")}
            W = W + (_invconv(par32, k, torch.float32)[0].to(dtype) - W.detach())
        W.retain_grad()
        Ws.append(W)
        lds.append(ld)
    const = sum(C * (par["an_logs"][k].sum() + lds[k]) for k in range(Ks))
    state = [[x0.new_zeros(B, H), x0.new_zeros(B, H)] for _ in range(Ks)]
    taps = [[None] * N for _ in range(Ks)]
    raw_scale = [[None] * N for _ in range(Ks)]
    nll = []
    for n in range(N):
        logdet = const
        x = x0[:, d.start + n]
        for k in range(Ks):
            x.retain_grad()
            xin = x
            a = (x + par["an_bias"][k]) * torch.exp(par["an_logs"][k])
            y = a @ Ws[k]
            z1, z2 = y[:, :Ch], y[:, Ch:]
            gi = gic[k, n * B:(n + 1) * B] + mm(z1, par["w_ih"][k][:, :Ch], x3_fwd, x3_bwd)
            hp, cp = state[k]
            gh = mm(hp, par["w_hh"][k], x3_fwd, x3_bwd) + par["b_hh"][k]
            if d.lstm:
                pre = gi + gh
                pre.retain_grad()
                tgi = tgh = pre
                i_, f_, o_ = sig(pre[:, :H]), sig(pre[:, H:2 * H]), sig(pre[:, 3 * H:])
                g_ = tanh(pre[:, 2 * H:3 * H])
                cn = f_ * cp + i_ * g_
                h = o_ * tanh(cn)
                state[k][1] = _carry(cn, k, n)
            else:
                gi.retain_grad()
                gh.retain_grad()
                tgi, tgh = gi, gh
                r = sig(gi[:, :H] + gh[:, :H])
                u = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
                cand = _gru_candidate(gi[:, 2 * H:], r, gh[:, 2 * H:], par["b_hh"][k][2 * H:], tanh)
                h = (1.0 - u) * cand + u * hp
            state[k][0] = _carry(h, k, n)
            lin = mm(h, par["w_fl"][k], False, x3_bwd) + par["b_fl"][k]
            lin.retain_grad()
            o = lin * torch.exp(3.0 * par["l_fl"][k])
            if d.affine:
                s = sig(o[:, 1::2] + 2.0)
                raw_scale[k][n] = s.detach()
                scale = _clamp_scale(s, d.scale_eps)
                z2 = (z2 + o[:, 0::2]) * scale
                logdet = logdet + torch.log(scale).sum(dim=1)
            else:
                z2 = z2 + o
            y.retain_grad()
            x = torch.cat([z1, z2], dim=1)
            taps[k][n] = dict(x=xin, a=a, y=y, h=h, gi=tgi, gh=tgh, lin=lin, out=x)
        nll.append(-(logdet + (-0.5 * (x ** 2 + LOG2PI)).sum(dim=1)) / LN2)
    nll = torch.stack(nll)
    (gscale * nll.sum()).backward(retain_graph=rows_bf16 or two_products or three_products)    # (_thin_products walks W's graph again)

    def grid(key, grad):
        return torch.stack([torch.stack([(taps[k][n][key].grad if grad else taps[k][n][key].detach()) for n in range(N)])
                            for k in range(Ks)])
    run = {"nll": nll.detach(), "h": grid("h", False), "x_out": grid("out", False), "dlin": grid("lin", True),
           "dgi": grid("gi", True), "dgh": grid("gh", True), "dx": grid("x", True), "a": grid("a", False), "y": grid("y", False),
           "dy": grid("y", True)}
    run["z"] = run["x_out"][Ks - 1]
    run["raw_scale"] = None if not d.affine else torch.stack([torch.stack(raw_scale[k]) for k in range(Ks)])
    grads = {k: par[k].grad for k in GRAD_KEYS if k in par and k not in ("w_ih", "b_ih")}
    dgi_f = run["dgi"].reshape(Ks, F, G)
    grads["b_ih"] = dgi_f.sum(dim=1)
    cmat = inp["c"].detach().to(dtype)
    w_ih = torch.cat([par["w_ih"].grad[:, :, :Ch], torch.stack([dgi_f[k].t() @ cmat[:, k * d.D:(k + 1) * d.D] for k in range(Ks)])],
                     dim=2)
    grads["w_ih"] = w_ih
    if rows_bf16:
        # lfi_flow.hip, backward walk Q1: "rounded as the products' operand split rounds its hi part: to nearest even" - the rows
        # go out as bf16 while the bias sums (bsi / bsh) take the unrounded values in the same loop
        run["dgi"], run["dgh"] = _bf16(run["dgi"]), _bf16(run["dgh"])
    if rows_bf16 or two_products or three_products:
        _thin_products(run, grads, par, Ws, lds, cmat, d, gscale, two_products, three_products)
    run["grads"] = grads
    return run


def _thin_products(run, grads, par, Ws, lds, cmat, d, gscale, two, three):
    """The weight gradients that lfi_flow_param_grads takes as products over the F frames, from the (rounded) rows of the run:
    w_fl = dlin^T h, w_hh = dgh[n >= 1]^T h[n - 1], w_ih[:, :Ch] = dgi^T z1, w_ih[:, Ch:] = dgi^T c, dW = a^T dy -> the 1x1
    convolution's parameters. A is the operand named first."""
    Ch, C2, Cout, NG, G, I = derived(d)
    B, N, H, Ks, C = d.B, d.N, d.H, d.Ks, d.C
    F = N * B

    def prod(A, Bm):
        if two:
            # lfi.h, lfi_gemm_desc.precision: "Bits 8 / 9 (0x100 / 0x200) DROP the a_lo * b_hi / a_hi * b_lo product": with 0x100
            # what is left is a_hi (b_hi + b_lo) - A rounded to bf16; lfi_wgrad.hip: "two products each (a_hi b_lo + a_hi b_hi)"
            bh, bl = _split(Bm)
            return _bf16(A).t() @ bh + _bf16(A).t() @ bl
        if three:
            # lfi.h, lfi_gemm_desc.precision 1: "operands split into bf16 hi + lo on the fly, three bf16 MFMAs per step"
            return _prod3(A.t(), Bm)
        return A.t() @ Bm
    h, dgi, dgh, dlin = (run[k].reshape(Ks, F, -1) for k in ("h", "dgi", "dgh", "dlin"))
    a, y, dy = (run[k].reshape(Ks, F, C) for k in ("a", "y", "dy"))
    if two or three:
        grads["w_fl"] = torch.stack([prod(dlin[k], h[k]) for k in range(Ks)])
    grads["w_hh"] = torch.stack([prod(dgh[k][B:], h[k][:F - B]) if N > 1 else torch.zeros_like(par["w_hh"][k]) for k in range(Ks)])
    grads["w_ih"] = torch.stack([torch.cat([prod(dgi[k], y[k][:, :Ch]), prod(dgi[k], cmat[:, k * d.D:(k + 1) * d.D])], dim=1)
                                 for k in range(Ks)])
    if not (two or three):      # rounded rows alone touch the two products that read them
        return
    # the 1x1 convolution: its parameters' gradients are the chain rule through W = P L U (or W itself) of dW, plus the constant
    # log-det term -gscale F C / ln 2 * d log|det W|
    keys = [k for k in ("inv_l", "inv_u", "inv_logs", "inv_w") if k in par]
    dW = [prod(a[k], dy[k]) for k in range(Ks)]
    obj = sum((Ws[k] * dW[k]).sum() - (gscale * F * C / LN2) * lds[k] for k in range(Ks))
    for key, g in zip(keys, torch.autograd.grad(obj, [par[k] for k in keys], allow_unused=True)):
        grads[key] = g if g is not None else torch.zeros_like(par[key])


def run_autograd(inp, d, dtype=torch.float64):
    """The reference run in `dtype` with autograd: fp64 is the exact reference, fp32 the second term of the bound.
    inp: dict x0 (B x T x C), gic (Ks x F x G), c (F x Ks D), gscale, params {lfi_flow_params name: (Ks x ...) tensor}."""
    return _run(inp, d, dtype)


def run_model(inp, d, **flags):
    """The same computation in fp64 with ONLY the roundings the kernels document, each behind a flag:

    fast_gates      sigmoid and tanh - the cells' gates and the coupling's sigmoid(. + 2) - are lfi_common.h's sigmoidf_ / tanhf_:
                    "Gate non-linearities on the hardware transcendental units (v_exp_f32 = 2^x, v_rcp_f32; ~1 ulp each) ...
                    Absolute error ~1e-7 on values in (-1, 1)"; the backward cells differentiate the stashed values
    x3_fwd          z1 W_ih[:, :Ch]^T and h W_hh^T as three bf16 products (flow_pipe_fwd_kernel<3, true>; lfi_flow_cells.h:
                    "forward walk: its products contract over h (H16) and over z1 (Ch16)"). LinearZeros and the 1x1 convolution
                    keep the f32 MFMA
    x3_bwd          dlin W_fl, dgh W_hh and dgi W_ih[:, :Ch] as three bf16 products (flow_pipe_bwd_kernel<3, true>: "Q1's bf16 x 3
                    operand", "bf16 x 3 form: pre-split 32-k fragments (flow_prep_x3_kernel)")
    rows_bf16       dgi | dgh leave the walk as bf16, to nearest even (lfi.h, gemm_precision bit 16); b_ih / b_hh are summed from
                    the unrounded values
    two_products    the thin products with their A operand rounded to bf16 and B as hi + lo (skip bit 0x100; lfi_wgrad.hip)
    three_products  the thin products as lfi_gemm_f32 at precision 1
    w_fp32          W = P L U is built in fp32 (lfi_flow.hip, flow_prep_invconv_kernel: "T = Lm Um", "W = P T" with float sums; lfi.h:
                    "W [Ks][C][C]" floats); its log-det stays exact (that kernel sums it in fp64)

    With every flag off this IS run_autograd(inp, d, torch.float64)."""
    return _run(inp, d, torch.float64, **flags)


# ---------------------------------------------------------------------------------------------- the comparison
def tail_start(B):
    """First row of the last batch tile when there is more than one tile, else None."""
    t = MB * ((B - 1) // MB)
    return t if t > 0 else None


def pieces(run, d):
    """The separately measured parts: z, x_out, h, dgi, dgh per (flow step, timestep); nll and dx[0] per timestep (dx[k >= 1] per
    cell as well); every parameter gradient per flow step, w_hh / b_ih / b_hh also per gate block, w_ih as [:, :Ch] and [:, Ch:];
    the rows of the last batch tile of z and dgi once more on their own."""
    Ch, C2, Cout, NG, G, I = derived(d)
    H, Ks, N = d.H, d.Ks, d.N
    tb = tail_start(d.B)
    out = []
    for n in range(N):
        out.append(("z[%d]" % n, run["z"][n]))
        out.append(("nll[%d]" % n, run["nll"][n]))
        if tb is not None:
            out.append(("z.tail[%d]" % n, run["z"][n, tb:]))
    for k in range(Ks):
        for n in range(N):
            for key in ("x_out", "h", "dgi", "dgh", "dx"):
                out.append(("%s[%d][%d]" % (key, k, n), run[key][k, n]))
            if tb is not None:
                out.append(("dgi.tail[%d][%d]" % (k, n), run["dgi"][k, n, tb:]))
    g = run["grads"]
    for k in range(Ks):
        for key in GRAD_KEYS:
            if key not in g or g[key] is None:
                continue
            t = g[key][k]
            if key == "w_ih":
                out.append(("w_ih[%d][:, :Ch]" % k, t[:, :Ch]))
                out.append(("w_ih[%d][:, Ch:]" % k, t[:, Ch:]))
                continue
            out.append(("%s[%d]" % (key, k), t))
            if key in ("w_hh", "b_ih", "b_hh"):
                out += [("%s[%d].gate%d" % (key, k, j), t[j * H:(j + 1) * H]) for j in range(NG)]
    return out


def compare(got, exact, model, fp32, d, skip=()):
    """-> rows (name, err, allowed, ok): err(got) <= MODEL_FACTOR * err(model) + F32_FACTOR * err(fp32), every error a rel_l2 against
    `exact` with no floor. A part whose exact norm is 0 must be exactly 0; non-finite values fail. skip: substrings of the names of parts that
    `got` does not hold (named by the caller, case by case)."""
    rows = []
    for (name, g), (_, e), (_, m), (_, f) in zip(pieces(got, d), pieces(exact, d), pieces(model, d), pieces(fp32, d)):
        if any(s in name for s in skip):
            continue
        assert g.shape == e.shape, (name, tuple(g.shape), tuple(e.shape))
        err = rel_l2(g, e)
        allowed = MODEL_FACTOR * rel_l2(m, e) + F32_FACTOR * rel_l2(f, e)
        ok = bool(torch.isfinite(g).all()) and err <= allowed
        rows.append((name, err, allowed, ok))
    return rows


CLAMP_EPS = 0.84375         # Glow.scale_eps of the clamp cases (exact in fp32): sigmoid(2) = 0.88 is where an untrained coupling sits
EPS = 2.0 ** -13            # ... and of every other case: 1.2e-4, final_model.yaml's 1e-4 as a value fp32 holds exactly


def make_inputs(d, dense=False, seed=0, device="cpu", gscale=None, clamp=False):
    """Parameters at trained-model scale (LinearZeros NOT at zero: that would switch the coupling off), frames ~ randn, gic and c
    random and independent of each other. fp32 values - what the kernels are given."""
    Ch, C2, Cout, NG, G, I = derived(d)
    g = torch.Generator().manual_seed(seed)
    B, C, H, Ks, F = d.B, d.C, d.H, d.Ks, d.N * d.B

    def rnd(*s, scale=1.0):
        return torch.randn(*s, generator=g) * scale
    par = {"an_bias": rnd(Ks, C, scale=0.2), "an_logs": rnd(Ks, C, scale=0.1),
           "w_ih": rnd(Ks, G, I, scale=1.0 / math.sqrt(I)), "w_hh": rnd(Ks, G, H, scale=1.0 / math.sqrt(H)),
           "b_ih": rnd(Ks, G, scale=0.1), "b_hh": rnd(Ks, G, scale=0.3),
           "w_fl": rnd(Ks, Cout, H, scale=1.0 / math.sqrt(H)), "b_fl": rnd(Ks, Cout, scale=0.3), "l_fl": rnd(Ks, Cout, scale=0.1)}
    if clamp:
        # the clamp cases: the scale columns of LinearZeros sit at +-2.5, so sigmoid(. + 2) is either well above or well below
        # CLAMP_EPS and no element comes within 1e-3 of it (checked on the fp64 run by tests/test_flow_reference_cpu.py)
        assert d.affine
        par["b_fl"][:, 1::2] = torch.where(torch.rand(Ks, Cout // 2, generator=g) < 0.5, -2.5, 2.5) + rnd(Ks, Cout // 2, scale=0.1)
    q, _ = torch.linalg.qr(rnd(Ks, C, C).double())
    w = (q + 0.05 * rnd(Ks, C, C).double())
    if dense:
        par["inv_w"] = w.float()
    else:
        p, l, u = torch.linalg.lu(w)
        s = torch.diagonal(u, dim1=1, dim2=2)
        par.update(inv_p=p.float(), inv_l=l.float(), inv_u=torch.triu(u, 1).float(), inv_logs=torch.log(s.abs()).float(),
                   inv_sign=torch.sign(s).float())
    inp = {"x0": rnd(B, d.T, C), "gic": rnd(Ks, F, G, scale=0.5), "c": rnd(F, Ks * d.D, scale=0.5).clamp(min=-0.05),
           "gscale": (1.0 / F) if gscale is None else gscale, "params": {k: v.to(device) for k, v in par.items()}}
    for k in ("x0", "gic", "c"):
        inp[k] = inp[k].to(device)
    return inp
