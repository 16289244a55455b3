"""tests/flow_reference.py checked on the CPU: the reference against the oracle's flow_forward + nll_bits walked over timesteps with a
carried state (and autograd through that walk), the arithmetic model flag by flag, the comparison of the GPU flow-walk tests against
planted defects - the evidence that its bounds would notice a subtly wrong kernel - the input conditions of the clamp cases, and
lfi_flow_walk_variant against a table written from the dispatch rules. (FlowStep.normal_flow, glow/models.py:311-342.)"""
import ctypes as C
import math

import pytest
import torch

import flow_reference as fr
import test_gpu_flow_walks as gw
from flow_reference import Dims
from helpers import rel_l2
from oracle import seqglow_oracle as oracle


def _errs(run, exact, d):
    return {n: rel_l2(a, b) for (n, a), (_, b) in zip(fr.pieces(run, d), fr.pieces(exact, d))}


# ------------------------------------------------------------------------------------------ (a) the oracle
@pytest.mark.parametrize("C_,H,lstm,affine,dense", [(7, 6, 0, 1, 0), (6, 5, 1, 0, 1), (5, 4, 0, 0, 0), (9, 6, 1, 1, 1), (2, 3, 0, 1, 0)])
def test_reference_is_the_oracle_walked_over_timesteps(C_, H, lstm, affine, dense):
    """z, nll and every gradient against oracle.flow_forward / nll_bits looped over N timesteps with one carried state, in fp64. gic and
    c are made consistent here (c = LeakyReLU(cond_transform(cond)), gic = c W_ih[:, Ch:]^T + b_ih), so the oracle's autograd gives
    the whole of w_ih and b_ih."""
    d = Dims(5, 9, 4, 3, C_, H, 3, 2, affine, lstm, 0.88 if affine else 1e-4)
    Ch, C2, Cout, NG, G, I = fr.derived(d)
    inp = fr.make_inputs(d, dense=bool(dense), seed=21)
    g = torch.Generator().manual_seed(5)
    E, F = 4, d.N * d.B
    par = {k: v.double() for k, v in inp["params"].items()}
    cond = torch.randn(d.N, d.B, E, generator=g, dtype=torch.float64)
    wct, bct = torch.randn(d.Ks, d.D, E, generator=g, dtype=torch.float64) * 0.5, torch.randn(d.Ks, d.D, generator=g, dtype=torch.float64) * 0.2
    cs = [torch.nn.functional.leaky_relu(cond.reshape(F, E) @ wct[k].t() + bct[k], 0.01) for k in range(d.Ks)]
    inp["c"] = torch.cat(cs, dim=1)
    inp["gic"] = torch.stack([cs[k] @ par["w_ih"][k][:, Ch:].t() + par["b_ih"][k] for k in range(d.Ks)])
    ours = fr.run_autograd(inp, d, torch.float64)
    if affine:
        clamped = float((ours["raw_scale"] < d.scale_eps).double().mean())
        assert 0.05 < clamped < 0.95, clamped        # the clamp and its gradient are part of what is compared

    hp = {"Glow": {"K": d.Ks, "L": 1, "scale_eps": d.scale_eps, "rnn_type": "lstm" if lstm else "gru",
                   "flow_coupling": "affine" if affine else "additive"}}
    names = {"an_bias": "actnorm.bias", "an_logs": "actnorm.logs", "inv_l": "invconv.l", "inv_u": "invconv.u", "inv_logs": "invconv.log_s",
             "inv_p": "invconv.p", "inv_sign": "invconv.sign_s", "inv_w": "invconv.weight", "w_ih": "f.rnn.weight_ih",
             "w_hh": "f.rnn.weight_hh", "b_ih": "f.rnn.bias_ih", "b_hh": "f.rnn.bias_hh", "w_fl": "f.final_linear.weight",
             "b_fl": "f.final_linear.bias", "l_fl": "f.final_linear.logs"}
    sd, leaves = {}, {}
    for key, t in par.items():
        leaves[key] = [t[k].clone().requires_grad_(key in fr.GRAD_KEYS) for k in range(d.Ks)]
        for k in range(d.Ks):
            sd["glow.flow.layers.%d.%s" % (k, names[key])] = leaves[key][k]
    for k in range(d.Ks):
        sd["glow.flow.layers.%d.f.cond_transform.0.weight" % k] = wct[k]
        sd["glow.flow.layers.%d.f.cond_transform.0.bias" % k] = bct[k]
    x0 = inp["x0"].double()
    state = oracle._new_state(hp)
    zs, nlls = [], []
    for n in range(d.N):
        z, logdet, _ = oracle.flow_forward(hp, sd, x0[:, d.start + n], cond[n], state)
        zs.append(z)
        nlls.append(oracle.nll_bits(logdet, z))
    (inp["gscale"] * torch.stack(nlls).sum()).backward()
    assert rel_l2(ours["z"], torch.stack(zs).detach()) < 1e-12 and rel_l2(ours["nll"], torch.stack(nlls).detach()) < 1e-12
    for key, t in ours["grads"].items():
        want = torch.stack([leaf.grad for leaf in leaves[key]])
        assert rel_l2(t, want) < 1e-10, key
    if d.N > 1:
        assert float(ours["grads"]["w_hh"].abs().max()) > 0


# ------------------------------------------------------------------------------------------ (b) the model's flags
FLAG_DIMS = Dims(5, 9, 4, 2, 7, 6, 3, 2, 1, 0, 1e-4)


@pytest.fixture(scope="module")
def flag_runs():
    inp = fr.make_inputs(FLAG_DIMS, seed=1)
    return inp, fr.run_autograd(inp, FLAG_DIMS)


@pytest.mark.parametrize("lstm,affine,dense", [(0, 1, 0), (1, 0, 1)])
def test_model_without_flags_is_the_reference_bit_for_bit(lstm, affine, dense):
    d = FLAG_DIMS._replace(lstm=lstm, affine=affine)
    inp = fr.make_inputs(d, dense=bool(dense), seed=3)
    exact, model = fr.run_autograd(inp, d), fr.run_model(inp, d)
    for (name, m), (_, e) in zip(fr.pieces(model, d), fr.pieces(exact, d)):
        assert torch.equal(m, e), name


def test_model_flags_round_what_they_say(flag_runs):
    """Each flag alone: the parts it cannot touch stay exactly as they were, the others move by about the precision it names."""
    inp, exact = flag_runs
    d = FLAG_DIMS
    fwd = ("z[3]", "nll[3]", "h[0][0]", "h[1][3]", "x_out[0][2]")
    bwd = ("dgi[1][0]", "dgh[0][3]", "dx[0][0]", "dx[1][2]")
    thin = ("w_fl[0]", "w_hh[1]", "w_hh[0].gate2", "w_ih[0][:, :Ch]", "w_ih[1][:, Ch:]", "inv_l[0]", "inv_u[1]", "inv_logs[1]")
    sums = ("b_ih[0]", "b_hh[1]", "b_fl[0]", "l_fl[0]", "an_logs[0]", "an_bias[1]")

    def run(**flags):
        return _errs(fr.run_model(inp, d, **flags), exact, d)
    e = run(fast_gates=True)                    # fp32 expressions: an ulp of 1.0 on every gate
    assert all(1e-9 < e[k] < 2e-6 for k in fwd + bwd + thin + sums), e
    e = run(w_fp32=True)                        # 2^-24 on W
    assert all(0 < e[k] < 3e-7 for k in fwd + bwd + thin + sums), e
    e = run(x3_fwd=True)                        # 2^-16 per product, forward and everything behind it
    assert all(2e-8 < e[k] < 5e-5 for k in fwd + bwd + thin + sums), e      # (an_logs: mostly the constant log-det term)
    e = run(x3_bwd=True)                       # the forward pass is untouched
    assert all(e[k] == 0.0 for k in fwd) and all(2e-8 < e[k] < 5e-5 for k in bwd + thin), e
    e = run(rows_bf16=True)                     # 2^-9 on the rows and the two products that read them; the sums see unrounded values
    assert all(e[k] == 0.0 for k in fwd + sums + ("dx[0][0]", "w_fl[0]", "inv_l[0]", "inv_logs[1]")), e
    assert all(1e-4 < e[k] < 4e-3 for k in ("dgi[1][0]", "dgh[0][3]", "w_hh[1]", "w_ih[0][:, :Ch]", "w_ih[1][:, Ch:]")), e
    e = run(two_products=True)                  # A rounded to bf16 in every thin product, nothing else
    assert all(e[k] == 0.0 for k in fwd + bwd + sums) and all(5e-5 < e[k] < 4e-3 for k in thin), e
    e = run(three_products=True)                # 2^-16
    assert all(e[k] == 0.0 for k in fwd + bwd + sums) and all(1e-7 < e[k] < 5e-5 for k in thin), e


# ------------------------------------------------------------------------------------------ (c) every GPU case, clean
_case_refs = {}


def _case_runs(c):
    d = gw.ref_dims(c)
    key = (d, c.dense, c.clamp)
    if key not in _case_refs:
        inp = fr.make_inputs(d, dense=bool(c.dense), seed=gw.SEED, clamp=bool(c.clamp))
        _case_refs[key] = {"inp": inp, "exact": fr.run_autograd(inp, d), "fp32": fr.run_autograd(inp, d, torch.float32), "models": {}}
    ref = _case_refs[key]
    return d, ref, gw._model(ref, d, gw.model_flags(c))


@pytest.mark.parametrize("c", gw.CASES, ids=[c.id for c in gw.CASES])
def test_clean_run_passes(c):
    """The fp32 reference handed to the comparison as if it were the case's kernels: it passes, and no part that has a value is
    allowed nothing."""
    d, ref, model = _case_runs(c)
    rows = fr.compare(ref["fp32"], ref["exact"], model, ref["fp32"], d)
    assert not fr.failures(rows), fr.failures(rows)
    exact = dict(fr.pieces(ref["exact"], d))
    for name, e, a, ok in rows:
        assert (a > 0) == (float(exact[name].abs().max()) > 0), name
    if c.N == 1:
        assert any(n.startswith("w_hh") and a == 0 for n, e, a, ok in rows)
    # the allowances are of the size of the arithmetic - fp32, 2^-16 products, bf16 rows - nothing like a fixed 1e-3 gate
    worst_allowed = max(a for n, e, a, ok in rows)
    assert worst_allowed < (2e-2 if (c.g16 or c.two) else 2e-3), worst_allowed


# ------------------------------------------------------------------------------------------ (d) planted defects
SMALL = Dims(17, 8, 4, 1, 6, 8, 3, 2, 1, 0, 1e-4)               # one full batch tile and a one-row tile
SPLIT = Dims(16, 16, 13, 0, 6, 8, 3, 2, 1, 0, 1e-4)              # 13 timesteps: ranges of 7 + 6
CLAMPED = SMALL._replace(scale_eps=fr.CLAMP_EPS)
X3 = dict(fast_gates=True, w_fp32=True, x3_fwd=True, x3_bwd=True, three_products=True)


def _fp32(inp, d):
    return fr.run_autograd(inp, d, torch.float32)


def _edit(run, **parts):
    run = dict(run, grads=dict(run["grads"]))
    for k, v in parts.items():
        (run["grads"] if k in fr.GRAD_KEYS else run)[k] = v
    return run


def _stale_row(run, inp, d, mp):
    z, dgi = run["z"].clone(), run["dgi"].clone()
    z[2, d.B - 1] = 0.0
    dgi[1, 2, d.B - 1] = 0.0
    return _edit(run, z=z, dgi=dgi)


def _hprev_zero(run, inp, d, mp):
    mp.setattr(fr, "_carry", lambda h, k, n: torch.zeros_like(h) if n == 0 else h)
    return _fp32(inp, d)


def _h_of_step_below(run, inp, d, mp):
    h = run["h"].clone()
    h[1] = h[0]
    return _edit(run, h=h)


def _lo_hi_dropped(run, inp, d, mp):
    def two(a, b):
        ah, al = fr._split(a)
        bh, bl = fr._split(b)
        return ah @ bh + ah @ bl
    mp.setattr(fr, "_prod3", two)
    return fr.run_model(inp, d, **X3)


def _clamp_passes_gradient(run, inp, d, mp):
    mp.setattr(fr, "_clamp_scale", lambda s, eps: s + (s.clamp(min=eps) - s).detach())
    return _fp32(inp, d)


def _exp_logs(run, inp, d, mp):
    return _edit(run, l_fl=run["grads"]["l_fl"] * torch.exp(-2.0 * inp["params"]["l_fl"]))


def _logdet_once(run, inp, d, mp):
    return _edit(run, an_logs=run["grads"]["an_logs"] + float(inp["gscale"]) * d.N * d.B * (d.C - 1) / fr.LN2)


def _whh_with_timestep0(run, inp, d, mp):
    extra = torch.stack([run["dgh"][k, 0].t() @ run["h"][k, 0] for k in range(d.Ks)])
    return _edit(run, w_hh=run["grads"]["w_hh"] + extra)


def _bhn_outside(run, inp, d, mp):
    mp.setattr(fr, "_gru_candidate", lambda gi_n, r, gh_n, b_n, tanh: tanh(gi_n + r * (gh_n - b_n) + b_n))
    return _fp32(inp, d)


def _range_loses_its_last_timestep(run, inp, d, mp):
    n = 6       # the last timestep of the first range of 7
    return _edit(run, w_fl=run["grads"]["w_fl"] - torch.stack([run["dlin"][k, n].t() @ run["h"][k, n] for k in range(d.Ks)]),
                 w_hh=run["grads"]["w_hh"] - torch.stack([run["dgh"][k, n].t() @ run["h"][k, n - 1] for k in range(d.Ks)]))


class _Leak(torch.autograd.Function):
    """The carried state with a backward that picks up something from columns that should contribute nothing."""
    @staticmethod
    def forward(ctx, h):
        return h.clone()

    @staticmethod
    def backward(ctx, g):
        return g + 1e-3 * g.abs().mean()


def _padding_contributes(run, inp, d, mp):
    mp.setattr(fr, "_carry", lambda h, k, n: _Leak.apply(h))
    return fr.run_model(inp, d, **X3)


# name -> (dims, clamp inputs, model flags of the case it belongs to, plant, parts that must fail)
DEFECTS = {
    "one row of the last batch tile left stale": (SMALL, 0, {}, _stale_row, ("z.tail[2]", "dgi.tail[1][2]")),
    "h_prev of timestep 1 taken from zero": (SMALL, 0, {}, _hprev_zero, ("h[0][1]", "w_hh[0]")),
    "h of flow step 1 read from step 0": (SMALL, 0, {}, _h_of_step_below, ("h[1][0]",)),
    "lo x hi product dropped from a three-product run": (SMALL, 0, X3, _lo_hi_dropped, ("h[0][0]", "dgi[0][0]")),
    "clamp's gradient not zeroed": (CLAMPED, 1, {}, _clamp_passes_gradient, ("dgi[1][3]", "b_fl[1]")),
    "exp(logs) for exp(3 logs) in l_fl's gradient": (SMALL, 0, {}, _exp_logs, ("l_fl[0]", "l_fl[1]")),
    "log-det constant counted once in an_logs' gradient": (SMALL, 0, {}, _logdet_once, ("an_logs[0]", "an_logs[1]")),
    "w_hh's sum includes timestep 0": (SMALL, 0, {}, _whh_with_timestep0, ("w_hh[0]", "w_hh[1].gate2")),
    "n gate with b_hn outside r * (.)": (SMALL, 0, {}, _bhn_outside, ("h[0][0]", "b_hh[0].gate2")),
    "a timestep range drops its last timestep": (SPLIT, 0, {}, _range_loses_its_last_timestep, ("w_fl[0]", "w_hh[1]")),
    "padding hidden units contribute to dh_prev": (SMALL._replace(H=7), 0, X3, _padding_contributes, ("dgh[0][0]", "dgi[1][2]")),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defect_is_rejected(name, monkeypatch):
    d, clamp, flags, plant, where = DEFECTS[name]
    inp = fr.make_inputs(d, seed=9, clamp=bool(clamp))
    exact, fp32, model = fr.run_autograd(inp, d), _fp32(inp, d), fr.run_model(inp, d, **flags)
    clean = fr.run_model(inp, d, **flags) if flags else fp32
    assert not fr.failures(fr.compare(clean, exact, model, fp32, d))
    if clamp:
        frac = float((exact["raw_scale"] < d.scale_eps).double().mean())
        assert 0.2 < frac < 0.8
    bad = plant(clean, inp, d, monkeypatch)
    monkeypatch.undo()
    rows = fr.compare(bad, exact, model, fp32, d)
    failed = {n for n, e, a, ok in rows if not ok}
    assert failed, "the defect went unnoticed: " + name
    for part in where:
        assert part in failed, (name, part, sorted(failed))
    n, e, a = fr.worst(rows)
    print("%s: %s %.2e against %.2e allowed" % (name, n, e, a))
    assert e > 10 * a, (name, n, e, a)      # rejected by a margin, not by noise


def test_accumulate_that_overwrites_is_rejected():
    d = SMALL
    inp = fr.make_inputs(d, seed=9)
    exact, fp32, model = fr.run_autograd(inp, d), _fp32(inp, d), fr.run_model(inp, d)
    g = torch.Generator().manual_seed(2)
    pre = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) * float(v.pow(2).mean().sqrt()) for k, v in exact["grads"].items()}

    def shifted(run):
        return dict(run, grads={k: v + pre[k].to(v.dtype) for k, v in run["grads"].items()})
    assert not fr.failures(fr.compare(shifted(fp32), shifted(exact), shifted(model), shifted(fp32), d))
    failed = {n for n, e, a, ok in fr.compare(fp32, shifted(exact), shifted(model), shifted(fp32), d) if not ok}
    for k in exact["grads"]:
        assert k + "[0]" in failed or k + "[0][:, :Ch]" in failed, k


def test_bound_rejects_nonfinite_and_nonzero_where_zero_is_exact():
    d = SMALL._replace(N=1, T=5)          # N = 1: w_hh is exactly 0
    inp = fr.make_inputs(d, seed=1)
    exact, fp32, model = fr.run_autograd(inp, d), _fp32(inp, d), fr.run_model(inp, d)
    assert float(exact["grads"]["w_hh"].abs().max()) == 0.0
    assert not fr.failures(fr.compare(fp32, exact, model, fp32, d))
    w = fp32["grads"]["w_hh"].clone()
    w[1, 9, 2] = 1e-30
    failed = {n for n, e, a, ok in fr.compare(_edit(fp32, w_hh=w), exact, model, fp32, d) if not ok}
    assert "w_hh[1]" in failed and "w_hh[1].gate1" in failed and "w_hh[0]" not in failed
    z = fp32["z"].clone()
    z[0, 3, 1] = float("nan")
    assert "z[0]" in {n for n, e, a, ok in fr.compare(_edit(fp32, z=z), exact, model, fp32, d) if not ok}


# ------------------------------------------------------------------------------------------ (e) the clamp cases' inputs
@pytest.mark.parametrize("cid", ["clamp", "clamp-x3"])
def test_clamp_cases_clamp_one_well_separated_set(cid):
    c = next(x for x in gw.CASES if x.id == cid)
    d, ref, model = _case_runs(c)
    assert d.scale_eps == fr.CLAMP_EPS
    s = ref["exact"]["raw_scale"]
    frac = float((s < d.scale_eps).double().mean())
    assert 0.2 <= frac <= 0.8, frac
    assert float((s - d.scale_eps).abs().min()) >= 1e-3      # the kernels' forward error is orders below: they clamp the same set
    for run in (ref["fp32"], model):
        assert torch.equal(run["raw_scale"] < d.scale_eps, s < d.scale_eps)


# ------------------------------------------------------------------------------------------ (f) which kernels a call takes
SWITCH_OFF = {"pipe0": {"LFI_FLOW_PIPE": "0"}, "x3off": {"LFI_PIPE_X3": "0"}, "generic": {"LFI_FLOW_GENERIC": "1"},
              "fused0": {"LFI_FLOW_WGRAD_FUSED": "0"}, "generic+pipe0": {"LFI_FLOW_GENERIC": "1", "LFI_FLOW_PIPE": "0"}}
ROWS16 = 0x10100        # bf16 gradient rows + two-product thin products, as lfi_flow_param_grads is given them
# (B, N, C, H, Ks, affine, lstm, gemm_precision), switches -> forward walk, backward walk, thin products. From the rules:
#   register-resident cells: C <= 64, H <= 128, Cout <= 64 and not LFI_FLOW_GENERIC=1; persistent: not LFI_FLOW_PIPE=0
#   bf16x3 forward: precision bit 0, GRU, H16 % 32 == 0 and Ch16 % 32 == 0, not LFI_PIPE_X3=0      (lfi_flow_cells.h, flow_x3_fwd_walk)
#   bf16x3 backward: precision bit 0, GRU, H16 % 32 == 0 and 3 H16 >= 128, not LFI_PIPE_X3=0       (flow_x3_bwd_walk)
#   one pass: bit 16, GRU, H = 128, B % 16 == 0, C <= 64, Ch <= 32, not LFI_FLOW_WGRAD_FUSED=0      (lfi_wgrad.hip, lfi_internal_flow_wgrad_ok)
VARIANTS = [
    ((32, 13, 50, 128, 3, 1, 0, 1 | ROWS16), None, (3, 3, 1)),
    ((32, 13, 50, 128, 3, 1, 0, 1 | ROWS16), "fused0", (3, 3, 0)),
    ((32, 13, 50, 128, 3, 1, 0, 1), None, (3, 3, 0)),               # fp32 rows: four products
    ((48, 2, 64, 128, 1, 1, 0, 1 | ROWS16), None, (3, 3, 1)),       # C = 64: Ch = 32, ldc = 64, the upper limit
    ((24, 2, 50, 128, 1, 1, 0, 1 | ROWS16), None, (3, 3, 0)),       # B not a multiple of 16
    ((32, 2, 50, 96, 1, 1, 0, 1 | ROWS16), None, (3, 3, 0)),        # H != 128
    ((33, 5, 50, 128, 3, 1, 0, 0), None, (2, 2, 0)),
    ((33, 5, 50, 128, 3, 1, 0, 1), "x3off", (2, 2, 0)),
    ((33, 5, 50, 128, 3, 1, 0, 1), "pipe0", (1, 1, 0)),
    ((33, 5, 50, 128, 3, 1, 0, 1), "generic", (0, 0, 0)),
    ((33, 5, 50, 128, 3, 1, 0, 1), "generic+pipe0", (0, 0, 0)),
    ((17, 4, 50, 120, 2, 1, 0, 1), None, (3, 3, 0)),                # H16 = 128
    ((17, 4, 50, 32, 2, 1, 0, 1), None, (3, 2, 0)),                 # 3 H16 = 96 < 128
    ((17, 4, 64, 64, 2, 1, 0, 1), None, (3, 3, 0)),                 # 3 H16 = 192
    ((17, 4, 50, 48, 2, 1, 0, 1), None, (2, 2, 0)),                 # H16 = 48
    ((6, 4, 15, 24, 4, 1, 0, 1), None, (2, 2, 0)),                  # Ch16 = 16; 3 H16 = 96
    ((6, 4, 16, 64, 4, 1, 0, 1), None, (2, 3, 0)),                  # Ch16 = 16 keeps the forward walk f32, not the backward walk
    ((17, 4, 50, 64, 2, 1, 1, 1), None, (2, 2, 0)),                 # LSTM
    ((32, 4, 50, 128, 2, 1, 1, 1 | ROWS16), None, (2, 2, 0)),
    ((5, 3, 50, 160, 2, 1, 0, 0), None, (0, 0, 0)),                 # H > 128
    ((5, 3, 66, 128, 2, 1, 0, 1), None, (0, 0, 0)),                 # C > 64
    ((5, 3, 64, 128, 2, 0, 0, 1), None, (3, 3, 0)),                 # additive: Cout = 32
]


def test_walk_variant_query(monkeypatch):
    from lets_face_it_amd import _lib
    from lets_face_it_amd._lib import FlowDims
    L = _lib.lib()
    for (B, N, C_, H, Ks, affine, lstm, prec), sw, want in VARIANTS:
        for k in gw.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in (SWITCH_OFF[sw] if sw else {}).items():
            monkeypatch.setenv(k, v)
        d = FlowDims(B, N, C_, H, 20, Ks, affine, lstm, 1e-4, prec)
        got = tuple(int(L.lfi_flow_walk_variant(C.byref(d), w)) for w in (0, 1, 2))
        assert got == want, ((B, N, C_, H, Ks, affine, lstm, hex(prec)), sw, got, want)
    for k in gw.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    d = FlowDims(32, 4, 50, 128, 20, 2, 1, 0, 1e-4, 1)
    assert L.lfi_flow_walk_variant(C.byref(d), 3) == -1 and L.lfi_flow_walk_variant(C.byref(d), -1) == -1
    assert L.lfi_flow_walk_variant(C.byref(FlowDims(0, 4, 50, 128, 20, 2, 1, 0, 1e-4, 1)), 0) == -1
    # the GPU cases' own expectations, answered here without a GPU
    for c in gw.CASES:
        for k in gw.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in c.env.items():
            monkeypatch.setenv(k, v)
        bwd_bits, pg_bits = gw.case_bits(c)
        got = (int(L.lfi_flow_walk_variant(C.byref(gw.flow_dims(c)), 0)), int(L.lfi_flow_walk_variant(C.byref(gw.flow_dims(c, bwd_bits)), 1)),
               int(L.lfi_flow_walk_variant(C.byref(gw.flow_dims(c, pg_bits)), 2)))
        assert got == c.expect, (c.id, got, c.expect)
        assert bool(L.lfi_flow_bwd_emits_planes(C.byref(gw.flow_dims(c, bwd_bits)))) >= bool(c.planes), c.id
        assert c.Ks * math.ceil(c.B / 16) <= 64
