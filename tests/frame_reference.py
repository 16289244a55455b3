"""The per-frame flow drivers of a sampler or a streaming session - lfi_flow_sample_seq_nll, lfi_flow_score_seq_from, lfi_flow_score_seq_chunk
(_rows), lfi_flow_step_rows_from - as include/lfi.h states them, in plain torch (any dtype) on tests/flow_reference.py: the definition
the kernels of lfi_flow_chain.hip / lfi_flow_chunk.hip / lfi_flow_chunk_rows.hip / lfi_sample.hip and the frame cells of lfi_flow_cells.h
are compared with, an arithmetic model of their documented roundings, and the comparison the GPU test and the planted-defect tests go
through. Written from glow/models.py as include/lfi.h cites it (reverse_flow :345-373, inference :567-596, create_conditioning :598-615).

Frame n of a run (t = start + n), on the B rows of the session:

    c      = LeakyReLU_0.01(pre_static[n] + faces[:, t - hist1:t].reshape(B, hist1 C) @ wct[:, col:col + hist1 C]^T)      (B x Ks D)
             or, with the window behind a ModalityEncoder of hid units (lfi_p1enc kind mlp / rnn / lstm, inp["p1enc"]):
    e      = LeakyReLU_0.01(window @ W1^T + b1)   |   the state behind the window's last frame of a GRU / an LSTM from h = c = 0
             over its hist1 frames (encoder_reference.windows_forward: the recurrence is not written a second time)      (B x hid)
    c      = LeakyReLU_0.01(pre_static[n] + e @ wct[:, col:col + hid]^T)
    gic[k] = c[:, k D:(k + 1) D] @ W_ih[k][:, Ch:]^T + b_ih[k]
    generate (steps Ks-1 .. 0 from the prior draw noise[n]):  [z1 | z2'] -> cell(z1, gic[k], state k) -> o -> z2 = z2' / scale - shift
                                                              (additive: z2' - o) -> a = [z1 | z2] W^-1 -> x = a exp(-logs) - bias
    observe  (steps 0 .. Ks-1 from the frame faces[:, t]):    flow_reference's forward step, the state carried per flow step
    nll      = -(logdet_fwd + sum_c -0.5 (z_c^2 + log 2 pi)) / ln 2 in both directions: the model's density of the frame

The recurrent cell sees the pass-through half z1 and gic, the same in both directions; its state is zero at the session's first frame.
A generated frame enters `faces` and is read back through the window. Every row takes a role per frame: GEN, OBS or ABSENT (a row
of a ragged chunk behind its length: nothing of it moves).

A run is a dict: x (N x B x C, the frame: generated or given), z (N x B x C: the prior draw or the latent), nll (N x B), h and cstate
(Ks x N x B x H, the state AFTER each frame; cstate None for the GRU cell), c (N x B x Ks D), gic (N x Ks x B x G), raw_scale
(N x Ks x B x C2, the coupling's sigmoid before the clamp; None when additive), logdet_const and, with an encoder, e (N x B x hid: for
the input conditions, not a compared part - where the kernels keep it is not ABI).
"""
import math

import torch

import encoder_reference as er
import flow_reference as fr
from flow_reference import (CLAMP_EPS, EPS, F32_FACTOR, LN2, LOG2PI, MB, MODEL_FACTOR, Dims, _fast_sigmoid, _fast_tanh,  # noqa: F401
                            _invconv, _prod3, derived, failures, make_inputs, rel_l2, tail_start, worst)

GEN, OBS, ABSENT = 0, 1, 2


def roles_all(d, role):
    return torch.full((d.N, d.B), role, dtype=torch.int64)


def roles_ragged(d, lengths):
    """Row b observes the first lengths[b] frames and is absent behind them."""
    n = torch.arange(d.N).unsqueeze(1)
    return torch.where(n < torch.as_tensor(lengths).unsqueeze(0), OBS, ABSENT)


ENCS = ("none", "mlp", "rnn", "lstm")        # lfi_p1enc.kind 0 .. 3


def make_frame_inputs(d, hist1, dense=False, seed=0, clamp=False, enc="none", ehid=0, col=0):
    """flow_reference.make_inputs' parameters and seed frames (x0 is `faces`, B x seq_len x C with seq_len = d.T), plus what a per-frame
    driver is given: wct (Ks D x E, the window's columns from `col`), pre_static (N x B x Ks D) and the prior draws (N x B x C).
    Scales of a trained model: the pre-activation of c has a standard deviation of about 0.5.

    enc "mlp" / "rnn" / "lstm" (lfi_p1enc.kind 1 / 2 / 3): the window goes through a ModalityEncoder of ehid units first, whose
    parameters are inp["p1enc"] - mlp: w1 (ehid x hist1 C), b1; rnn / lstm: w_ih (ng ehid x C), w_hh (ng ehid x ehid), b_ih, b_hh,
    ng = 3 / 4 - and its features meet the columns [col, col + ehid) of wct. E >= col + ehid + 4 and every column of wct is drawn
    alike: a column outside the block is wrong to read, and reading it shows. Scales: the features have a mean magnitude of a few
    tenths and their term has about the variance of pre_static (tests/test_frame_reference_cpu.py checks both on the fp64 runs)."""
    assert enc in ENCS
    inp = make_inputs(d, dense=dense, seed=seed, clamp=clamp)
    g = torch.Generator().manual_seed(seed + 1000)
    K1 = hist1 * d.C
    if enc == "none":
        assert ehid == 0 and col == 0
        E = ((K1 + 3) & ~3) + 4
        inp["wct"] = torch.randn(d.Ks * d.D, E, generator=g) * (0.3 / math.sqrt(K1))
    else:
        assert ehid > 0 and col >= 0
        E = ((col + ehid + 3) & ~3) + 4
        inp["wct"] = torch.randn(d.Ks * d.D, E, generator=g) * (1.5 / math.sqrt(ehid))
    inp["pre_static"] = torch.randn(d.N, d.B, d.Ks * d.D, generator=g) * 0.4
    inp["noise"] = torch.randn(d.N, d.B, d.C, generator=g)
    inp["hist1"], inp["col"] = hist1, col
    if enc == "mlp":
        inp["p1enc"] = {"kind": enc, "hid": ehid, "w1": torch.randn(ehid, K1, generator=g) * (0.8 / math.sqrt(K1)),
                        "b1": torch.randn(ehid, generator=g) * 0.1}
    elif enc != "none":
        ng = 4 if enc == "lstm" else 3
        inp["p1enc"] = {"kind": enc, "hid": ehid, "w_ih": torch.randn(ng * ehid, d.C, generator=g) * (1.0 / math.sqrt(d.C)),
                        "w_hh": torch.randn(ng * ehid, ehid, generator=g) * (1.0 / math.sqrt(ehid)),
                        "b_ih": torch.randn(ng * ehid, generator=g) * 0.1, "b_hh": torch.randn(ng * ehid, generator=g) * 0.3}
    del inp["gic"], inp["c"]
    return inp


# ---- pieces of the arithmetic model
def _split_h(x):
    """fp16 hi + lo of the fp32 value: hi = fp16(v), lo = fp16(v - hi) (x3h_split2 / sc_split)."""
    v = x.to(torch.float32)
    hi = v.to(torch.float16).to(torch.float32)
    lo = (v - hi).to(torch.float16).to(torch.float32)
    return hi.to(x.dtype), lo.to(x.dtype)


def _prod3h(a, b):
    """a @ b as three fp16 products of two-piece operands: lo hi + hi lo + hi hi, lo lo dropped (x3h_mma)."""
    ah, al = _split_h(a)
    bh, bl = _split_h(b)
    return al @ bh + ah @ bl + ah @ bh


def _split3(x):
    v = x.to(torch.float32)
    p0 = v.to(torch.bfloat16).to(torch.float32)
    p1 = (v - p0).to(torch.bfloat16).to(torch.float32)
    p2 = (v - p0 - p1).to(torch.bfloat16).to(torch.float32)
    return p0.to(x.dtype), p1.to(x.dtype), p2.to(x.dtype)


def _prod6(a, b):
    """a @ b as six bf16 products of three-piece operands: every pair of pieces above 2^-24 relative."""
    a0, a1, a2 = _split3(a)
    b0, b1, b2 = _split3(b)
    return a2 @ b0 + a1 @ b1 + a0 @ b2 + a1 @ b0 + a0 @ b1 + a0 @ b0


# ---- seams the planted-defect tests replace (tests/test_frame_reference_cpu.py); the reference itself never changes them
def _state_in(state, k, n):
    """The (h, c) flow step k reads at frame n: its own, as frame n - 1 left it."""
    return state[k]


def _carry(new, old, k, n):
    """The state step k leaves behind frame n."""
    return new


def _keep_absent(new, old, absent):
    """An absent row keeps its state."""
    return torch.where(absent.unsqueeze(1), old, new)


def _window(faces, t, hist1):
    """prev_p1_face of frame t: the hist1 frames in front of it (incl = 0, lfi_gather_windows)."""
    return faces[:, t - hist1:t].reshape(faces.shape[0], -1)


def _enc_window(faces, t, hist1):
    """The same frames as the encoder reads them: B x hist1 x C, oldest first (ModalityEncoder.forward, glow/models.py:55-80)."""
    return faces[:, t - hist1:t]


def _enc_state0(last, zero):
    """The state the window's recurrence starts from: zero at every frame (last: where the previous frame's recurrence ended)."""
    return zero


def _enc_features(hseq):
    """The features of a recurrent encoder: its state behind the window's last frame (output folded: the hidden state once)."""
    return hseq[-1]


def _enc_mlp_act(y):
    return torch.nn.functional.leaky_relu(y, 0.01)


def _enc_cols(wct, col, ehid):
    """The columns of wct the features meet."""
    return wct[:, col:col + ehid]


def _halves(y, Ch):
    """(pass-through half, transformed half)."""
    return y[:, :Ch], y[:, Ch:]


def _join(z1, z2):
    return torch.cat([z1, z2], dim=1)


def _uncouple(z2n, shift, scale):
    """FlowStep.reverse_flow: z2 = z2 / scale, then z2 = z2 - shift (glow/models.py:356-365)."""
    return z2n / scale - shift


def _clamp_scale_rev(s, eps):
    return s.clamp(min=eps)


def _frame_in(given, generated, gen_rows):
    """What `faces` holds for frame t afterwards: a generating row's generated frame, every other row's frame as it was."""
    return torch.where(gen_rows.unsqueeze(1), generated, given)


def _nll(logdet_const, logdet_coupling, z):
    return -(logdet_const + logdet_coupling + (-0.5 * (z ** 2 + LOG2PI)).sum(dim=1)) / LN2


def _run(inp, d, roles, dtype, given=None, fast_gates=False, w_fp32=False, x3h_rev=False, x3h_fwd=False, front=0,
         enc_three_products=False, enc_loop_front=False):
    Ch, C2, Cout, NG, G, I = derived(d)
    B, N, H, Ks, C, D = d.B, d.N, d.H, d.Ks, d.C, d.D
    hist1, col = inp["hist1"], inp["col"]
    K1 = hist1 * C
    assert roles.shape == (N, B) and hist1 <= d.start and d.start + N <= d.T
    par64 = {k: v.detach().double() for k, v in inp["params"].items() if v is not None}
    par = {k: v.to(dtype) for k, v in par64.items()}
    faces = inp["x0"].detach().to(dtype).clone()
    if given is not None:
        for n in range(N):
            m = roles[n] != GEN         # (an absent row's slot holds its frame too: the front end of a ragged chunk stays dense)
            faces[m, d.start + n] = given[n].to(dtype)[m]
    wct, pre_static, noise = (inp[k].detach().to(dtype) for k in ("wct", "pre_static", "noise"))
    sig, tanh = (_fast_sigmoid, _fast_tanh) if fast_gates else (torch.sigmoid, torch.tanh)
    fmm = {0: torch.matmul, 1: _prod3, 5: _prod6, 9: _prod3h}[front]
    enc = inp.get("p1enc")
    if enc is not None:
        ekind, ehid = enc["kind"], enc["hid"]
        ew = {k: v.detach().to(dtype) for k, v in enc.items() if torch.is_tensor(v)}
        emm = _prod3 if enc_three_products else fmm if enc_loop_front else torch.matmul
        edims = er.Dims(B, hist1, 1, hist1 - 1, hist1, ehid, 0, 0)       # one window per row: its hist1 frames, from h = c = 0
        e_last = None

    def cmm(x3h):
        return _prod3h if x3h else torch.matmul
    Ws, Winvs, const = [], [], 0.0
    for k in range(Ks):
        W, ld = _invconv(par, k, dtype)
        Winv = torch.linalg.inv(_invconv(par64, k, torch.float64)[0])     # lfi.h: "Winv [Ks][C][C] (reverse weight, fp64 inverse ..."
        if w_fp32:
            par32 = {key: v.float() for key, v in par.items() if key.startswith("inv_")}
            W = _invconv(par32, k, torch.float32)[0].to(dtype)
            Winv = Winv.float()                                             # "... cast to fp32)"
        Ws.append(W)
        Winvs.append(Winv.to(dtype))
        const = const + C * (par["an_logs"][k].sum() + ld)

    def cell(k, n, z1, gic_k, st, mm):
        hp, cp = st
        gi = gic_k + mm(z1, par["w_ih"][k][:, :Ch].t())
        gh = mm(hp, par["w_hh"][k].t()) + par["b_hh"][k]
        if d.lstm:
            pre = gi + gh
            i_, f_, o_ = sig(pre[:, :H]), sig(pre[:, H:2 * H]), sig(pre[:, 3 * H:])
            cn = f_ * cp + i_ * tanh(pre[:, 2 * H:3 * H])
            h = o_ * tanh(cn)
        else:
            r = sig(gi[:, :H] + gh[:, :H])
            u = sig(gi[:, H:2 * H] + gh[:, H:2 * H])
            h = (1.0 - u) * fr._gru_candidate(gi[:, 2 * H:], r, gh[:, 2 * H:], par["b_hh"][k][2 * H:], tanh) + u * hp
            cn = cp
        o = (mm(h, par["w_fl"][k].t()) + par["b_fl"][k]) * torch.exp(3.0 * par["l_fl"][k])
        return h, cn, o

    zero = faces.new_zeros(B, H)
    state = [(zero, zero) for _ in range(Ks)]
    out = {k: [] for k in ("x", "z", "nll", "c", "gic", "h", "cstate", "raw_scale") + (("e",) if enc is not None else ())}
    for n in range(N):
        t = d.start + n
        role = roles[n]
        gen_rows, obs_rows, absent = role == GEN, role == OBS, role == ABSENT
        if enc is None:
            c = torch.nn.functional.leaky_relu(pre_static[n] + fmm(_window(faces, t, hist1), wct[:, col:col + K1].t()), 0.01)
        else:
            win = _enc_window(faces, t, hist1)
            if ekind == "mlp":
                e = _enc_mlp_act(fmm(win.reshape(B, K1), ew["w1"].t()) + ew["b1"])
            else:
                Xp = fmm(win.reshape(B * hist1, C), ew["w_ih"].t())          # row b hist1 + s: frame s of row b's window
                hseq, _ = er.windows_forward(Xp, ew["w_hh"], ew["b_ih"], ew["b_hh"], None, edims, lstm=ekind == "lstm",
                                             h0=_enc_state0(e_last, faces.new_zeros(B, ehid)), mm=emm, sig=sig, tanh=tanh)
                e, e_last = _enc_features(hseq), hseq[-1]
            c = torch.nn.functional.leaky_relu(pre_static[n] + fmm(e, _enc_cols(wct, col, ehid).t()), 0.01)
            out["e"].append(e)
        gic = [fmm(c[:, k * D:(k + 1) * D], par["w_ih"][k][:, Ch:].t()) + par["b_ih"][k] for k in range(Ks)]
        st_in = [_state_in(state, k, n) for k in range(Ks)]
        new = [None] * Ks
        raw = [faces.new_zeros(B, C2) for _ in range(Ks)]
        x, z, nll = faces[:, t].clone(), noise[n].clone(), faces.new_zeros(B)

        def pick(a, b, rows):
            return torch.where(rows.unsqueeze(1) if a.dim() == 2 else rows, a, b)
        if bool(gen_rows.any()):
            mm = cmm(x3h_rev)
            y, ld = noise[n], faces.new_zeros(B)
            for k in range(Ks - 1, -1, -1):
                z1, z2n = _halves(y, Ch)
                h, cn, o = cell(k, n, z1, gic[k], st_in[k], mm)
                if d.affine:
                    s = sig(o[:, 1::2] + 2.0)
                    raw[k] = pick(s, raw[k], gen_rows)
                    scale = _clamp_scale_rev(s, d.scale_eps)
                    z2 = _uncouple(z2n, o[:, 0::2], scale)
                    ld = ld + torch.log(scale).sum(dim=1)
                else:
                    z2 = z2n - o
                y = mm(_join(z1, z2), Winvs[k]) * torch.exp(-par["an_logs"][k]) - par["an_bias"][k]
                new[k] = (h, cn)
            x = _frame_in(x, y, gen_rows)
            nll = pick(_nll(const, ld, noise[n]), nll, gen_rows)
        if bool(obs_rows.any()):
            mm = cmm(x3h_fwd)
            y, ld = faces[:, t], faces.new_zeros(B)
            for k in range(Ks):
                a = (y + par["an_bias"][k]) * torch.exp(par["an_logs"][k])
                z1, z2 = _halves(mm(a, Ws[k]), Ch)
                h, cn, o = cell(k, n, z1, gic[k], st_in[k], mm)
                if d.affine:
                    s = sig(o[:, 1::2] + 2.0)
                    raw[k] = pick(s, raw[k], obs_rows)
                    scale = fr._clamp_scale(s, d.scale_eps)
                    z2 = (z2 + o[:, 0::2]) * scale
                    ld = ld + torch.log(scale).sum(dim=1)
                else:
                    z2 = z2 + o
                y = _join(z1, z2)
                new[k] = (h, cn) if new[k] is None else (pick(h, new[k][0], obs_rows), pick(cn, new[k][1], obs_rows))
            z = pick(y, z, obs_rows)
            nll = pick(_nll(const, ld, y), nll, obs_rows)
        for k in range(Ks):
            old = st_in[k] if new[k] is None else None
            hn, cn = new[k] if new[k] is not None else old
            hn, cn = _carry(hn, state[k][0], k, n), _carry(cn, state[k][1], k, n)
            state[k] = (_keep_absent(hn, state[k][0], absent), _keep_absent(cn, state[k][1], absent))
        faces[:, t] = x
        out["x"].append(x)
        out["z"].append(z)
        out["nll"].append(nll)
        out["c"].append(c)
        out["gic"].append(torch.stack(gic))
        out["h"].append(torch.stack([s[0] for s in state]))
        out["cstate"].append(torch.stack([s[1] for s in state]))
        out["raw_scale"].append(torch.stack(raw))
    run = {k: torch.stack(v) for k, v in out.items()}
    run["h"], run["cstate"] = run["h"].transpose(0, 1), run["cstate"].transpose(0, 1)      # Ks x N x B x H
    if not d.lstm:
        run["cstate"] = None
    if not d.affine:
        run["raw_scale"] = None
    run["logdet_const"] = const
    run["faces"] = faces
    return run


def run_exact(inp, d, roles, dtype=torch.float64, given=None):
    """The reference run in `dtype`: fp64 is the exact reference, fp32 the second term of the bound. given (N x B x C): the frames of
    the rows that do not generate (default: what inp["x0"] holds at start + n)."""
    with torch.no_grad():
        return _run(inp, d, roles, dtype, given=given)


def run_model(inp, d, roles, given=None, **flags):
    """The same run in fp64 with ONLY the roundings the kernels document, each behind a flag:

    fast_gates   sigmoid and tanh - the cells' gates and the coupling's sigmoid(. + 2) - are lfi_common.h's sigmoidf_ / tanhf_: "Gate
                 non-linearities on the hardware transcendental units (v_exp_f32 = 2^x, v_rcp_f32; ~1 ulp each) ... Absolute error
                 ~1e-7 on values in (-1, 1)"
    w_fp32       W = P L U is built in fp32 (lfi_flow.hip, flow_prep_invconv_kernel: "W = P T" with float sums) and the reverse
                 weight is include/lfi.h's "Winv [Ks][C][C] (reverse weight, fp64 inverse cast to fp32)"
    x3h_rev      every product of the reverse cell - z1 W_ih[:, :Ch]^T, h W_hh^T, h' W_fl^T, [z1 | z2] W^-1 - as lfi_flow_cells.h's
                 "three fp16 products of two-piece operands" (FramePlan.x3; "fp16 pieces (11 + 11 mantissa bits: 2^-22 relative,
                 fp32-grade)": hi = fp16(x), lo = fp16(x - hi), x3h_mma sums a.lo w.hi + a.hi w.lo + a.hi w.hi)
    x3h_fwd      the same for the forward cell, a W included (fwd_chain_cell: "X3: every product as three fp16 products of two-piece
                 operands (x3h_*, fp32-grade: 2^-22 relative)"; FramePlan.x3f: "for per-frame arithmetic 9 ONLY")
    front        lfi_gemm_desc.precision of the front end's two products, window @ wct^T and c @ W_ih[:, Ch:]^T (lfi.h): 0 "exact fp32
                 (f32-input MFMA)"; 1 "bf16x3 - operands split into bf16 hi + lo on the fly, three bf16 MFMAs per step"; 5 "SIX bf16
                 products of three-piece operands (x = p0 + p1 + p2, 24 mantissa bits; what is dropped is 2^-24 relative"; 9 "three
                 products of FP16 pieces (11 + 11 mantissa bits, 2^-22 relative" - which is also the fused kernel's arithmetic
                 (lfi_sample.hip: "Arithmetic as the per-frame GEMMs it replaces (lfi_gemm_desc.precision 9)", c kept "as fp16 hi / lo
                 pieces")

    and, where the window goes through an encoder (inp["p1enc"]), that encoder's, as encoder_reference.run_model words them:

    front        also the mlp's product window W1^T, the recurrent kinds' input projection window W_ih^T and e wct[:, col:col + hid]^T
                 (lfi_internal_sample_front_rows hands d->gemm_precision to all of them)
    enc_three_products  both operands of h W_hh^T are split into bf16 hi + lo, summed as hi hi + hi lo + lo hi: the fused GRU kernels
                 at lfi_enc_desc.precision = 1 - "1 -> bf16x3 recurrence; any other value -> exact f32 recurrence" (lfi.h, lfi_p1enc)
    enc_loop_front  h W_hh^T per history step at `front`'s arithmetic: the unfused loop (hid > 256) and the LSTM loop - "loops take the
                 GEMM mode as given"
    fast_gates   covers the encoder's sigmoid and tanh too (ENC_SIG / ENC_TANH are sigmoidf_ / tanhf_)

    With every flag off this IS run_exact(inp, d, roles, torch.float64)."""
    with torch.no_grad():
        return _run(inp, d, roles, torch.float64, given=given, **flags)


# ---------------------------------------------------------------------------------------------- the comparison
def pieces(run, d, roles):
    """The separately measured parts of what `run` holds (a value of None is a quantity the run does not have;
    run["state_frames"]: the frames whose state it has, default all): x[n] over the generating rows, z[n] over the observing
    rows (the other rows' are inputs), nll[n] over the rows that are not absent, c[n]; h[k][n] and cstate[k][n] over all rows; the
    rows of the last batch tile of x and h once more on their own; in a frame with both roles, the observing and the generating rows
    of nll and h on their own, and x.obs[n]: the observing rows' frames, which every run holds exactly as given."""
    N, B = roles.shape
    tb = tail_start(B)
    out = []

    def add(name, t, rows=None):
        if t is None:
            return
        if rows is not None:
            if not bool(rows.any()):
                return
            t = t[rows.to(t.device)]
        out.append((name, t))
    for n in range(N):
        live = roles[n] != ABSENT
        mixed = bool((roles[n] == GEN).any()) and bool((roles[n] == OBS).any())
        gen, obs = roles[n] == GEN, roles[n] == OBS
        if run.get("x") is not None:        # (an observing row's frame is given: where the roles mix it must still be there, exactly)
            add("x[%d]" % n, run["x"][n], gen)
            if tb is not None:
                add("x.tail[%d]" % n, run["x"][n], gen & (torch.arange(B) >= tb))
            if mixed:
                add("x.obs[%d]" % n, run["x"][n], obs)
        if run.get("z") is not None:        # (a generating row's z is its prior draw: an input)
            add("z[%d]" % n, run["z"][n], obs)
        if run.get("nll") is not None:
            add("nll[%d]" % n, run["nll"][n], live)
            if mixed:
                add("nll.obs[%d]" % n, run["nll"][n], obs)
                add("nll.gen[%d]" % n, run["nll"][n], gen)
        if run.get("c") is not None:
            add("c[%d]" % n, run["c"][n])
    for n in run.get("state_frames", range(N)):
        mixed = bool((roles[n] == GEN).any()) and bool((roles[n] == OBS).any())
        for k in range(d.Ks):
            for key in ("h", "cstate"):
                if run.get(key) is None:
                    continue
                add("%s[%d][%d]" % (key, k, n), run[key][k, n])
                if mixed:
                    add("%s.obs[%d][%d]" % (key, k, n), run[key][k, n], roles[n] == OBS)
                    add("%s.gen[%d][%d]" % (key, k, n), run[key][k, n], roles[n] == GEN)
            if tb is not None:
                add("h.tail[%d][%d]" % (k, n), run["h"][k, n, tb:])
    return out


def compare(got, exact, model, fp32, d, roles):
    """-> rows (name, err, allowed, ok) over every part `got` holds: err(got) <= MODEL_FACTOR * err(model) + F32_FACTOR * err(fp32),
    every error a rel_l2 against `exact` with no floor (flow_reference.compare's rule). A part whose exact norm is 0 must be exactly 0;
    a non-finite value fails; nothing `got` holds is skipped."""
    e_, m_, f_ = (dict(pieces(r, d, roles)) for r in (exact, model, fp32))
    rows = []
    for name, g in pieces(got, d, roles):
        e = e_[name]
        assert g.shape == e.shape, (name, tuple(g.shape), tuple(e.shape))
        err = rel_l2(g.cpu(), e)
        allowed = MODEL_FACTOR * rel_l2(m_[name], e) + F32_FACTOR * rel_l2(f_[name], e)
        ok = bool(torch.isfinite(g).all()) and err <= allowed
        rows.append((name, err, allowed, ok))
    return rows
