"""tests/frame_reference.py checked on the CPU: the reference against the oracle's flow_reverse / flow_forward / nll_bits looped over
frames with one carried state, the two directions against each other, ragged and mixed-role runs against the dense ones row by row,
the arithmetic model flag by flag, every case of the GPU test clean and within its input conditions, the comparison against planted
defects - the evidence that its bounds would notice a subtly wrong kernel - and lfi_flow_frame_plan for every case and switch. The
window behind a ModalityEncoder (lfi_p1enc kind mlp / rnn / lstm) throughout: oracle.encode_window in the oracle loop, the encoder's
flags, the input conditions that keep a wrong encoder from hiding behind pre_static, eight planted encoder defects, and the
window-encoder kernel every recurrent case reaches (lfi_encode_windows_fwd_variant, host only).
(SeqGlow.inference, glow/models.py:567-596; FlowStep.reverse_flow :345-373.)"""
import ctypes as C

import pytest
import torch

import flow_reference as fr
import frame_reference as fq
import test_gpu_frame_drivers as gd
from flow_reference import Dims
from helpers import rel_l2
from oracle import seqglow_oracle as oracle

HIST1, START = gd.HIST1, gd.START


def _errs(run, exact, d, roles):
    e = dict(fq.pieces(exact, d, roles))
    return {n: rel_l2(a, e[n]) for n, a in fq.pieces(run, d, roles)}


def _mixed_roles(d):
    b, n = torch.arange(d.B).unsqueeze(0), torch.arange(d.N).unsqueeze(1)
    kind = (b // 16 + n) % 3
    return torch.where(kind == 0, fq.OBS, torch.where(kind == 1, fq.GEN, (b + n) % 2))


# ------------------------------------------------------------------------------------------ (a) the oracle
_ORACLE = [(7, 6, 0, 1, 0, "none"), (6, 5, 1, 0, 1, "none"), (5, 4, 0, 0, 0, "none"), (9, 6, 1, 1, 1, "none"), (2, 3, 0, 1, 0, "none"),
           (7, 6, 0, 1, 0, "mlp"), (7, 6, 0, 1, 0, "rnn"), (6, 5, 1, 0, 1, "lstm"), (5, 4, 0, 0, 0, "rnn"), (9, 6, 1, 1, 1, "mlp")]
ECOL, EHID = 3, 5       # the encoded kinds' block of the conditioning: columns [3, 8) of E = 12


@pytest.mark.parametrize("C_,H,lstm,affine,dense,enc", _ORACLE, ids=["-".join(str(v) for v in c if v != "none") for c in _ORACLE])
def test_reference_is_the_oracle_looped_over_frames(C_, H, lstm, affine, dense, enc):
    """x, z, nll and the state of both directions against oracle.flow_reverse / flow_forward / nll_bits looped over N frames with one
    carried state, in fp64. c and gic are made consistent: the oracle's cond_transform reads [window | extra features] with wct's own
    columns, and pre_static is the extra features' part of it with the bias. The encoded kinds: the p1_face block of the conditioning
    is oracle.encode_window's (ModalityEncoder.forward) over the same window - of a recurrent kind's cat(seq[:, -1], h_n[0]) the state
    once, the folded layout - in columns [col, col + hid) between extra features on both sides."""
    d = Dims(5, START + 5, 4, START, C_, H, 3, 2, affine, lstm, 0.88 if affine else 1e-4)
    Ch, C2, Cout, NG, G, I = fr.derived(d)
    g = torch.Generator().manual_seed(5)
    K1 = HIST1 * d.C
    if enc == "none":
        inp = fq.make_frame_inputs(d, HIST1, dense=bool(dense), seed=21)
        wct = inp["wct"].double()
        E = wct.shape[1]
        extra = torch.randn(d.N, d.B, E - K1, generator=g, dtype=torch.float64)
        bct = torch.randn(d.Ks * d.D, generator=g, dtype=torch.float64) * 0.2
        inp["pre_static"] = extra @ wct[:, K1:].t() + bct

        def cond_of(faces, t, n):
            return torch.cat([faces[:, t - HIST1:t].reshape(d.B, K1), extra[n]], dim=1)
    else:
        inp = fq.make_frame_inputs(d, HIST1, dense=bool(dense), seed=21, enc=enc, ehid=EHID, col=ECOL)
        wct = inp["wct"].double()
        E = wct.shape[1]
        assert E >= ECOL + EHID + 4 and bool((wct != 0).all())
        extra = torch.randn(d.N, d.B, E, generator=g, dtype=torch.float64)
        extra[:, :, ECOL:ECOL + EHID] = 0.0
        bct = torch.randn(d.Ks * d.D, generator=g, dtype=torch.float64) * 0.2
        inp["pre_static"] = extra @ wct.t() + bct
        pe = inp["p1enc"]
        prefix = "feature_encoder.p1_face_encoder."
        esd = ({prefix + "encoder.0.weight": pe["w1"].double(), prefix + "encoder.0.bias": pe["b1"].double()} if enc == "mlp" else
               {prefix + "encoder.weight_ih_l0": pe["w_ih"].double(), prefix + "encoder.weight_hh_l0": pe["w_hh"].double(),
                prefix + "encoder.bias_ih_l0": pe["b_ih"].double(), prefix + "encoder.bias_hh_l0": pe["b_hh"].double()})

        def cond_of(faces, t, n):
            feats = oracle.encode_window(faces[:, t - HIST1:t], enc, esd, prefix)
            if enc != "mlp":
                assert feats.shape[1] == 2 * EHID and torch.equal(feats[:, :EHID], feats[:, EHID:])
            cond = extra[n].clone()
            cond[:, ECOL:ECOL + EHID] = feats[:, :EHID]
            return cond
    par = {k: v.double() for k, v in inp["params"].items()}
    hp = {"Glow": {"K": d.Ks, "L": 1, "scale_eps": d.scale_eps, "rnn_type": "lstm" if lstm else "gru",
                   "flow_coupling": "affine" if affine else "additive"}}
    names = {"an_bias": "actnorm.bias", "an_logs": "actnorm.logs", "inv_l": "invconv.l", "inv_u": "invconv.u", "inv_logs": "invconv.log_s",
             "inv_p": "invconv.p", "inv_sign": "invconv.sign_s", "inv_w": "invconv.weight", "w_ih": "f.rnn.weight_ih",
             "w_hh": "f.rnn.weight_hh", "b_ih": "f.rnn.bias_ih", "b_hh": "f.rnn.bias_hh", "w_fl": "f.final_linear.weight",
             "b_fl": "f.final_linear.bias", "l_fl": "f.final_linear.logs"}
    sd = {}
    for key, t in par.items():
        for k in range(d.Ks):
            sd["glow.flow.layers.%d.%s" % (k, names[key])] = t[k]
    for k in range(d.Ks):
        sd["glow.flow.layers.%d.f.cond_transform.0.weight" % k] = wct[k * d.D:(k + 1) * d.D]
        sd["glow.flow.layers.%d.f.cond_transform.0.bias" % k] = bct[k * d.D:(k + 1) * d.D]

    def states(state):
        h = torch.stack([s[0] for s in state])
        return h, (torch.stack([s[1] for s in state]) if lstm else None)
    gen = fq.run_exact(inp, d, fq.roles_all(d, fq.GEN))
    if affine:
        clamped = float((gen["raw_scale"] < d.scale_eps).double().mean())
        assert 0.05 < clamped < 0.95, clamped        # the clamp is part of what is compared
    faces = inp["x0"].double().clone()
    state = oracle._new_state(hp)
    for n in range(d.N):
        t = START + n
        cond = cond_of(faces, t, n)
        x, logdet = oracle.flow_reverse(hp, sd, inp["noise"][n].double(), cond, state)
        faces[:, t] = x
        h, cs = states(state)
        assert rel_l2(gen["x"][n], x) < 1e-11 and rel_l2(gen["nll"][n], oracle.nll_bits(-logdet, inp["noise"][n].double())) < 1e-12
        assert rel_l2(gen["h"][:, n], h) < 1e-11 and (not lstm or rel_l2(gen["cstate"][:, n], cs) < 1e-11)
    # the forward direction over frames of its own (the seed sequence's, not a reverse run's)
    obs = fq.run_exact(inp, d, fq.roles_all(d, fq.OBS))
    faces = inp["x0"].double()
    state = oracle._new_state(hp)
    for n in range(d.N):
        t = START + n
        cond = cond_of(faces, t, n)
        z, logdet, _ = oracle.flow_forward(hp, sd, faces[:, t], cond, state)
        h, cs = states(state)
        assert rel_l2(obs["z"][n], z) < 1e-12 and rel_l2(obs["nll"][n], oracle.nll_bits(logdet, z)) < 1e-12
        assert rel_l2(obs["h"][:, n], h) < 1e-12 and (not lstm or rel_l2(obs["cstate"][:, n], cs) < 1e-12)
        assert torch.equal(obs["x"][n], faces[:, t])


# ------------------------------------------------------------------------------------------ (b) the directions, the roles
@pytest.mark.parametrize("lstm,affine,dense", [(0, 1, 0), (1, 1, 1), (0, 0, 0)])
def test_directions_and_roles_are_consistent(lstm, affine, dense):
    """Observing the frames a reverse run generated gives that run's z, nll, h and cstate; a ragged run is the dense run cut off row by
    row; a mixed-role run over the generated frames is the generating run."""
    d = Dims(19, START + 5, 4, START, 7, 6, 3, 2, affine, lstm, 0.88 if affine else 1e-4)
    inp = fq.make_frame_inputs(d, HIST1, dense=bool(dense), seed=2)
    gen = fq.run_exact(inp, d, fq.roles_all(d, fq.GEN))
    obs = fq.run_exact(inp, d, fq.roles_all(d, fq.OBS), given=gen["x"])
    keys = ("z", "nll", "h") + (("cstate",) if lstm else ())
    for key in keys + ("x", "c"):
        assert rel_l2(obs[key], gen[key]) < 1e-10, key
    lengths = [b % (d.N + 1) for b in range(d.B)]
    roles = fq.roles_ragged(d, lengths)
    rag = fq.run_exact(inp, d, roles, given=gen["x"])
    for b, n_b in enumerate(lengths):
        for n in range(d.N):
            last = min(n, n_b - 1)      # the frame whose state row b still holds behind frame n
            want = obs["h"][:, last, b] if last >= 0 else torch.zeros_like(obs["h"][:, 0, b])
            assert torch.equal(rag["h"][:, n, b], want), (b, n)
            if n < n_b:
                assert torch.equal(rag["z"][n, b], obs["z"][n, b]) and torch.equal(rag["nll"][n, b], obs["nll"][n, b])
    names = [n for n, _ in fq.pieces(rag, d, roles)]
    assert "z[%d]" % (d.N - 1) in names and "h[0][0]" in names
    assert dict(fq.pieces(rag, d, roles))["z[%d]" % (d.N - 1)].shape[0] == sum(v == d.N for v in lengths)
    roles = _mixed_roles(d)
    mix = fq.run_exact(inp, d, roles, given=gen["x"])
    for key in ("x", "nll", "h", "c"):
        assert rel_l2(mix[key], gen[key]) < 1e-10, key
    names = [n for n, _ in fq.pieces(mix, d, roles)]
    assert {"x.obs[0]", "x[0]", "nll.gen[0]", "nll.obs[1]", "h.gen[1][2]", "h.tail[0][3]", "x.tail[0]"} <= set(names), names


# ------------------------------------------------------------------------------------------ (c) the model's flags
FLAG_DIMS = Dims(5, START + 5, 4, START, 7, 6, 3, 2, 1, 0, 1e-4)


_NOFLAGS = [(0, 1, 0, "none"), (1, 0, 1, "none"), (0, 1, 0, "mlp"), (0, 1, 0, "rnn"), (1, 0, 1, "lstm")]


@pytest.mark.parametrize("lstm,affine,dense,enc", _NOFLAGS, ids=["-".join(str(v) for v in c if v != "none") for c in _NOFLAGS])
def test_model_without_flags_is_the_reference_bit_for_bit(lstm, affine, dense, enc):
    d = FLAG_DIMS._replace(lstm=lstm, affine=affine)
    inp = fq.make_frame_inputs(d, HIST1, dense=bool(dense), seed=3, **(dict(enc=enc, ehid=6, col=3) if enc != "none" else {}))
    for roles in (fq.roles_all(d, fq.GEN), fq.roles_all(d, fq.OBS), _mixed_roles(d), fq.roles_ragged(d, [0, 4, 1, 2, 3])):
        exact, model = fq.run_exact(inp, d, roles), fq.run_model(inp, d, roles)
        got = fq.pieces(model, d, roles)
        assert len(got) == len(fq.pieces(exact, d, roles))
        for (name, m), (_, e) in zip(got, fq.pieces(exact, d, roles)):
            assert torch.equal(m, e), name
        assert (enc == "none") == ("e" not in exact) and (enc == "none" or torch.equal(model["e"], exact["e"]))


def test_raw_window_inputs_do_not_depend_on_the_encoder_arguments():
    """enc = "none" is the function as it was: the same draws in the same order whether the new arguments are named or not, no
    encoder in the inputs, no e in the run; and an encoded kind changes wct's width and scale but not the draws behind it."""
    d = FLAG_DIMS
    a, b = fq.make_frame_inputs(d, HIST1, seed=3), fq.make_frame_inputs(d, HIST1, seed=3, enc="none", ehid=0, col=0)
    K1 = HIST1 * d.C
    assert "p1enc" not in a and a["col"] == 0 and a["wct"].shape == (d.Ks * d.D, ((K1 + 3) & ~3) + 4)
    g = torch.Generator().manual_seed(1003)
    assert torch.equal(a["wct"], torch.randn(d.Ks * d.D, a["wct"].shape[1], generator=g) * (0.3 / K1 ** 0.5))
    assert torch.equal(a["pre_static"], torch.randn(d.N, d.B, d.Ks * d.D, generator=g) * 0.4)
    for k in ("wct", "pre_static", "noise", "x0"):
        assert torch.equal(a[k], b[k]), k
    e = fq.make_frame_inputs(d, HIST1, seed=3, enc="rnn", ehid=6, col=3)
    assert e["wct"].shape[1] == 16 and e["col"] == 3 and torch.equal(e["x0"], a["x0"]) and bool((e["wct"] != 0).all())
    for k in a["params"]:
        assert a["params"][k] is None or torch.equal(a["params"][k], e["params"][k]), k


def test_encoder_flags_round_what_they_say():
    """The encoder's flags, each alone, on c - the part right behind the encoder: front moves every kind by the precision it names;
    enc_three_products moves a recurrent kind by bf16x3's 2^-16 and an mlp not at all; enc_loop_front is `front` on h W_hh^T, so
    nothing without a front and more than front alone with one; fast_gates reaches the encoder's gates (the first frame's c has no
    other gate in front of it)."""
    d = FLAG_DIMS
    roles = fq.roles_all(d, fq.OBS)
    for enc in ("mlp", "rnn", "lstm"):
        inp = fq.make_frame_inputs(d, HIST1, seed=1, enc=enc, ehid=6, col=3)
        exact = fq.run_exact(inp, d, roles)

        def c0(**flags):
            return _errs(fq.run_model(inp, d, roles, **flags), exact, d, roles)["c[0]"]
        for front, lo, hi in ((1, 1e-6, 5e-5), (5, 1e-9, 3e-7), (9, 3e-8, 2e-6)):
            assert lo < c0(front=front) < hi, (enc, front, c0(front=front))
        assert c0(enc_loop_front=True) == 0.0
        if enc == "mlp":
            assert c0(enc_three_products=True) == 0.0 and c0(fast_gates=True) == 0.0 and c0(front=9, enc_loop_front=True) == c0(front=9)
        else:
            assert 1e-7 < c0(enc_three_products=True) < 5e-5, (enc, c0(enc_three_products=True))
            assert 1e-9 < c0(fast_gates=True) < 2e-6, (enc, c0(fast_gates=True))
            assert c0(front=1, enc_loop_front=True) != c0(front=1)


def test_model_flags_round_what_they_say():
    """Each flag alone: the parts it cannot touch stay exactly as they were, the others move by about the precision it names."""
    d = FLAG_DIMS
    inp = fq.make_frame_inputs(d, HIST1, seed=1)
    groles, oroles = fq.roles_all(d, fq.GEN), fq.roles_all(d, fq.OBS)
    gen = fq.run_exact(inp, d, groles)
    obs = fq.run_exact(inp, d, oroles, given=gen["x"].float())
    cells_g = ("x[0]", "x[3]", "nll[0]", "h[0][0]", "h[1][3]")
    cells_o = ("z[0]", "z[3]", "nll[0]", "h[0][0]", "h[1][3]")

    def g(**flags):
        return _errs(fq.run_model(inp, d, groles, **flags), gen, d, groles)

    def o(**flags):
        return _errs(fq.run_model(inp, d, oroles, given=gen["x"].float(), **flags), obs, d, oroles)
    e = g(fast_gates=True)                        # fp32 expressions: an ulp of 1.0 on every gate; the first frame's front end has none
    assert all(1e-9 < e[k] < 2e-6 for k in cells_g + ("h[1][0]", "c[1]")) and e["c[0]"] == 0.0, e
    e = o(fast_gates=True)                        # (observed frames are given: no c moves)
    assert all(1e-9 < e[k] < 2e-6 for k in cells_o) and all(e["c[%d]" % n] == 0.0 for n in range(d.N)), e
    e = g(w_fp32=True)                            # 2^-24 on W^-1: the top cell of the first frame has not seen it yet
    assert all(0 < e[k] < 3e-7 for k in cells_g) and e["h[1][0]"] == 0.0 and e["c[0]"] == 0.0, e
    e = o(w_fp32=True)
    assert all(0 < e[k] < 3e-7 for k in cells_o), e
    e = g(x3h_rev=True)                           # 2^-22 per product of the reverse cell, and nothing of the forward cell
    assert all(0 < e[k] < 2e-6 for k in cells_g + ("h[1][0]",)) and e["c[0]"] == 0.0, e
    assert all(v == 0.0 for v in o(x3h_rev=True).values())
    e = o(x3h_fwd=True)
    assert all(0 < e[k] < 2e-6 for k in cells_o) and all(e["c[%d]" % n] == 0.0 for n in range(d.N)), e
    assert all(v == 0.0 for v in g(x3h_fwd=True).values())
    for front, lo, hi in ((1, 1e-6, 5e-5), (5, 1e-9, 3e-7), (9, 3e-8, 2e-6)):     # 2^-16, 2^-24, 2^-22 on both products of the front end
        for e, cells in ((o(front=front), cells_o), (g(front=front), cells_g)):
            assert all(0 < e[k] < hi for k in cells) and all(lo < e[k] < hi for k in ("c[0]", "c[3]")), (front, e)
    c0 = [o(front=front)["c[0]"] for front in (1, 9, 5)]
    assert c0[0] > 10 * c0[1] > 100 * c0[2] * 0.1 and c0[1] > 10 * c0[2], c0


# ------------------------------------------------------------------------------------------ (d) every GPU case, clean
def _legs(c):
    ref = gd.references(c)
    return gd.ref_dims(c), ref


@pytest.mark.parametrize("c", gd.CASES, ids=[c.id for c in gd.CASES])
def test_clean_run_passes(c):
    """The fp32 reference handed to the comparison as if it were the case's kernels, leg by leg: it passes, no part that has a value is
    allowed nothing, and the allowances are of the size of the arithmetic."""
    d, ref = _legs(c)
    flags = gd.model_flags(c)
    worst_allowed = 0.0
    for leg, Lg in ref["legs"].items():
        rows = fq.compare(Lg["fp32"], Lg["exact"], gd.model_run(ref, leg, d, flags), Lg["fp32"], d, Lg["roles"])
        assert not fq.failures(rows), (leg, fq.failures(rows))
        exact = dict(fq.pieces(Lg["exact"], d, Lg["roles"]))
        for name, e, a, ok in rows:
            assert (a > 0) == (float(exact[name].abs().max()) > 0) or name.startswith("x.obs"), (leg, name)
            # (nothing allowed: only the state of rows no frame has reached yet, and the given frames of observing rows)
            assert a > 0 or name.split("[")[0].split(".")[0] in ("h", "cstate") or name.startswith("x.obs"), (leg, name)
        worst_allowed = max(worst_allowed, max(a for n, e, a, ok in rows))
    print("%s: largest allowance %.2e" % (c.id, worst_allowed))
    # the ceiling, from these runs: 1.7e-5 where the front end's products are three bf16 products (final-1), 9.3e-6 (h120) at most
    # everywhere else - fp32-grade arithmetic, nothing like a fixed 1e-4 gate. The encoded kinds stay under the same two ceilings:
    # 2.9e-5 (rnn128-1: the bf16x3 recurrence behind bf16x3 front products) at precision 1, 7.6e-6 (rnn-hist4) at most everywhere else
    assert worst_allowed < (5e-5 if c.p == 1 else 2e-5), worst_allowed


@pytest.mark.parametrize("c", gd.CASES, ids=[c.id for c in gd.CASES])
def test_input_conditions(c):
    """Conditions, not measurements: every kernel input and every frame, state, c and gic of the fp64 runs stays below 100 (fp16's
    range is 65504); the clamp case clamps between 20 % and 80 % of the raw scales, none within 1e-3 of the threshold, and the fp32
    run and the model clamp the same set."""
    d, ref = _legs(c)
    inp = ref["inp"]
    big = max(float(v.abs().max()) for v in [inp["wct"], inp["pre_static"], inp["noise"], inp["x0"]] +
              [v for v in inp["params"].values() if v is not None])
    for leg, Lg in ref["legs"].items():
        big = max([big] + [float(Lg["exact"][k].abs().max()) for k in ("x", "z", "h", "c", "gic")])
        assert all(bool(torch.isfinite(Lg["exact"][k]).all()) for k in ("x", "z", "nll", "h", "c"))
    assert big < 100.0, big
    if c.enc != "none":
        # the encoder is neither dead nor saturated, and a wrong one cannot hide behind pre_static: its term carries a quarter of the
        # variance of c's pre-activation at least
        pe = inp["p1enc"]
        big = max([big] + [float(v.abs().max()) for v in pe.values() if torch.is_tensor(v)])
        blk = inp["wct"][:, c.col:c.col + c.ehid].double()
        for leg, Lg in ref["legs"].items():
            e = Lg["exact"]["e"]
            assert e.shape == (c.N, c.B, c.ehid) and bool(torch.isfinite(e).all())
            mean = float(e.abs().mean())
            assert 0.05 <= mean <= 0.8, (leg, mean)
            term = e @ blk.t()
            share = float(term.var()) / float((inp["pre_static"].double() + term).var())
            print("%s %s: mean |e| %.3f, the encoded term's share of the variance %.2f" % (c.id, leg, mean, share))
            assert share >= 0.25, (leg, share)
            big = max(big, float(e.abs().max()), float(term.abs().max()))
        assert big < 100.0, big
    if c.clamp:
        assert d.scale_eps == fr.CLAMP_EPS
        for leg in ("gen", "obs"):
            Lg = ref["legs"][leg]
            s = Lg["exact"]["raw_scale"]
            frac = float((s < d.scale_eps).double().mean())
            assert 0.2 <= frac <= 0.8, (leg, frac)
            assert float((s - d.scale_eps).abs().min()) >= 1e-3, leg
            for run in (Lg["fp32"], gd.model_run(ref, leg, d, gd.model_flags(c))):
                assert torch.equal(run["raw_scale"] < d.scale_eps, s < d.scale_eps), leg


# ------------------------------------------------------------------------------------------ (e) planted defects
SMALL = Dims(17, START + 5, 4, START, 6, 8, 3, 2, 1, 0, 1e-4)           # one full batch tile and a one-row tile
CLAMPED = SMALL._replace(scale_eps=fr.CLAMP_EPS)
X3 = dict(fast_gates=True, w_fp32=True, x3h_rev=True, x3h_fwd=True, front=9)


def _patched(name, fn, module=fq):
    def plant(clean, inp, d, roles, given, flags, mp):
        mp.setattr(module, name, fn)
        return fq.run_model(inp, d, roles, given=given, **flags) if flags else fq.run_exact(inp, d, roles, torch.float32, given=given)
    return plant


def _stale_row(clean, inp, d, roles, given, flags, mp):
    x, h = clean["x"].clone(), clean["h"].clone()
    x[2, d.B - 1] = x[1, d.B - 1]
    h[1, 2, d.B - 1] = h[1, 1, d.B - 1]
    return dict(clean, x=x, h=h)


def _swap_halves(clean, inp, d, roles, given, flags, mp):
    Ch = d.C // 2
    mp.setattr(fq, "_halves", lambda y, ch: (y[:, -Ch:], y[:, :-Ch]))
    mp.setattr(fq, "_join", lambda z1, z2: torch.cat([z2, z1], dim=1))
    return fq.run_exact(inp, d, roles, torch.float32, given=given)


def _two_products(a, b):
    ah, al = fq._split_h(a)
    bh, bl = fq._split_h(b)
    return ah @ bl + ah @ bh


def _lstm_gates_ifog(clean, inp, d, roles, given, flags, mp):
    """The encoder's gate blocks read as i, f, o, g: the same as its blocks g and o exchanged in all four parameters."""
    hid = inp["p1enc"]["hid"]
    order = torch.cat([torch.arange(2 * hid), torch.arange(3 * hid, 4 * hid), torch.arange(2 * hid, 3 * hid)])
    pe = {k: (v[order] if torch.is_tensor(v) else v) for k, v in inp["p1enc"].items()}
    return fq.run_exact(dict(inp, p1enc=pe), d, roles, torch.float32, given=given)


GEN_, OBS_, RAG_, MIX_ = "gen", "obs", "ragged", "mixed"
EHID6 = 6       # the planted encoder defects: (kind, ehid, col) at the SMALL dims
# name -> (dims, clamp inputs, leg, model flags of the case it belongs to, plant, parts that must fail[, (enc, ehid, col)])
DEFECTS = {
    "one cell's state not updated": (SMALL, 0, GEN_, {}, _patched("_carry", lambda new, old, k, n: old if (k, n) == (1, 2) else new),
                                     ("h[1][2]", "x[3]")),
    "state of step k read from step k - 1": (SMALL, 0, GEN_, {}, _patched("_state_in", lambda st, k, n: st[max(k - 1, 0)]),
                                             ("h[1][1]", "x[1]")),
    "zero state used at the second frame": (SMALL, 0, OBS_, {}, _patched("_state_in", lambda st, k, n: tuple(torch.zeros_like(v) for v in st[k])
                                                                        if n == 1 else st[k]), ("h[0][1]", "z[1]")),
    "one row of the last tile left stale": (SMALL, 0, GEN_, {}, _stale_row, ("x.tail[2]", "h.tail[1][2]")),
    "the window taken one frame late": (SMALL, 0, OBS_, {}, _patched("_window", lambda f, t, h1: f[:, t - h1 + 1:t + 1].reshape(f.shape[0], -1)),
                                        ("c[0]", "z[0]")),
    "the pass-through half swapped": (SMALL, 0, GEN_, {}, _swap_halves, ("x[0]", "h[0][0]")),
    "b_hn outside r * (.)": (SMALL, 0, GEN_, {}, _patched("_gru_candidate", lambda gi_n, r, gh_n, b_n, tanh: tanh(gi_n + r * (gh_n - b_n) + b_n),
                                                          fr), ("h[1][0]", "x[0]")),
    "reverse coupling as (z2 - shift) / scale": (SMALL, 0, GEN_, {}, _patched("_uncouple", lambda z2n, shift, scale: (z2n - shift) / scale),
                                                 ("x[0]", "h[0][0]")),
    "the clamp missing in the reverse direction": (CLAMPED, 1, GEN_, {}, _patched("_clamp_scale_rev", lambda s, eps: s), ("x[0]", "nll[0]")),
    "the constant log-det term missing from nll": (SMALL, 0, GEN_, {}, _patched("_nll", lambda const, ld, z: -(ld + (-0.5 * (z ** 2 + fq.LOG2PI)).sum(dim=1)) / fq.LN2),
                                                   ("nll[0]", "nll[3]")),
    "the lo x hi product dropped from a three-product cell": (SMALL, 0, GEN_, X3, _patched("_prod3h", _two_products), ("h[1][0]", "x[0]")),
    "an absent row's state advanced": (SMALL, 0, RAG_, {}, _patched("_keep_absent", lambda new, old, absent: new), ("h[0][3]", "h.tail[1][3]")),
    "an observing row given the generated frame": (SMALL, 0, MIX_, {}, _patched("_frame_in", lambda given, generated, gen_rows: generated),
                                                   ("x.obs[1]", "x[1]")),
    # ---- the window behind an encoder (the first frame has no earlier one to carry a state from: that defect shows from frame 1)
    "enc: state carried from the previous frame": (SMALL, 0, GEN_, {}, _patched("_enc_state0", lambda last, zero: zero if last is None else last),
                                                   ("c[1]", "x[1]"), ("rnn", EHID6, 0)),
    "enc: window fed newest-first": (SMALL, 0, OBS_, {}, _patched("_enc_window", lambda f, t, h1: f[:, t - h1:t].flip(1)),
                                     ("c[0]", "z[0]"), ("rnn", EHID6, 0)),
    "enc: features from the step before the last": (SMALL, 0, GEN_, {}, _patched("_enc_features", lambda hseq: hseq[-2]),
                                                    ("c[0]", "x[0]"), ("rnn", EHID6, 0)),
    "enc: the mlp's LeakyReLU missing": (SMALL, 0, OBS_, {}, _patched("_enc_mlp_act", lambda y: y), ("c[0]", "z[0]"), ("mlp", EHID6, 0)),
    "enc: wct columns from col + 1": (SMALL, 0, GEN_, {}, _patched("_enc_cols", lambda wct, col, ehid: wct[:, col + 1:col + 1 + ehid]),
                                      ("c[0]", "x[0]"), ("rnn", EHID6, 3)),
    "enc: wct columns from 0 although col != 0": (SMALL, 0, OBS_, {}, _patched("_enc_cols", lambda wct, col, ehid: wct[:, :ehid]),
                                                  ("c[0]", "z[0]"), ("mlp", EHID6, 3)),
    "enc: LSTM gate blocks read as i, f, o, g": (SMALL, 0, GEN_, {}, _lstm_gates_ifog, ("c[0]", "x[0]"), ("lstm", EHID6, 3)),
    "enc: the window taken one frame late": (SMALL, 0, OBS_, {}, _patched("_enc_window", lambda f, t, h1: f[:, t - h1 + 1:t + 1]),
                                             ("c[0]", "z[0]"), ("rnn", EHID6, 3)),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_defect_is_rejected(name, monkeypatch):
    d, clamp, leg, flags, plant, where = DEFECTS[name][:6]
    enc, ehid, col = DEFECTS[name][6] if len(DEFECTS[name]) > 6 else ("none", 0, 0)
    inp = fq.make_frame_inputs(d, HIST1, seed=9, clamp=bool(clamp), enc=enc, ehid=ehid, col=col)
    g = torch.Generator().manual_seed(3)
    frames = torch.randn(d.N, d.B, d.C, generator=g)          # what observing rows are given (the mixed run: frames of their own)
    roles = {GEN_: fq.roles_all(d, fq.GEN), OBS_: fq.roles_all(d, fq.OBS), MIX_: _mixed_roles(d),
             RAG_: fq.roles_ragged(d, [[0, d.N, 1, 2][b % 4] for b in range(d.B - 1)] + [1])}[leg]
    given = None if leg == GEN_ else frames
    exact, fp32 = fq.run_exact(inp, d, roles, given=given), fq.run_exact(inp, d, roles, torch.float32, given=given)
    model = fq.run_model(inp, d, roles, given=given, **flags)
    clean = fq.run_model(inp, d, roles, given=given, **flags) if flags else fp32
    assert not fq.failures(fq.compare(clean, exact, model, fp32, d, roles))
    if clamp:
        frac = float((exact["raw_scale"] < d.scale_eps).double().mean())
        assert 0.2 < frac < 0.8
    bad = plant(clean, inp, d, roles, given, flags, monkeypatch)
    monkeypatch.undo()
    rows = fq.compare(bad, exact, model, fp32, d, roles)
    failed = {n for n, e, a, ok in rows if not ok}
    assert failed, "the defect went unnoticed: " + name
    for part in where:
        assert part in failed, (name, part, sorted(failed))
    by = {n: (e, a) for n, e, a, ok in rows}
    for part in where:
        e, a = by[part]
        print("%s: %s %.2e against %.2e allowed" % (name, part, e, a))
        assert e > 10 * a, (name, part, e, a)      # rejected by a margin, not by noise


def test_bound_rejects_nonfinite_and_missing_parts():
    d = SMALL
    inp = fq.make_frame_inputs(d, HIST1, seed=1)
    roles = fq.roles_all(d, fq.GEN)
    exact, fp32, model = fq.run_exact(inp, d, roles), fq.run_exact(inp, d, roles, torch.float32), fq.run_model(inp, d, roles)
    x = fp32["x"].clone()
    x[0, 3, 1] = float("nan")
    failed = {n for n, e, a, ok in fq.compare(dict(fp32, x=x), exact, model, fp32, d, roles) if not ok}
    assert failed == {"x[0]"}
    # a run that holds only the final state is compared on that state, and on every frame it has
    part = dict(fp32, z=None, c=None, state_frames=[d.N - 1])
    names = [n for n, e, a, ok in fq.compare(part, exact, model, fp32, d, roles)]
    assert "h[0][%d]" % (d.N - 1) in names and "h[0][0]" not in names and "c[0]" not in names and "x[0]" in names


# ------------------------------------------------------------------------------------------ (f) which kernels a call takes
def test_frame_plan_of_every_case(monkeypatch):
    """lfi_flow_frame_plan and lfi_flow_score_chunk_ok for every GPU case under its switches, against the case table's `expect` column
    (derived by hand from flow_frame_plan in lfi_flow_cells.h). Host only."""
    from lets_face_it_amd import _lib
    L = _lib.lib()
    for c in gd.CASES:
        for k in gd.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in c.env.items():
            monkeypatch.setenv(k, v)
        dims = gd.flow_dims(c)
        assert int(L.lfi_flow_frame_plan(C.byref(dims))) == c.expect, c.id
        assert bool(L.lfi_flow_score_chunk_ok(C.byref(dims))) == bool(c.expect & 2), c.id
        assert c.Ks * -(-c.B // 16) <= 64
        fused = c.p == 9 and c.D == 512 and (3 + c.lstm) * c.H in (384, 512) and c.env.get("LFI_SAMPLE_FUSED") != "0" and c.enc == "none"
        assert (c.front == gd.FUSED) == fused, c.id      # lfi_sample.hip, lfi_internal_sample_cond_ok, and SampleFront's precision rule
        # the window-encoder kernel of a recurrent kind, for the per-frame legs' B windows and the chunk legs' N B: the `evar` column
        # (by hand from enc_plan_fwd in lfi_encoder_common.h)
        if c.enc in ("rnn", "lstm"):
            assert gd.enc_variants(L, c) == [c.evar, c.evar], (c.id, gd.enc_variants(L, c))
        else:
            assert c.evar is None, c.id
    assert L.lfi_flow_frame_plan(None) == 0
