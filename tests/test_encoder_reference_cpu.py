"""tests/encoder_reference.py checked on the CPU: the window reference against torch.nn.GRU / torch.nn.LSTM themselves, the arithmetic
model with every flag off against the autograd reference, and the comparison routine of the GPU kernel tests against planted errors -
the evidence that its gates would notice a subtly wrong kernel. (ModalityEncoder, glow/models.py:55-80.)"""
import pytest
import torch

import encoder_reference as er
from encoder_reference import Dims
from helpers import rel_l2

# (hid, hist, B, N, start, col, dup): hist 1; pos0 = start - hist + 1 = 0; dup 1
SHAPES = [(8, 1, 3, 4, 2, 0, 0), (12, 5, 2, 6, 4, 3, 0), (6, 3, 4, 5, 5, 2, 1)]


def _dims(shape):
    hid, hist, B, N, start, col, dup = shape
    return Dims(B, start + N + 2, N, start, hist, hid, col, dup)


@pytest.mark.parametrize("lstm", [False, True])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_windows_forward_is_torch_rnn(shape, masked, lstm):
    """windows_forward in fp64 against nn.GRU / nn.LSTM(batch_first=True) run on the gathered windows: the input projection is applied
    outside (W_ih = identity, so the module's input IS mask * Xp[row]) and the mask to the input. Forward and all four gradients to
    1e-12 relative."""
    dims = _dims(shape)
    hid, G, F = dims.hid, (4 if lstm else 3) * dims.hid, dims.N * dims.B
    inp = er.make_inputs(dims, lstm=lstm, masked=masked, seed=11, ldcond=dims.col + 2 * hid + 3)
    ours = er.run_autograd(inp, dims, torch.float64, lstm)

    rnn = (torch.nn.LSTM if lstm else torch.nn.GRU)(G, hid, batch_first=True).double()
    leaves = {k: inp[k].double().clone().requires_grad_(True) for k in ("Xp", "whh", "b_ih", "b_hh")}
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(torch.eye(G, dtype=torch.float64))
    # the module's own parameters are replaced by our leaves through the functional call, so autograd reaches them
    x = leaves["Xp"][er.window_rows(dims)]                                  # (F, hist, G)
    if masked:
        x = x * inp["mask"].double().unsqueeze(-1)
    params = {"weight_ih_l0": torch.eye(G, dtype=torch.float64), "weight_hh_l0": leaves["whh"], "bias_ih_l0": leaves["b_ih"],
              "bias_hh_l0": leaves["b_hh"]}
    seq, hn = torch.func.functional_call(rnn, params, (x,))
    h_n = hn[0][0] if lstm else hn[0]
    assert torch.equal(seq[:, -1], h_n)
    feats = torch.cat([seq[:, -1], h_n], dim=1) if dims.dup else h_n        # cat(seq[:, -1], h_n[0]) or its folded form
    (feats * inp["dcond"].double()[:, dims.col:dims.col + hid * (1 + dims.dup)]).sum().backward()
    assert ours["features"].shape == (F, hid * (1 + dims.dup)) and ours["hseq"].shape == (dims.hist, F, hid)
    assert rel_l2(ours["features"], feats.detach()) < 1e-12
    assert rel_l2(ours["hseq"], seq.detach().transpose(0, 1)) < 1e-12
    for key, leaf in (("dXp", "Xp"), ("dW_hh", "whh"), ("db_ih", "b_ih"), ("db_hh", "b_hh")):
        assert rel_l2(ours[key], leaves[leaf].grad) < 1e-12, key
    # rows no window reads get no gradient: the T = start + N + 2 layout leaves some
    read = torch.zeros(dims.B * dims.T, dtype=torch.bool)
    read[er.window_rows(dims).reshape(-1)] = True
    assert not bool(read.all()) and bool((ours["dXp"][~read] == 0).all())


@pytest.mark.parametrize("lstm", [False, True])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_model_without_flags_is_the_reference(shape, masked, lstm):
    """The hand-written BPTT of the arithmetic model with every rounding off: every part of the run to 1e-12 of autograd's."""
    dims = _dims(shape)
    inp = er.make_inputs(dims, lstm=lstm, masked=masked, seed=5)
    exact = er.run_autograd(inp, dims, torch.float64, lstm)
    model = er.run_model(inp, dims, lstm=lstm)
    for (name, m), (_, e) in zip(er.pieces(model, dims.hid), er.pieces(exact, dims.hid)):
        assert rel_l2(m, e) < 1e-12, name
    # dW_hh at hist 1 has no term: the exact-zero rule
    if dims.hist == 1:
        assert float(exact["dW_hh"].abs().max()) == 0.0 and rel_l2(model["dW_hh"], exact["dW_hh"]) == 0.0


def test_model_flags_round_what_they_say():
    """Each flag moves the model away from the reference by about the precision it names, and only the parts it touches."""
    dims = Dims(3, 12, 5, 5, 4, 16, 0, 0)
    inp = er.make_inputs(dims, seed=2)
    exact = er.run_autograd(inp, dims)
    e3 = dict((n, rel_l2(m, e)) for (n, m), (_, e) in zip(er.pieces(er.run_model(inp, dims, three_products=True), 16), er.pieces(exact, 16)))
    assert e3["hseq[0]"] == 0.0 and 0 < e3["features"] < 1e-4          # no product at step 0; ~2^-16 after
    g = dict((n, rel_l2(m, e)) for (n, m), (_, e) in zip(er.pieces(er.run_model(inp, dims, grads_bf16=True), 16), er.pieces(exact, 16)))
    assert g["features"] == 0.0 and g["db_ih"] < 1e-12 and 1e-4 < g["dgh[3]"] < 4e-3 and 1e-5 < g["dXp"] < 4e-3
    h = dict((n, rel_l2(m, e)) for (n, m), (_, e) in zip(er.pieces(er.run_model(inp, dims, stash_f16=True), 16), er.pieces(exact, 16)))
    assert h["features"] == 0.0 and h["hseq[3]"] < 1e-15 and 1e-5 < h["dgi[3]"] < 1e-3
    t = dict((n, rel_l2(m, e)) for (n, m), (_, e) in zip(er.pieces(er.run_model(inp, dims, two_products=True), 16), er.pieces(exact, 16)))
    assert t["dgh[3]"] < 1e-15 and 1e-4 < t["dgh[2]"] < 4e-3             # the last step's derivatives see no product
    b = dict((n, rel_l2(m, e)) for (n, m), (_, e) in zip(er.pieces(er.run_model(inp, dims, three_products=True, bwd_exact=True), 16),
                                                         er.pieces(exact, 16)))
    assert 0 < b["dgh[0]"] <= e3["dgh[0]"] * 1.5


# ---- planted errors: a correct run with ONE defect must fail compare(); the clean run must pass it. Two stand-ins for a correct
# kernel: the reference in fp32 (bounds of fp32 size, as the exact-f32 kernels get) and the arithmetic model with the training step's
# flags (bounds of bf16 size on the gradient stashes, as the two-product kernels get)
TRAINING = dict(three_products=True, two_products=True, grads_bf16=True, stash_f16=True, fast_gates=True)


def _derived(run, inp, dims, rerun):
    """Re-derive what the GPU harness derives from the stashes (dW_hh) after a defect touched them."""
    run = dict(run)
    run["dW_hh"] = er.dwhh_from_stashes(run["dgh"], run["hseq"])
    return run


def _ragged_bias(run, inp, dims, rerun):
    """A 64-window workgroup whose rows past F recompute the last window (w = min(wbase + i, F - 1)) and ALSO sums them into bias_part."""
    F = dims.N * dims.B
    extra = -F % 64
    assert extra > 0
    run = dict(run)
    run["db_ih"] = run["db_ih"] + extra * run["dgi"][:, F - 1].sum(0)
    run["db_hh"] = run["db_hh"] + extra * run["dgh"][:, F - 1].sum(0)
    return run


def _mask_dropped(run, inp, dims, rerun):
    m = inp["mask"].clone()
    m[:, 1] = 1.0
    return rerun(dict(inp, mask=m))


def _unit_left_zero(run, inp, dims, rerun):
    run = dict(run, hseq=run["hseq"].clone(), features=run["features"].clone())
    run["hseq"][:, :, 3] = 0.0
    run["features"][:, 3] = 0.0
    return _derived(run, inp, dims, rerun)


def _halves_not_summed(run, inp, dims, rerun):
    assert dims.dup == 1
    dc = inp["dcond"].clone()
    dc[:, dims.col + dims.hid:dims.col + 2 * dims.hid] = 0.0
    return dict(rerun(dict(inp, dcond=dc)), features=run["features"], hseq=run["hseq"])


def _row_missing(run, inp, dims, rerun):
    run = dict(run, dXp=run["dXp"].clone())
    run["dXp"][int(er.window_rows(dims)[7, 1])] = 0.0
    return run


DEFECTS = {"ragged rows summed into the bias gradients": (_ragged_bias, ("db_ih", "db_hh")),
           "mask dropped at one history step": (_mask_dropped, ("features", "hseq[1]", "dXp")),
           "one hidden unit's state left at zero": (_unit_left_zero, ("features", "hseq[0]")),
           "dcond halves not summed under dup 1": (_halves_not_summed, ("dgh[2]", "dXp", "db_hh")),
           "one frame row missing from the scatter": (_row_missing, ("dXp",))}


@pytest.fixture(scope="module", params=["fp32", "training"])
def planted(request):
    """fp32: the tilings test's ragged case in small - B = 250 -> F = 14 000 = 218 * 64 + 48 windows, the case whose bias gate sits
    at 1e-3 today. training: the GPU cases' F = 8130 = 127 * 64 + 2. hist 3, hid 32, dup 1.
    -> dims, inputs, exact, fp32, model (the bound's two terms), clean run, how to run it again on other inputs."""
    dims = Dims(250, 60, 56, 2, 3, 32, 4, 1) if request.param == "fp32" else Dims(271, 34, 30, 2, 3, 32, 4, 1)
    inp = er.make_inputs(dims, seed=7)
    exact = er.run_autograd(inp, dims, torch.float64)
    fp32 = er.run_autograd(inp, dims, torch.float32)
    if request.param == "fp32":
        return dims, inp, exact, fp32, er.run_model(inp, dims), fp32, lambda i: er.run_autograd(i, dims, torch.float32)
    model = er.run_model(inp, dims, **TRAINING)
    return dims, inp, exact, fp32, model, model, lambda i: er.run_model(i, dims, **TRAINING)


def test_clean_run_passes(planted):
    dims, inp, exact, fp32, model, clean, rerun = planted
    rows = er.compare(_derived(clean, inp, dims, rerun), exact, model, fp32, dims.hid)
    assert not er.failures(rows), er.failures(rows)
    assert all(a > 0 for n, e, a, ok in rows), "a zero allowance would make this test vacuous"
    # the allowances are of the size of the arithmetic: fp32 / bf16 (2^-9) - nothing like the 1e-2 of an absolute gate
    assert max(a for n, e, a, ok in rows) < (1e-5 if clean is fp32 else 8e-3)


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_planted_error_is_rejected(planted, name):
    dims, inp, exact, fp32, model, clean, rerun = planted
    plant, where = DEFECTS[name]
    rows = er.compare(plant(clean, inp, dims, rerun), exact, model, fp32, dims.hid)
    failed = {n for n, e, a, ok in rows if not ok}
    assert failed, "the defect went unnoticed: " + name
    for part in where:
        assert part in failed, (name, part, sorted(failed))
    # ... and not by noise. Against fp32-sized bounds the worst part misses by more than 100 x. Against the bf16-sized bounds of the
    # training arithmetic every defect still fails, the narrowest being ONE missing row among the 9214 of dXp (8.3e-3 against 5.1e-3:
    # a whole-tensor L2 sees a single row as 1 / sqrt(rows)) - the GPU cases on few rows (group A) are where that defect shows
    n, e, a = er.worst(rows)
    print("%s: %s %.2e against %.2e allowed" % (name, n, e, a))
    assert e > (100 if clean is fp32 else 1.5) * a, (name, n, e, a)


def test_bound_rejects_nonfinite_and_nonzero_where_zero_is_exact():
    dims = Dims(2, 8, 3, 3, 1, 8, 0, 0)          # hist 1: dW_hh is exactly 0
    inp = er.make_inputs(dims, seed=1)
    exact, fp32, model = er.run_autograd(inp, dims), er.run_autograd(inp, dims, torch.float32), er.run_model(inp, dims)
    assert not er.failures(er.compare(fp32, exact, model, fp32, dims.hid))
    bad = dict(fp32, dW_hh=fp32["dW_hh"].clone())
    bad["dW_hh"][5, 2] = 1e-30
    assert any(n.startswith("dW_hh[0]") for n, e, a, ok in er.compare(bad, exact, model, fp32, dims.hid) if not ok)
    bad = dict(fp32, dXp=fp32["dXp"].clone())
    bad["dXp"][0, 0] = float("nan")
    assert "dXp" in {n for n, e, a, ok in er.compare(bad, exact, model, fp32, dims.hid) if not ok}
