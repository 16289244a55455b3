"""Every kernel behind lfi_flow_seq_fwd / lfi_flow_seq_bwd(_planes) / lfi_flow_param_grads against an fp64 flow written from the
definition (tests/flow_reference.py), through the C ABI in the order engine.forward / backward / _backward_chain call it - lfi_flow_prep,
the forward walk, the backward walk, the parameter gradients - with an error per (flow step, timestep) cell, per gate block and for
the rows of the last batch tile on their own. (FlowStep.normal_flow, glow/models.py:311-342; f_seq.forward :204-214.)

Bound, for every case and every part, every error a relative L2 with no floor against the fp64 autograd run:

    err(kernel) <= 3 * err(model run with the flags that describe the case's kernels) + 8 * err(reference in torch fp32)

Which kernels a case reaches is asserted with lfi_flow_walk_variant before anything is launched (codes: 0 generic diagonal cells,
1 register-resident diagonal cells, 2 persistent walk f32, 3 persistent walk bf16x3; thin products 0 four split-K products, 1 one
pass): a case that lands elsewhere fails. Every buffer has exactly the size its *_floats query returns, between two guard bands.

What the walks do not hold: the gradient of the frames (dx of flow step 0) is never written - frames are data. It is derived here
in fp64 from the dy the backward walk leaves for step 0, dx[0] = (dy[0] W^T) exp(an_logs); dx of every later step is read as written.
"""
import ctypes as C
from collections import namedtuple

import pytest
import torch

import flow_reference as fr
from helpers import report

pytestmark = pytest.mark.gpu

SWITCHES = ("LFI_FLOW_PIPE", "LFI_PIPE_X3", "LFI_FLOW_GENERIC", "LFI_FLOW_WGRAD_FUSED", "LFI_FLOW_WGRAD_IH", "LFI_PIPE_FENCE",
            "LFI_PIPE_FORCE_ABORT")
G_, F_, P_, X_ = 0, 1, 2, 3       # walk codes
FOUR, ONE = 0, 1                  # thin products

Case = namedtuple("Case", "id C H Ks B N start D affine lstm dense p planes g16 two env acc clamp expect")


def case(id, C, H, Ks, B, N, expect, start=0, D=20, affine=1, lstm=0, dense=0, p=1, planes=None, g16=0, two=0, env=None, acc=0, clamp=0):
    """planes: None (lfi_flow_seq_bwd) | 'two' (hi + lo planes) | 'hi' (hi_only). expect: (forward walk, backward walk, thin products)."""
    return Case(id, C, H, Ks, B, N, start, D, affine, lstm, dense, p, planes, g16, two, env or {}, acc, clamp, expect)


FINAL = dict(C=50, H=128, Ks=3, B=33, N=5, start=2)            # final_model.yaml's cell, two full batch tiles + one row, frames behind
FINAL32 = dict(C=50, H=128, Ks=3, B=32, N=13)                  # wgrad_splits: two timestep ranges, 7 + 6
ONEPASS = dict(planes="hi", g16=1, two=1)
CASES = [
    case("final-x3", expect=(X_, X_, FOUR), **FINAL),
    case("final-x3-acc", expect=(X_, X_, FOUR), acc=1, **FINAL),
    case("final-p0", expect=(P_, P_, FOUR), p=0, **FINAL),
    case("final-x3off", expect=(P_, P_, FOUR), env={"LFI_PIPE_X3": "0"}, **FINAL),
    case("final-diag", expect=(F_, F_, FOUR), p=0, env={"LFI_FLOW_PIPE": "0"}, **FINAL),
    case("final-generic-p0", expect=(G_, G_, FOUR), p=0, env={"LFI_FLOW_GENERIC": "1"}, **FINAL),
    case("final-generic-p1", expect=(G_, G_, FOUR), env={"LFI_FLOW_GENERIC": "1"}, **FINAL),
    case("clamp", expect=(P_, P_, FOUR), p=0, clamp=1, **FINAL),
    case("clamp-x3", expect=(X_, X_, FOUR), clamp=1, **FINAL),
    case("final-planes", expect=(X_, X_, FOUR), planes="two", **FINAL32),
    case("final-onepass", expect=(X_, X_, ONE), **ONEPASS, **FINAL32),
    case("final-onepass-acc", expect=(X_, X_, ONE), acc=1, **ONEPASS, **FINAL32),
    case("final-onepass-off", expect=(X_, X_, FOUR), env={"LFI_FLOW_WGRAD_FUSED": "0"}, **ONEPASS, **FINAL32),
    case("final-onepass-n1", 50, 128, 3, 32, 1, (X_, X_, ONE), **ONEPASS),
    case("c64-onepass", 64, 128, 2, 32, 9, (X_, X_, ONE), **ONEPASS),
    case("h120", 50, 120, 2, 17, 4, (X_, X_, FOUR)),                       # H16 = 128: eight padding hidden units
    case("h96-planes", 34, 96, 2, 32, 4, (X_, X_, FOUR), planes="two", g16=1, two=1),
    case("h32", 50, 32, 2, 17, 4, (X_, P_, FOUR)),                         # NG * H16 = 96 < 128: the backward walk stays f32
    case("odd", 15, 24, 4, 6, 4, (P_, P_, FOUR), dense=1),
    case("h44", 50, 44, 3, 8, 4, (P_, P_, FOUR)),
    case("additive", 50, 128, 2, 17, 4, (X_, X_, FOUR), affine=0),
    case("lstm", 50, 64, 2, 17, 4, (P_, P_, FOUR), lstm=1),
    case("lstm-diag", 50, 64, 2, 17, 4, (F_, F_, FOUR), lstm=1, env={"LFI_FLOW_PIPE": "0"}),
    case("h160", 50, 160, 2, 5, 3, (G_, G_, FOUR), p=0),
    case("tiles", 50, 128, 3, 271, 3, (X_, X_, FOUR)),                     # 17 batch tiles, the last one 15 rows
    case("n1-k1", 50, 128, 1, 1, 1, (X_, X_, FOUR)),
]
SEED = 4      # the clamp cases' conditions hold at this seed (tests/test_flow_reference_cpu.py checks them)


def ref_dims(c):
    return fr.Dims(c.B, c.start + c.N + 3, c.N, c.start, c.C, c.H, c.D, c.Ks, c.affine, c.lstm, fr.CLAMP_EPS if c.clamp else fr.EPS)


def flow_dims(c, extra_bits=0):
    from lets_face_it_amd._lib import FlowDims
    d = ref_dims(c)
    return FlowDims(c.B, c.N, c.C, c.H, c.D, c.Ks, c.affine, c.lstm, d.scale_eps, c.p | extra_bits)


def case_bits(c):
    """gemm_precision of (the backward walk, lfi_flow_param_grads) - the bits engine._backward_chain sets."""
    g16 = (1 << 16) if c.g16 else 0
    return g16, (0x100 if c.two else 0) | g16


def model_flags(c):
    """The roundings the case's kernels document, by the variant each call is expected to take."""
    fwd, bwd, thin = c.expect
    flags = dict(fast_gates=True, w_fp32=True, x3_fwd=fwd == X_, x3_bwd=bwd == X_)
    if c.g16:
        flags["rows_bf16"] = True
    if c.two and (c.p & 1):
        flags["two_products"] = True
    elif c.p & 1:
        flags["three_products"] = True
    return flags


_gpu_error = []
_refs = {}      # one input set's references at a time (the cases of a shape are neighbours in CASES)


def _references(c, dev):
    d = ref_dims(c)
    key = (d, c.dense, c.clamp)
    if key not in _refs:
        _refs.clear()
        inp = fr.make_inputs(d, dense=bool(c.dense), seed=SEED, device=dev, clamp=bool(c.clamp))
        _refs[key] = {"inp": inp, "exact": fr.run_autograd(inp, d, torch.float64), "fp32": fr.run_autograd(inp, d, torch.float32),
                      "models": {}}
    return _refs[key]


def _model(ref, d, flags):
    key = tuple(sorted(flags.items()))
    if key not in ref["models"]:
        ref["models"][key] = fr.run_model(ref["inp"], d, **flags)
    return ref["models"][key]


GUARD = 64          # floats on either side (256 bytes: the interior keeps the allocation's alignment)
PATTERN = 7.0


class Guarded:
    """n floats between two guard bands of PATTERN; the interior starts as `fill`."""

    def __init__(self, n, dev, fill=0.0):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, device=dev)
        self.t = self.buf[GUARD:GUARD + self.n]
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.n:] == PATTERN).all())


def _part(L, fn, dims, g, which, shape):
    """A view of one region of a stash through lfi_flow_stash_ptr / lfi_flow_bstash_ptr."""
    p = fn(C.byref(dims), g.ptr(), which)
    assert p, "stash pointer %d" % which
    off = (p - g.ptr()) // 4
    n = 1
    for s in shape:
        n *= s
    assert 0 <= off and off + n <= g.n, ("stash region outside the buffer", which, off, n, g.n)
    return g.t[off:off + n].view(*shape)


def run_case(c, dev, monkeypatch):
    from lets_face_it_amd import _lib
    from lets_face_it_amd._lib import FlowGrads, FlowParams, check
    L = _lib.lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    d = ref_dims(c)
    Ch, C2, Cout, NG, G, I = fr.derived(d)
    B, N, Ks, H, Cc, T = c.B, c.N, c.Ks, c.H, c.C, d.T
    F = N * B
    ldc, ldo = (Cc + 3) & ~3, (Cout + 3) & ~3
    assert Ks * -(-B // 16) <= 64, "the persistent walks must be co-resident many times over"
    bwd_bits, pg_bits = case_bits(c)
    dims, bdims, pgdims = flow_dims(c), flow_dims(c, bwd_bits), flow_dims(c, pg_bits)

    # ---- the kernels these calls take, before anything is launched
    got_variant = (int(L.lfi_flow_walk_variant(C.byref(dims), 0)), int(L.lfi_flow_walk_variant(C.byref(bdims), 1)),
                   int(L.lfi_flow_walk_variant(C.byref(pgdims), 2)))
    assert got_variant == c.expect, ("kernels", got_variant, c.expect)
    if c.planes:
        assert L.lfi_flow_bwd_emits_planes(C.byref(bdims)), "planes refused"

    ref = _references(c, dev)
    inp, exact, fp32 = ref["inp"], ref["exact"], ref["fp32"]
    model = _model(ref, d, model_flags(c))
    par = {k: v.contiguous() for k, v in inp["params"].items()}
    p = FlowParams()
    for name, t in par.items():
        setattr(p, name, t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    x0, gic, cmat = inp["x0"].contiguous(), inp["gic"].contiguous(), inp["c"].contiguous()
    gscale = float(inp["gscale"])

    # ---- prep, forward walk
    prep = Guarded(L.lfi_flow_prep_floats(C.byref(dims)), dev)
    stash = Guarded(L.lfi_flow_stash_floats(C.byref(dims)), dev)
    z, nll = Guarded(F * Cc, dev, float("nan")), Guarded(F, dev, float("nan"))
    check(L.lfi_flow_prep(C.byref(dims), C.byref(p), prep.ptr(), 0, st), "prep")
    check(L.lfi_flow_seq_fwd(C.byref(dims), C.byref(p), prep.ptr(), x0.data_ptr(), T, c.start, gic.data_ptr(), stash.ptr(), z.ptr(),
                             nll.ptr(), st), "fwd")
    torch.cuda.synchronize()
    if c.expect[0] >= P_:
        words = _part(L, L.lfi_flow_stash_ptr, dims, stash, 8, (2,)).view(torch.int32)
        assert int(words[1]) == 0, "the forward walk was abandoned"

    # ---- backward walk
    bstash = Guarded(L.lfi_flow_bstash_floats(C.byref(bdims)), dev)
    planes = None
    if c.planes:
        n_pl = int(L.lfi_planes_elems(Ks * F, G))
        planes = Guarded((n_pl + 1) // 2, dev, PATTERN)
        check(L.lfi_flow_seq_bwd_planes(C.byref(bdims), C.byref(p), prep.ptr(), stash.ptr(), gscale, bstash.ptr(), planes.ptr(),
                                        1 if c.planes == "hi" else 0, st), "bwd planes")
    else:
        check(L.lfi_flow_seq_bwd(C.byref(bdims), C.byref(p), prep.ptr(), stash.ptr(), gscale, bstash.ptr(), st), "bwd")
    torch.cuda.synchronize()
    if c.expect[1] >= P_:
        words = _part(L, L.lfi_flow_bstash_ptr, bdims, bstash, 9, (2,)).view(torch.int32)
        assert int(words[1]) == 0, "the backward walk was abandoned"

    # ---- parameter gradients: overwritten (arrays start as PATTERN) or added to random values of the gradient's own size
    shapes = {k: tuple(v.shape) for k, v in exact["grads"].items()}
    garr, prefill = {}, {}
    gen = torch.Generator().manual_seed(17)
    for k, shp in shapes.items():
        n = 1
        for s in shp:
            n *= s
        garr[k] = Guarded(n, dev, PATTERN)
        if c.acc:
            rms = float(exact["grads"][k].pow(2).mean().sqrt())
            prefill[k] = (torch.randn(shp, generator=gen) * max(rms, 1e-6)).float().to(dev)
            garr[k].t.copy_(prefill[k].reshape(-1))
    g = FlowGrads()
    for k in shapes:
        setattr(g, k, garr[k].ptr())
    work = Guarded(L.lfi_flow_param_grads_work_floats(C.byref(pgdims)), dev)
    with_c = not c.g16      # bf16 rows: the caller runs dgi^T c on operand planes itself, lfi_flow_param_grads refuses c
    check(L.lfi_flow_param_grads(C.byref(pgdims), C.byref(p), prep.ptr(), stash.ptr(), bstash.ptr(), cmat.data_ptr() if with_c else None,
                                 Ks * c.D, gscale, C.byref(g), c.acc, work.ptr(), st, None), "param grads")
    torch.cuda.synchronize()

    # ---- every write stayed inside
    named = [("prep", prep), ("stash", stash), ("z", z), ("nll", nll), ("bstash", bstash), ("work", work)] + \
        [("grad " + k, v) for k, v in garr.items()] + ([("planes", planes)] if planes else [])
    for name, gb in named:
        assert gb.intact(), "guard band of " + name

    # ---- decode
    got = {"z": z.t.view(N, B, Cc), "nll": nll.t.view(N, B),
           "h": _part(L, L.lfi_flow_stash_ptr, dims, stash, 3, (Ks, N, B, H)),
           "x_out": _part(L, L.lfi_flow_stash_ptr, dims, stash, 2, (Ks, N, B, ldc))[..., :Cc]}
    assert torch.equal(got["z"], got["x_out"][Ks - 1]), "z is the last step's x_out"
    if c.g16:
        def rows(which):
            t = _part(L, L.lfi_flow_bstash_ptr, bdims, bstash, which, (Ks * F * G,))
            assert bool((t[(Ks * F * G + 1) // 2:] == 0).all()), "bf16 rows wrote past their half"
            return t.view(torch.bfloat16)[:Ks * F * G].float().view(Ks, N, B, G)
        got["dgi"], got["dgh"] = rows(1), rows(2)
    else:
        got["dgi"] = _part(L, L.lfi_flow_bstash_ptr, bdims, bstash, 1, (Ks, N, B, G))
        got["dgh"] = _part(L, L.lfi_flow_bstash_ptr, bdims, bstash, 2, (Ks, N, B, G))
    dx = _part(L, L.lfi_flow_bstash_ptr, bdims, bstash, 4, (Ks, N, B, ldc))[..., :Cc].double().clone()
    dy0 = _part(L, L.lfi_flow_bstash_ptr, bdims, bstash, 3, (Ks, N, B, ldc))[0, ..., :Cc].double()
    par64 = {k: v.double() for k, v in par.items()}
    W0, _ = fr._invconv(par64, 0, torch.float64)
    dx[0] = (dy0 @ W0.t()) * torch.exp(par64["an_logs"][0])
    got["dx"] = dx
    got["grads"] = {k: garr[k].t.view(shapes[k]) for k in shapes}
    skip = ()
    if not with_c:
        skip = ("[:, Ch:]",)
        untouched = got["grads"]["w_ih"][:, :, Ch:]
        assert torch.equal(untouched, prefill["w_ih"][:, :, Ch:] if c.acc else torch.full_like(untouched, PATTERN)), \
            "w_ih[:, Ch:] is the caller's product when c is NULL"

    # ---- planes: bit for bit what lfi_planes_from_f32 makes of the rows the same walk wrote
    if c.planes:
        rows32 = torch.cat([got["dgi"][k].reshape(F, G) for k in range(Ks)]).float().contiguous()
        ref_pl = Guarded((n_pl + 1) // 2, dev, PATTERN)
        check(L.lfi_planes_from_f32(rows32.data_ptr(), G, Ks * F, G, ref_pl.ptr(), st), "planes_from_f32")
        torch.cuda.synchronize()
        assert ref_pl.intact()
        blocks = (Ks * F // 32) * (G // 16)
        a = planes.t.view(torch.int16)[:blocks * 1024].view(blocks, 2, 512)
        b = ref_pl.t.view(torch.int16)[:blocks * 1024].view(blocks, 2, 512)
        assert torch.equal(a[:, 0], b[:, 0]), "hi planes"
        if c.planes == "two" and not c.g16:
            assert torch.equal(a[:, 1], b[:, 1]), "lo planes"
        if c.planes == "hi":
            assert bool((planes.t[:blocks * 512].view(blocks, 2, 256)[:, 1] == PATTERN).all()), "hi_only wrote lo planes"

    # ---- the comparison (accumulate: everything the arrays held before is part of the expected value)
    def shifted(run):
        if not c.acc:
            return run
        return dict(run, grads={k: run["grads"][k] + prefill[k].to(run["grads"][k].dtype) for k in run["grads"]})
    rows_ = fr.compare(got, shifted(exact), shifted(model), shifted(fp32), d, skip=skip)
    summary = {}
    for name, e, a, ok in rows_:
        k = name.split("[")[0]
        ratio = (e / a) if a > 0 else (0.0 if e == 0 else float("inf"))
        if k not in summary or ratio >= summary[k][0]:
            summary[k] = (ratio, e, a, name)
    report("flow-walk %-18s %s  %s" % (c.id, "".join("GFPX"[v] for v in c.expect[:2]) + ("1" if c.expect[2] else "4"), "  ".join(
        "%s %.1e/%.1e" % (v[3], v[1], v[2]) for k, v in sorted(summary.items()))))
    if c.N == 1:
        assert float(exact["grads"]["w_hh"].abs().max()) == 0.0      # ... so compare() asked for exact zeros (or the prefill)
    assert not fr.failures(rows_), (c.id, fr.failures(rows_))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_flow_walk_vs_fp64(gpu_device, monkeypatch, c):
    """One case of the list above: kernels asserted, writes in bounds, walks not abandoned, every part within 3 x model + 8 x fp32 of
    the fp64 reference."""
    if _gpu_error:
        pytest.fail("not run: an earlier case ended in a GPU error (%s)" % _gpu_error[0])
    try:
        run_case(c, gpu_device, monkeypatch)
    except AssertionError:
        raise
    except Exception as e:      # a HIP error is sticky: launch nothing more on this device from this module
        _gpu_error.append("%s: %s" % (c.id, str(e)[:200]))
        raise


def test_case_list_covers_the_table():
    """The list itself: every walk code in both directions, both forms of the thin products, both plane forms, bf16 rows, both
    accumulate modes on both thin forms, a ragged last tile behind full ones, start > 0, C = 64, N = 1."""
    assert {c.expect[0] for c in CASES} == {G_, F_, P_, X_} and {c.expect[1] for c in CASES} == {G_, F_, P_, X_}
    assert {(c.expect[2], c.acc) for c in CASES} >= {(FOUR, 0), (FOUR, 1), (ONE, 0), (ONE, 1)}
    assert {c.planes for c in CASES} == {None, "two", "hi"} and any(c.g16 and c.expect[2] == FOUR for c in CASES)
    assert any(c.B > 32 and c.B % 16 == 1 for c in CASES) and any(c.start > 0 for c in CASES) and any(c.C == 64 for c in CASES)
    assert any(c.N == 1 and c.expect[2] == ONE for c in CASES) and any(c.expect[0] != c.expect[1] for c in CASES)
    assert all(c.Ks * -(-c.B // 16) <= 64 for c in CASES)
