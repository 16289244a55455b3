"""Every kernel behind lfi_encode_windows_fwd / _bwd / _scatter against an fp64 GRU / LSTM written from the definition
(tests/encoder_reference.py), through the C ABI in the order engine._encoder_backward calls it, with an error measure per history
step. (ModalityEncoder, glow/models.py:55-80.)

Bound, for every case and every part (features; hseq, dgi, dgh per history step; dXp; dW_hh per gate block; db_ih; db_hh), every
error a relative L2 against the fp64 autograd run:

    err(kernel) <= 3 * err(model run with the flags that describe the case's kernels) + 8 * err(reference in torch fp32)

Which case reaches which kernel (asserted per case with the ABI's own queries: a case that lands elsewhere fails):

  forward   0 unfused loop            C/gru320-*            LSTM loop  C/lstm*
            1 accumulator layout      exact f32: A/*-p0*;  bf16x3: A/h50-*, A/col6-*, A/unaligned, A/wide0; no stash: A/fwd-h50-*
            2 32-window row layout    A/*-p1* (hid % 4 == 0, aligned); no stash: A/fwd-h128-*; 255 groups: B/r64off
            3 64-window 32x32x16      B/m16off*, B/h192-*, B/h128-*, B/h64-*; no stash: B/fwd-m16off-*
            4 64-window 16x16x32      B/v4-*, B/h252-*, B/hist1, B/hist5; no stash: B/fwd-t16off-*
            5 epilogue under MFMAs    no stash (default): B/fwd-v5-*; with a stash (LFI_ENC_T16=2): B/v5-*
  backward  accumulator layout        A/*-p0*, A/h50-*, A/col6-*, A/widebwd0
            32-window row layout      A/*-p1*, A/wide0, A/unaligned, B/r64off   (<two products, fp16 stash> = <1,1> <0,0> <0,1> <1,0> in A/h256-* and A/h128-*)
            64-window row layout      B/* (<1,1> m16off, <0,0> v4-m, <1,0> v4-u-dup, <0,1> v5-m-s16)
            unfused loop / LSTM loop  C/*
"""
import ctypes as C
from collections import namedtuple

import pytest
import torch

import encoder_reference as er
from encoder_reference import Dims
from helpers import report

pytestmark = pytest.mark.gpu

SWITCHES = ("LFI_ENC_WIDE", "LFI_ENC_WIDE_BWD", "LFI_ENC_M16", "LFI_ENC_R64", "LFI_ENC_T16", "LFI_ENC_SCATTER16")

Case = namedtuple("Case", "id hid hist B N start col ldcond dup lstm precision masked two_products stash_f16 env fwd bwd stash unaligned")


def case(id, hid, hist, B, N, fwd, bwd, precision=1, masked=True, two=0, s16=0, dup=0, start=None, col=4, ldcond=None, lstm=0,
         env=None, stash=True, unaligned=False):
    """start=None: pos0 = start - hist + 1 = 0. ldcond=None: four columns behind the block, a multiple of 4 where hid is.
    fwd: the forward variant expected; bwd: 'acc' | 'w32' | 'w64' | 'unfused' | 'lstm' | None (forward only, no stash)."""
    start = hist - 1 if start is None else start
    ldcond = col + hid * (1 + dup) + 4 if ldcond is None else ldcond
    return Case(id, hid, hist, B, N, start, col, ldcond, dup, lstm, precision, masked, two, s16, env or {}, fwd, bwd, stash, unaligned)


M16OFF, T16OFF, T16ALL, R64OFF = {"LFI_ENC_M16": "0"}, {"LFI_ENC_T16": "0"}, {"LFI_ENC_T16": "2"}, {"LFI_ENC_R64": "0"}
BIG = dict(B=271, N=30)      # F = 8130 = 127 * 64 + 2: ceil(F / 64) = 128 workgroups, the last one holds two windows
CASES = [
    # ---- group A: few workgroups. precision 1 -> 32-window row-layout kernels, precision 0 -> exact-f32 accumulator layout
    case("A/h256-p1-m-two-s16", 256, 24, 5, 8, 2, "w32", two=1, s16=1),                    # F 40: one full group + 8 windows
    case("A/h256-p1-u-dup", 256, 24, 5, 8, 2, "w32", masked=False, dup=1),
    case("A/h256-p0-m", 256, 24, 5, 8, 1, "acc", precision=0),
    case("A/h128-p1-m-s16", 128, 16, 3, 11, 2, "w32", s16=1, start=17),                    # F 33, under one 64-window group
    case("A/h128-p1-u-two-dup", 128, 16, 3, 11, 2, "w32", masked=False, two=1, dup=1, start=17),
    case("A/h128-p0-u-dup", 128, 16, 3, 11, 1, "acc", precision=0, masked=False, dup=1, start=17),
    case("A/h64-p1-m-two-s16-dup", 64, 4, 1, 1, 2, "w32", two=1, s16=1, dup=1, start=5),   # F 1 (its one window is fully masked)
    case("A/h64-p0-u-two", 64, 4, 1, 1, 1, "acc", precision=0, masked=False, two=1, start=5),
    case("A/h192-p1-m-two-s16", 192, 2, 7, 19, 2, "w32", two=1, s16=1, start=3),           # Jp 256, Kp 192: a column group of padding
    case("A/h192-p1-u", 192, 2, 7, 19, 2, "w32", masked=False, start=3),
    case("A/h192-p0-m-dup", 192, 2, 7, 19, 1, "acc", precision=0, dup=1, start=3),
    case("A/h252-p1-m-two-s16-dup", 252, 3, 5, 9, 2, "w32", two=1, s16=1, dup=1, start=4),  # Kp 256: four k of padding
    case("A/h252-p1-u-s16", 252, 3, 5, 9, 2, "w32", masked=False, s16=1, start=4),
    case("A/h252-p0-u", 252, 3, 5, 9, 1, "acc", precision=0, masked=False, start=4),
    case("A/h256-hist1-p1-m-two-s16", 256, 1, 6, 7, 2, "w32", two=1, s16=1, start=2),
    case("A/h256-hist1-p1-u-dup", 256, 1, 6, 7, 2, "w32", masked=False, dup=1, start=0),
    case("A/h256-hist1-p0-m", 256, 1, 6, 7, 1, "acc", precision=0, start=2),
    case("A/h50-p1-m", 50, 5, 4, 9, 1, "acc", start=6),                                    # hid % 4 != 0: accumulator layout, bf16x3 forward
    case("A/h50-p1-u-two-dup", 50, 5, 4, 9, 1, "acc", masked=False, two=1, dup=1, start=6),
    case("A/h50-p0-m", 50, 5, 4, 9, 1, "acc", precision=0, start=6),
    case("A/col6-p1-m-two", 128, 3, 5, 9, 1, "acc", two=1, col=6, ldcond=391, start=4),
    case("A/col6-p1-u-dup", 128, 3, 5, 9, 1, "acc", masked=False, dup=1, col=6, ldcond=391, start=4),
    case("A/unaligned", 128, 3, 5, 9, 2, "w32", two=1, start=4, unaligned=True),          # (the query answers for aligned buffers: see run_case)
    case("A/wide0", 128, 16, 3, 11, 1, "w32", two=1, start=17, env={"LFI_ENC_WIDE": "0"}),
    case("A/widebwd0", 128, 16, 3, 11, 2, "acc", two=1, start=17, env={"LFI_ENC_WIDE_BWD": "0"}),
    case("A/fwd-h50-p1-m", 50, 5, 4, 9, 1, None, start=6, stash=False),
    case("A/fwd-h50-p1-u", 50, 5, 4, 9, 1, None, masked=False, start=6, stash=False),
    case("A/fwd-h50-p0-m", 50, 5, 4, 9, 1, None, precision=0, start=6, stash=False),
    case("A/fwd-h50-p0-u", 50, 5, 4, 9, 1, None, precision=0, masked=False, start=6, stash=False),
    case("A/fwd-h128-p1-m", 128, 16, 3, 11, 2, None, start=17, stash=False),
    case("A/fwd-h128-p1-u-dup", 128, 16, 3, 11, 2, None, masked=False, dup=1, start=17, stash=False),
    # ---- group B: the 64-window kernels, ceil(F / 2R) = 128 workgroups with a nearly empty last one
    case("B/m16off-m-two-s16", 256, 3, fwd=3, bwd="w64", two=1, s16=1, env=M16OFF, **BIG),
    case("B/m16off-u", 256, 3, fwd=3, bwd="w64", masked=False, env=M16OFF, **BIG),
    case("B/v4-m", 256, 3, fwd=4, bwd="w64", **BIG),
    case("B/v4-u-two-dup", 256, 3, fwd=4, bwd="w64", masked=False, two=1, dup=1, **BIG),
    case("B/v5-m-s16", 256, 3, fwd=5, bwd="w64", s16=1, env=T16ALL, **BIG),
    case("B/v5-u-two", 256, 3, fwd=5, bwd="w64", masked=False, two=1, env=T16ALL, **BIG),
    case("B/v5-m-two", 256, 3, fwd=5, bwd="w64", two=1, env=T16ALL, **BIG),
    case("B/v5-u-s16", 256, 3, fwd=5, bwd="w64", masked=False, s16=1, env=T16ALL, **BIG),
    case("B/fwd-v5-m", 256, 3, fwd=5, bwd=None, stash=False, **BIG),
    case("B/fwd-v5-u-dup", 256, 3, fwd=5, bwd=None, masked=False, dup=1, stash=False, **BIG),
    case("B/fwd-t16off-m", 256, 3, fwd=4, bwd=None, stash=False, env=T16OFF, **BIG),
    case("B/fwd-t16off-u-dup", 256, 3, fwd=4, bwd=None, masked=False, dup=1, stash=False, env=T16OFF, **BIG),
    case("B/fwd-m16off-m", 256, 3, fwd=3, bwd=None, stash=False, env=M16OFF, **BIG),
    case("B/fwd-m16off-u-dup", 256, 3, fwd=3, bwd=None, masked=False, dup=1, stash=False, env=M16OFF, **BIG),
    case("B/r64off", 256, 3, fwd=2, bwd="w32", two=1, s16=1, env=R64OFF, **BIG),            # the 32-window kernels on 255 groups
    case("B/h252-m-two-s16", 252, 3, fwd=4, bwd="w64", two=1, s16=1, **BIG),               # the 16x16x32 kernel on padded k
    case("B/h252-u", 252, 3, fwd=4, bwd="w64", masked=False, **BIG),
    case("B/h192-m-two-s16", 192, 2, fwd=3, bwd="w64", two=1, s16=1, **BIG),
    case("B/h192-u-dup", 192, 2, fwd=3, bwd="w64", masked=False, dup=1, **BIG),
    case("B/hist1", 256, 1, fwd=4, bwd="w64", two=1, s16=1, **BIG),
    case("B/hist5", 256, 5, fwd=4, bwd="w64", masked=False, s16=1, **BIG),
    case("B/h128-m-two", 128, 2, 271, 60, 3, "w64", two=1),                                    # F 16260 = 127 * 128 + 4
    case("B/h64-m-two-s16", 64, 2, 271, 120, 3, "w64", two=1, s16=1),                      # F 32520 = 127 * 256 + 8
    case("B/h64-u-s16", 64, 2, 271, 120, 3, "w64", masked=False, s16=1),
    # ---- group C: the loops (one GEMM + one gate kernel per history step)
    case("C/gru320-p0-m", 320, 3, 5, 8, 0, "unfused", precision=0, start=4),
    case("C/gru320-p1-u-dup", 320, 3, 5, 8, 0, "unfused", masked=False, dup=1, start=4),
    case("C/lstm64-p0-m", 64, 4, 3, 11, 0, "lstm", precision=0, lstm=1, start=5),
    case("C/lstm256-p1-m-dup", 256, 2, 5, 8, 0, "lstm", lstm=1, dup=1, start=3),
]

_gpu_error = []
_refs = {}      # one shape's references at a time (the cases of a shape are neighbours in CASES)


def _references(c, dims, dev):
    key = (c.hid, c.hist, c.B, c.N, c.start, c.col, c.ldcond, c.dup, c.lstm, c.masked)
    if key not in _refs:
        _refs.clear()
        inp = er.make_inputs(dims, lstm=bool(c.lstm), masked=c.masked, seed=3, ldcond=c.ldcond, device=dev)
        _refs[key] = {"inp": inp, "exact": er.run_autograd(inp, dims, torch.float64, bool(c.lstm)),
                      "fp32": er.run_autograd(inp, dims, torch.float32, bool(c.lstm)), "models": {}}
    return _refs[key]


def _model(ref, dims, lstm, flags):
    key = tuple(sorted(flags.items()))
    if key not in ref["models"]:
        ref["models"][key] = er.run_model(ref["inp"], dims, lstm=lstm, **flags)
    return ref["models"][key]


def _tiling(hid):
    """(ncg, R): column groups and windows per 4-wave workgroup of the fused kernels (enc_fused_shape)."""
    ncg = 1
    while ncg * 64 < hid:
        ncg *= 2
    return ncg, 32 * (4 // ncg)


GUARD = 64


def _stash(n, dev):
    """n floats of NaN and a guard tail of 7.0 behind them."""
    t = torch.full((n + GUARD,), float("nan"), device=dev)
    t[n:] = 7.0
    return t


def _tail_ok(t):
    return bool((t[-GUARD:] == 7.0).all())


def run_case(c, dev, monkeypatch):
    from lets_face_it_amd import _lib
    from lets_face_it_amd._lib import EncDesc, check
    L = _lib.lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    lstm = bool(c.lstm)
    hid, hist, B, N = c.hid, c.hist, c.B, c.N
    T = c.start + N + 2                      # trailing frame rows that no window reads
    F, G = N * B, (4 if lstm else 3) * hid
    width = hid * (1 + c.dup)
    assert c.col + width <= c.ldcond
    dims = Dims(B, T, N, c.start, hist, hid, c.col, c.dup)
    ref = _references(c, dims, dev)
    inp = ref["inp"]
    d = EncDesc(B, T, N, c.start, hist, hid, c.ldcond, c.col, c.precision, c.dup, c.lstm, c.two_products, c.stash_f16)
    dp = C.byref(d)
    st = torch.cuda.current_stream().cuda_stream

    # ---- which kernels the plan picks
    ncg, R = _tiling(hid)
    probe = EncDesc(B, T, N, c.start, hist, hid, c.ldcond, c.col, c.precision, c.dup, c.lstm, 1, 0)
    row_bwd = bool(L.lfi_encode_windows_grad_stash_bf16(C.byref(probe)))      # would the row-layout backward take it?
    g16 = bool(L.lfi_encode_windows_grad_stash_bf16(dp))
    compact = bool(L.lfi_encode_windows_compact_dgi(dp))
    prow = int(L.lfi_encode_windows_bias_rows(dp))
    assert int(L.lfi_encode_windows_fwd_variant(dp, int(c.masked), int(c.stash))) == c.fwd, "forward kernel"
    if c.stash_f16:
        assert L.lfi_encode_windows_stash_f16_ok(dp), "fp16 stash refused"
    if c.bwd in ("acc", "w32", "w64"):
        groups = -(-F // (2 * R if c.bwd == "w64" else R))
        assert compact and prow == groups * (4 // ncg), ("backward grid", prow, groups)
        assert row_bwd == (c.bwd != "acc"), "backward layout"
        assert g16 == bool(c.two_products and c.bwd != "acc")
        if c.bwd == "acc":
            assert not L.lfi_encode_windows_stash_f16_ok(dp)
    elif c.bwd is not None:
        assert prow == 0 and not compact and not g16 and not row_bwd

    # ---- buffers: cond with a row behind it and 7.0 everywhere; NaN stashes with guard tails; dXp with a row behind it
    def dev_f32(t, off=0):
        buf = torch.zeros(t.numel() + off, device=dev)
        buf[off:] = t.reshape(-1)
        return buf[off:].view(t.shape)
    off = 1 if c.unaligned else 0
    xp = dev_f32(inp["Xp"], off)
    cond_buf = torch.full(((F + 1) * c.ldcond + off,), 7.0, device=dev)
    cond = cond_buf[off:].view(F + 1, c.ldcond)
    whh, b_ih, b_hh, dcond = (inp[k].contiguous() for k in ("whh", "b_ih", "b_hh", "dcond"))
    mask = inp["mask"].contiguous() if c.masked else None
    mptr = mask.data_ptr() if c.masked else None
    work = torch.zeros(max(int(L.lfi_encode_windows_work_floats(dp)), 1), device=dev)
    n_gates = hist * F * (5 if lstm else 4) * hid
    gates = _stash(n_gates, dev) if c.stash else None
    hseq = _stash(hist * F * hid, dev) if c.stash else None
    if c.unaligned:     # the launcher, not the query, sees the pointers: with them it must take the accumulator-layout kernel, which
        d16 = EncDesc(B, T, N, c.start, hist, hid, c.ldcond, c.col, c.precision, c.dup, c.lstm, c.two_products, 1)   # has no fp16 stash
        assert xp.data_ptr() % 16 == 4 and cond.data_ptr() % 16 == 4 and L.lfi_encode_windows_stash_f16_ok(C.byref(d16))
        rc = L.lfi_encode_windows_fwd(C.byref(d16), xp.data_ptr(), whh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), mptr, cond.data_ptr(),
                                      gates.data_ptr(), hseq.data_ptr(), work.data_ptr(), st)
        assert rc != 0 and b"16-byte aligned" in L.lfi_last_error()
    check(L.lfi_encode_windows_fwd(dp, xp.data_ptr(), whh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), mptr, cond.data_ptr(),
                                   gates.data_ptr() if c.stash else None, hseq.data_ptr() if c.stash else None, work.data_ptr(), st), "fwd")
    torch.cuda.synchronize()
    outside = torch.ones(c.ldcond, dtype=torch.bool, device=dev)
    outside[c.col:c.col + width] = False
    assert bool((cond[F] == 7.0).all()), "forward wrote the row behind cond"
    assert bool((cond[:F][:, outside] == 7.0).all()), "forward wrote outside its columns"
    if c.unaligned:
        assert float(cond_buf[0]) == 7.0
    got = {"features": cond[:F, c.col:c.col + width].clone()}
    flags = {"three_products": c.precision == 1, "fast_gates": True}
    if c.bwd is None:
        assert torch.isfinite(got["features"]).all()
        model = _model(ref, dims, lstm, flags)
        err = er.rel_l2(got["features"], ref["exact"]["features"])
        allowed = er.MODEL_FACTOR * er.rel_l2(model["features"], ref["exact"]["features"]) + \
            er.F32_FACTOR * er.rel_l2(ref["fp32"]["features"], ref["exact"]["features"])
        report("enc-kernel %-26s fwd %d (no stash)  features %.2e/%.2e" % (c.id, c.fwd, err, allowed))
        assert err <= allowed, (c.id, err, allowed)
        return

    # ---- backward, bias gradients, scatter - the order of engine._encoder_backward
    n_dgi, n_dgh = hist * F * (hid if compact else G), hist * F * G
    dgi, dgh = _stash(n_dgi, dev), _stash(n_dgh, dev)
    part = _stash(prow * 4 * hid, dev) if prow else None
    check(L.lfi_encode_windows_bwd(dp, dcond.data_ptr(), c.ldcond, whh.data_ptr(), gates.data_ptr(), hseq.data_ptr(), dgi.data_ptr(),
                                   dgh.data_ptr(), part.data_ptr() if prow else None, work.data_ptr(), st), "bwd")
    gbi, gbh = _stash(G, dev), _stash(G, dev)
    if prow:
        check(L.lfi_encode_windows_bias_grads(part.data_ptr(), prow, hid, gbi.data_ptr(), gbh.data_ptr(), st), "bias grads")
    dxp = torch.full((B * T + 1, G), 7.0, device=dev)
    check(L.lfi_encode_windows_scatter(dp, dgi.data_ptr(), dgh.data_ptr(), mptr, dxp.data_ptr(), st), "scatter")
    torch.cuda.synchronize()

    # ---- decode the stashes; every write stayed inside
    for name, t in (("gates", gates), ("hseq", hseq), ("dgi", dgi), ("dgh", dgh), ("db_ih", gbi), ("db_hh", gbh)) + ((("bias_part", part),) if prow else ()):
        assert _tail_ok(t), "guard tail of " + name
    got["hseq"] = hseq[:hist * F * hid].view(hist, F, hid)
    if c.stash_f16:     # [hist][F][hid][4] halves in the first half of the buffer; the second half is never touched
        gdec = gates.view(torch.float16)[:n_gates].float()
        assert bool(torch.isnan(gates[n_gates // 2:n_gates]).all()), "fp16 gate stash wrote past its half"
    else:
        gdec = gates[:n_gates]
    if g16:
        dgh_d = dgh.view(torch.bfloat16)[:n_dgh].float().view(hist, F, G)
        dgi_d = dgi.view(torch.bfloat16)[:n_dgi].float().view(hist, F, -1)
        assert bool(torch.isnan(dgh[(n_dgh + 1) // 2:n_dgh]).all()) and bool(torch.isnan(dgi[(n_dgi + 1) // 2:n_dgi]).all()), "bf16 stash wrote past its half"
    else:
        dgh_d, dgi_d = dgh[:n_dgh].view(hist, F, G), dgi[:n_dgi].view(hist, F, -1)
    got["dgh"] = dgh_d
    got["dgi"] = torch.cat([dgh_d[..., :2 * hid], dgi_d], dim=-1) if compact else dgi_d
    got["dW_hh"] = er.dwhh_from_stashes(dgh_d, got["hseq"])       # torch fp64 on the decoded stashes: the kernels, not the GEMM
    if prow:
        got["db_ih"], got["db_hh"] = gbi[:G], gbh[:G]
    else:
        got["db_ih"], got["db_hh"] = got["dgi"].double().sum(dim=(0, 1)), got["dgh"].double().sum(dim=(0, 1))
    for name in ("hseq", "dgi", "dgh", "db_ih", "db_hh"):
        assert bool(torch.isfinite(got[name]).all()), name + " holds values nobody wrote"
    assert bool(torch.isfinite(gdec).all()), "gate stash holds values nobody wrote"
    assert bool((dxp[B * T] == 7.0).all()), "scatter wrote the row behind dXp"
    got["dXp"] = dxp[:B * T]
    read = torch.zeros(B * T, dtype=torch.bool, device=dev)
    read[er.window_rows(dims, dev).reshape(-1)] = True
    assert not bool(read.all()) and bool((got["dXp"][~read] == 0).all()), "frame rows no window reads must be exactly 0"

    # ---- the model that describes this case's kernels
    if c.bwd in ("w32", "w64"):
        flags.update(stash_f16=bool(c.stash_f16), two_products=g16, grads_bf16=g16)
    elif c.bwd == "acc":
        flags.update(bwd_exact=True)      # exact-f32 recurrence whatever the precision; fp32 stashes
    model = _model(ref, dims, lstm, flags)
    rows = er.compare(got, ref["exact"], model, ref["fp32"], hid)
    summary = {}
    for name, e, a, ok in rows:
        k = name.split("[")[0]
        ratio = (e / a) if a > 0 else (0.0 if e == 0 else float("inf"))
        if k not in summary or ratio >= summary[k][0]:
            summary[k] = (ratio, e, a)
    report("enc-kernel %-26s fwd %d bwd %-7s %s" % (c.id, c.fwd, c.bwd, "  ".join(
        "%s %.1e/%.1e" % (k, summary[k][1], summary[k][2]) for k in ("features", "hseq", "dgi", "dgh", "dXp", "dW_hh", "db_ih", "db_hh"))))
    assert not er.failures(rows), (c.id, er.failures(rows))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_window_encoder_kernel_vs_fp64(gpu_device, monkeypatch, c):
    """One case of the list above: kernels asserted, writes in bounds, every part within 3 x model + 8 x fp32 of the fp64 reference."""
    if _gpu_error:
        pytest.fail("not run: an earlier case ended in a GPU error (%s)" % _gpu_error[0])
    try:
        run_case(c, gpu_device, monkeypatch)
    except AssertionError:
        raise
    except Exception as e:      # a HIP error is sticky: launch nothing more on this device from this module
        _gpu_error.append("%s: %s" % (c.id, str(e)[:200]))
        raise


def test_case_list_reaches_every_kernel_form():
    """The list itself: every forward variant in masked / unmasked, fp32-stash / fp16-stash / no-stash form and every fused backward
    kernel in its <two products, fp16 stash> forms (the accumulator-layout backward has one form), plus both loops."""
    fwd = {(c.fwd, c.masked, "none" if not c.stash else ("f16" if c.stash_f16 else "f32")) for c in CASES if not c.lstm}
    for v in (1, 2, 3, 4, 5):
        for m in (True, False):
            for s in ("f32", "none") + (("f16",) if v >= 2 else ()):
                assert (v, m, s) in fwd, (v, m, s)
    assert {m for v, m, s in fwd if v == 0} == {True, False}
    bwd = {(c.bwd, c.two_products, c.stash_f16) for c in CASES}
    for k in ("w32", "w64"):
        for two in (0, 1):
            for s16 in (0, 1):
                assert (k, two, s16) in bwd, (k, two, s16)
    assert {c.bwd for c in CASES} >= {"acc", "unfused", "lstm"}
    assert {c.precision for c in CASES if c.fwd == 1 and c.stash} == {0, 1} and {c.dup for c in CASES if c.lstm} == {0, 1}
