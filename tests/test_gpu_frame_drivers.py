"""The per-frame flow drivers - lfi_flow_sample_seq_nll, lfi_flow_score_seq_from, lfi_flow_score_seq_chunk, lfi_flow_score_seq_chunk_rows
and lfi_flow_step_rows_from: the kernels of lfi_flow_chain.hip, lfi_flow_chunk.hip, lfi_flow_chunk_rows.hip, lfi_sample.hip and the frame
cells of lfi_flow_cells.h - against an fp64 flow written from the definition (tests/frame_reference.py), through the C ABI in the order
stream.py / engine.py call it: lfi_flow_prep(with_inverse = 1), then the drivers, on a raw prev_p1_face window or on one that goes
through a ModalityEncoder per frame (lfi_p1enc kind mlp / rnn / lstm). An error per frame and per (flow step, frame) cell of the recurrent state, for the rows of the last batch tile and for each role group on their own.
(SeqGlow.inference, glow/models.py:567-596; FlowStep.reverse_flow :345-373.)

Bound, for every case, leg and part, every error a relative L2 with no floor against the fp64 run:

    err(kernel) <= 3 * err(model run with the flags that describe the case's kernels) + 8 * err(reference in torch fp32)

Which kernels a case reaches is asserted before anything is launched: lfi_flow_frame_plan's bits (1 register-resident cells, 2 one
launch per frame's chain, 4 reverse cells with three fp16 products, 8 their weights from the fp16 images, 16 forward cells with three
fp16 products) and lfi_flow_score_chunk_ok. Which front end ran is read from pre_static afterwards: bit-identical = the fused
conditioning kernel (it never writes c), otherwise it holds c, one more compared part. Every work area has exactly the size its
*_floats query returns, between two guard bands; outputs start as NaN or a sentinel.

The encoded kinds (ENC_CASES): what joins the tested leaf kernels - lfi_internal_sample_front_rows, sample_front_setup / _frame,
chunk_front / chunk_carve and lfi_flow_sample_p1_work_floats. The per-frame legs read the window straight out of `faces` ((t - hist1) C
floats into a row of pitch seq_len C: 16-byte aligned on every other frame at C = 50), the chunk legs from an aligned stage with
N B rows; the feature buffer has pitch (hid + 3) & ~3 and p1work starts as NaN between guard bands, so a padding column or a slot
nobody wrote poisons c; wct's block starts at `col`, every other column is non-zero. Their front end is always the GEMMs, so c[n] is a
compared part everywhere - the part that sees the encoder most directly. Which window-encoder kernel a recurrent kind reaches
(lfi_encode_windows_fwd_variant on the descriptor the front end builds, for B and for N B rows) is asserted before the launch too:
lfi_enc_desc.precision is gemm_precision, of which the fused GRU kernels know only "== 1" (bf16x3 recurrence; anything else is the
exact f32 recurrence) while the unfused and LSTM loops hand it to their per-step GEMM - model_flags says which.

Legs, one set of inputs per case: gen (lfi_flow_sample_seq_nll frame by frame, and again with nll = NULL: bit-identical frames and
state), gen1 (the N frames in one call: the window-fragment hand-over from a frame's chain to the next frame's conditioning), obs
(lfi_flow_score_seq_from over the fp64 run's frames rounded to fp32, frame by frame, and once as one call with z = NULL), chunk (dense
in one call and in two, ragged with lengths 0 .. N - 1 behind a dense first frame), roles (lfi_flow_step_rows_from with roles that
change from frame to frame).

Not covered here: lfi_flow_sample_cand_from / _cand_seq and lfi_flow_step_rows_seq - tests/test_gpu_stream_candidates.py, _rollouts.py and
_rows_many.py hold them bit for bit to the entry points above, whose bodies they share; the 64-window encoder kernels (variants 3 - 5:
8192 windows a call at least, fp64 cases of their own in tests/test_gpu_encoder_kernels.py); the window movers of lfi_stream.hip - exact
copies, tested with torch.equal (tests/test_gpu_stream_windows.py). No case abandons a chain on purpose: a chain that gives up leaves NaN,
which the comparison rejects.
"""
import ctypes as C
import time
from collections import namedtuple

import pytest
import torch

import flow_reference as fr
import frame_reference as fq
from helpers import report
from test_gpu_flow_walks import Guarded

pytestmark = pytest.mark.gpu

SWITCHES = ("LFI_SAMPLE_FUSED", "LFI_SAMPLE_WFRAG16", "LFI_PIPE_X3", "LFI_SAMPLE_CHAIN", "LFI_FLOW_GENERIC", "LFI_SAMPLE_XFRAG",
            "LFI_SAMPLE_XF_CHAIN", "LFI_SAMPLE_COND_ROWS", "LFI_CHUNK_ONLY", "LFI_PIPE_FORCE_ABORT", "LFI_PIPE_FENCE")
HIST1, START = 3, 4
FUSED, GEMMS = "fused", "GEMMs"
SENT = 1234.5       # frame slots nobody has written yet, z / nll behind a row's length (finite: a dense front end may read a slot)

Case = namedtuple("Case", "id C H Ks B N D affine lstm dense p env clamp roles expect front enc ehid col hist1 evar")


def case(id, p, expect, front, C=50, H=128, Ks=3, B=33, N=4, D=512, affine=1, lstm=0, dense=0, env=None, clamp=0, roles=0,
         enc="none", ehid=0, col=0, hist1=HIST1, evar=None):
    """expect: lfi_flow_frame_plan's bits; front: the front end lfi_flow_sample_seq_nll / _score_seq_from / _step_rows_from take;
    enc, ehid, col, hist1: the lfi_p1enc the window goes through; evar: lfi_encode_windows_fwd_variant of a recurrent kind."""
    return Case(id, C, H, Ks, B, N, D, affine, lstm, dense, p, env or {}, clamp, roles, expect, front, enc, ehid, col, hist1, evar)


RAW_CASES = [
    case("final-9", 9, 31, FUSED, B=65, roles=1),          # five 16-row tiles and two 64-row conditioning tiles, each ending in one row
    case("final-9-unfused", 9, 31, GEMMS, env={"LFI_SAMPLE_FUSED": "0"}),
    case("final-9-wfrag0", 9, 23, FUSED, env={"LFI_SAMPLE_WFRAG16": "0"}),
    case("final-5", 5, 15, GEMMS, roles=1),
    case("final-1", 1, 15, GEMMS),
    case("final-0", 0, 3, GEMMS),
    case("final-9-x3off", 9, 3, FUSED, env={"LFI_PIPE_X3": "0"}),
    case("final-9-steps", 9, 21, FUSED, env={"LFI_SAMPLE_CHAIN": "0"}, roles=1),     # one launch per flow step, exact f32
    case("final-9-generic", 9, 20, FUSED, env={"LFI_FLOW_GENERIC": "1"}),            # streaming cells
    case("clamp-9", 9, 31, FUSED, clamp=1),
    case("lstm128", 9, 3, FUSED, lstm=1, roles=1),                                   # G = 512: the other size of sc_cond_kernel
    case("lstm64", 0, 3, GEMMS, lstm=1, H=64, D=64),
    case("lstm64-steps", 0, 1, GEMMS, lstm=1, H=64, D=64, env={"LFI_SAMPLE_CHAIN": "0"}),     # (not in the issue's table: the LSTM cell per step)
    case("h120", 9, 31, GEMMS, H=120, D=64, B=17),                                   # H16 = 128: eight padding hidden units
    case("c64", 9, 31, FUSED, C=64, Ks=2, B=32),
    case("additive", 9, 31, FUSED, affine=0, Ks=2, B=17),
    case("odd", 9, 3, GEMMS, C=15, H=24, Ks=4, B=6, D=20, dense=1, roles=1),
    case("h44", 5, 3, GEMMS, H=44, B=8, D=64),
    case("h160", 0, 0, GEMMS, H=160, Ks=2, B=5, D=64),
    case("tiles", 9, 31, FUSED, B=130, roles=1),           # nine batch tiles and three conditioning tiles, the last of two rows
    case("one", 9, 31, FUSED, B=1, Ks=1, N=1),
]


def enc_case(id, enc, ehid, col, p, expect, evar=None, hist1=HIST1, **kw):
    return case(id, p, expect, GEMMS, enc=enc, ehid=ehid, col=col, hist1=hist1, evar=evar, **kw)


# The encoded kinds, at the smallest shapes that still reach each path (none is a workload shape). expect: what the same flow shape
# has above. evar, by hand from enc_plan_fwd (lfi_encoder_common.h): an LSTM and hid > 256 -> 0, the loop of one GEMM + one gate kernel
# per history step; precision 1, hid % 4 == 0, ldcond = hid4 and col = 0 multiples of 4, aligned -> 2, the 32-window row-layout kernel
# (the 64-window kernels want >= 128 workgroups of 64 windows); everything else -> 1, the accumulator-layout kernel, bf16x3 at
# precision 1 and exact f32 otherwise. With C = 50 and N = 4 the window start (t - hist1) C is 16-byte aligned on two frames and not on
# the other two.
ENC_CASES = [
    enc_case("mlp30-9", "mlp", 30, 6, 9, 31, roles=1),        # hid % 4 = 2 (hid4 = 32), wct + col misaligned, two tiles + one row
    enc_case("mlp30-1", "mlp", 30, 6, 1, 15),                 # bf16x3 front products
    enc_case("mlp30-0", "mlp", 30, 6, 0, 3, B=17),            # exact front, per-step plan
    enc_case("rnn128-1", "rnn", 128, 0, 1, 15, evar=2, roles=1),      # row-layout GRU kernel, bf16x3 recurrence
    enc_case("rnn128-9", "rnn", 128, 0, 9, 31, evar=1, roles=1),      # precision 9: exact f32 recurrence, front at fp16x3
    enc_case("rnn50-1", "rnn", 50, 6, 1, 15, evar=1),         # hid % 4 != 0: accumulator layout with bf16x3, hid4 = 52
    enc_case("rnn260-9", "rnn", 260, 0, 9, 31, evar=0, B=5),  # hid > 256: the unfused loop, hs and per-step GEMMs at 9
    enc_case("lstm64-9", "lstm", 64, 0, 9, 31, evar=0),       # LSTM loop, gate + cell stash inside p1work
    enc_case("lstm30-1", "lstm", 30, 6, 1, 15, evar=0, B=17),         # LSTM with padded pitch and misaligned col
    enc_case("rnn-hist1", "rnn", 128, 0, 9, 31, evar=1, hist1=1, B=17),       # one-step recurrence from zero
    enc_case("rnn-hist4", "rnn", 64, 4, 9, 31, evar=1, hist1=4, B=17),        # the first frame's window starts at frame 0 of faces
    enc_case("rnn-lstmflow", "rnn", 64, 0, 0, 3, evar=1, B=17, lstm=1, H=64, D=64),       # the LSTM cell's chain, cstate carried
    # (not in the issue's table: the same without a chain plan - the encoded front end in front of launch_rev_frame)
    enc_case("rnn-lstmflow-steps", "rnn", 64, 0, 0, 1, evar=1, B=17, lstm=1, H=64, D=64, env={"LFI_SAMPLE_CHAIN": "0"}),
    enc_case("rnn-tiles", "rnn", 128, 0, 9, 31, evar=1, B=130, roles=1),      # nine batch tiles; the chunk leg encodes 520 windows
    enc_case("mlp-one", "mlp", 12, 0, 9, 31, B=1, Ks=1, N=1),                 # one row, one frame
    enc_case("rnn-odd", "rnn", 12, 3, 0, 3, evar=1, C=15, H=24, Ks=4, B=6, D=20, dense=1, roles=1),   # every window start 4-byte aligned only
]
CASES = RAW_CASES + ENC_CASES
SEED = 4      # the clamp case's conditions hold at this seed (tests/test_frame_reference_cpu.py checks them)


def ref_dims(c):
    return fr.Dims(c.B, START + c.N + 1, c.N, START, c.C, c.H, c.D, c.Ks, c.affine, c.lstm, fr.CLAMP_EPS if c.clamp else fr.EPS)


def flow_dims(c, N=None):
    from lets_face_it_amd._lib import FlowDims
    d = ref_dims(c)
    return FlowDims(c.B, c.N if N is None else N, c.C, c.H, c.D, c.Ks, c.affine, c.lstm, d.scale_eps, c.p)


def model_flags(c):
    """The roundings the case's kernels document, by the plan bits the case asserts: the chains' three-product forms "are used where
    bit 2 is set" (lfi.h); every other cell is the exact f32 MFMA. The front end's products run at the case's gemm_precision."""
    chain = bool(c.expect & 2)
    flags = dict(fast_gates=True, w_fp32=True, front=c.p, x3h_rev=chain and bool(c.expect & 4), x3h_fwd=chain and bool(c.expect & 16))
    if c.enc in ("rnn", "lstm"):
        # lfi.h beside lfi_p1enc: "1 -> bf16x3 recurrence; any other value -> exact f32 recurrence; loops take the GEMM mode as given"
        fused = c.enc == "rnn" and c.evar in (1, 2)
        flags.update(enc_three_products=fused and c.p == 1, enc_loop_front=not fused)
    return flags


def enc_desc(c, rows):
    """The descriptor lfi_internal_sample_front_rows builds for `rows` windows of a recurrent kind (the GRU without a gate stash)."""
    from lets_face_it_amd._lib import EncDesc
    ed = EncDesc()
    ed.B, ed.T, ed.N, ed.start, ed.hist, ed.hid = rows, c.hist1, 1, c.hist1 - 1, c.hist1, c.ehid
    ed.ldcond, ed.col, ed.precision, ed.dup, ed.lstm = (c.ehid + 3) & ~3, 0, c.p, 0, int(c.enc == "lstm")
    return ed


def enc_variants(L, c):
    """lfi_encode_windows_fwd_variant for the per-frame legs' B windows and the chunk legs' N B (host only)."""
    return [int(L.lfi_encode_windows_fwd_variant(C.byref(enc_desc(c, rows)), 0, 0)) for rows in (c.B, c.N * c.B)]


def ragged_lengths(c):
    """Lengths over the N - 1 frames behind the dense first one: 0, N - 1 and what lies between, the second batch tile all 0."""
    n1 = c.N - 1
    L = [[0, n1, 1, 2][b % 4] if n1 >= 2 else b % 2 * n1 for b in range(c.B)]
    L = [min(v, n1) for v in L]
    if c.B >= 32:
        L[16:32] = [0] * 16
    return L


def leg_roles(c):
    """name -> roles (N x B) of the reference run each leg is compared with."""
    d = ref_dims(c)
    out = {"gen": fq.roles_all(d, fq.GEN), "obs": fq.roles_all(d, fq.OBS)}
    if c.N >= 2:
        out["ragged"] = fq.roles_ragged(d, [1 + v for v in ragged_lengths(c)])
    if c.roles:
        b, n = torch.arange(c.B).unsqueeze(0), torch.arange(c.N).unsqueeze(1)
        kind = (b // 16 + n) % 3            # per (frame, 16-row tile): all observe, all generate, mixed
        out["roles"] = torch.where(kind == 0, fq.OBS, torch.where(kind == 1, fq.GEN, (b + n) % 2))
    return out


_gpu_error = []
_refs = {}      # one input set's references at a time (the cases of a shape are neighbours in CASES)


def references(c):
    """inp, and per leg the roles, the given frames and the fp64 / fp32 runs - on the host, at most 8 threads."""
    d = ref_dims(c)
    key = (d, c.dense, c.clamp, c.roles, c.enc, c.ehid, c.col, c.hist1)
    if key not in _refs:
        _refs.clear()
        torch.set_num_threads(min(8, torch.get_num_threads()))
        inp = fq.make_frame_inputs(d, c.hist1, dense=bool(c.dense), seed=SEED, clamp=bool(c.clamp), enc=c.enc, ehid=c.ehid, col=c.col)
        legs = {}
        for name, roles in leg_roles(c).items():
            given = None if name == "gen" else legs["gen"]["exact"]["x"].float()
            legs[name] = {"roles": roles, "given": given, "exact": fq.run_exact(inp, d, roles, given=given),
                          "fp32": fq.run_exact(inp, d, roles, torch.float32, given=given), "models": {}}
        _refs[key] = {"inp": inp, "legs": legs}
    return _refs[key]


def model_run(ref, leg, d, flags):
    key = tuple(sorted(flags.items()))
    L = ref["legs"][leg]
    if key not in L["models"]:
        L["models"][key] = fq.run_model(ref["inp"], d, L["roles"], given=L["given"], **flags)
    return L["models"][key]


class Session:
    """The device side of one case: parameters, prep, the inputs, and fresh outputs per leg."""

    def __init__(self, c, dev, ref):
        from lets_face_it_amd import _lib
        from lets_face_it_amd._lib import FlowParams, P1Enc, check
        self.c, self.dev, self.L, self.check = c, dev, _lib.lib(), check
        self.d = d = ref_dims(c)
        self.dims = flow_dims(c)
        inp = ref["inp"]
        self.par = {k: v.to(dev).contiguous() for k, v in inp["params"].items()}
        self.p = FlowParams()
        for name, t in self.par.items():
            setattr(self.p, name, t.data_ptr())
        self.st = torch.cuda.current_stream().cuda_stream
        self.wct, self.noise, self.x0 = (inp[k].to(dev).contiguous() for k in ("wct", "noise", "x0"))
        self.pre_host = inp["pre_static"].to(dev).contiguous()
        self.E, self.T, self.KD = self.wct.shape[1], d.T, c.Ks * c.D
        self.guards = []
        self.prep = self.guarded("prep", self.L.lfi_flow_prep_floats(C.byref(self.dims)))
        check(self.L.lfi_flow_prep(C.byref(self.dims), C.byref(self.p), self.prep.ptr(), 1, self.st), "prep")
        self.work = self.guarded("work", self.L.lfi_flow_sample_work_floats(C.byref(self.dims)))
        self.nll_work = self.guarded("nll_work", self.L.lfi_flow_sample_nll_work_floats(C.byref(self.dims)))
        self.pre = self.guarded("pre_static", c.N * c.B * self.KD)
        # the encoder the window goes through: its parameters, and a p1work of exactly the size asked for that starts as NaN
        self.p1, self.p1work = None, None
        if c.enc != "none":
            self.enc = {k: v.to(dev).contiguous() for k, v in inp["p1enc"].items() if torch.is_tensor(v)}
            self.p1 = P1Enc()
            self.p1.kind, self.p1.hid, self.p1.col = fq.ENCS.index(c.enc), c.ehid, c.col
            for name, t in self.enc.items():
                setattr(self.p1, name, t.data_ptr())
            self.p1work = self.guarded("p1work", self.L.lfi_flow_sample_p1_work_floats(C.byref(self.dims), C.byref(self.p1), c.hist1),
                                       float("nan"))

    def p1ref(self):
        return C.byref(self.p1) if self.p1 is not None else None

    def guarded(self, name, n, fill=0.0):
        g = Guarded(n, self.dev, fill)
        self.guards.append((name, g))
        return g

    def fresh(self, given=None):
        """faces (seed frames, then SENT or the given frames), zero state, NaN nll / z."""
        c = self.c
        s = {"faces": self.guarded("faces", c.B * self.T * c.C, SENT), "h": self.guarded("h", c.Ks * c.B * c.H),
             "cstate": self.guarded("cstate", c.Ks * c.B * c.H) if c.lstm else None,
             "nll": self.guarded("nll", c.N * c.B, float("nan")), "z": self.guarded("z", c.N * c.B * c.C, float("nan"))}
        f = s["faces"].t.view(c.B, self.T, c.C)
        f[:, :START] = self.x0[:, :START]
        if given is not None:
            f[:, START:START + c.N] = given.to(self.dev).transpose(0, 1)
        return s

    def frames(self, s):
        return s["faces"].t.view(self.c.B, self.T, self.c.C)

    def upload(self):
        self.pre.t.copy_(self.pre_host.reshape(-1))

    def front_of(self, n0, n1, expect):
        """Which front end ran over frames n0 .. n1 - 1, from pre_static itself; -> c of those frames, or None (the fused kernel)."""
        torch.cuda.synchronize()
        got, was = self.pre.t.view(self.c.N, self.c.B, self.KD)[n0:n1], self.pre_host[n0:n1]
        front = FUSED if torch.equal(got, was) else GEMMS
        assert front == expect, ("front end", front, expect)
        return None if front == FUSED else got.clone()

    def args(self, s, n, nframes, noise=False, N=None, p1work=True):
        """The arguments every driver shares up to p1work (p1work = False: NULL, as stream.py calls the chunk drivers, which carve
        their own), for frames n .. n + nframes - 1 of the session."""
        c, o = self.c, lambda g, per: g.ptr() + 4 * n * per
        dims = self.dims if N is None else flow_dims(c, N)
        a = [C.byref(dims), C.byref(self.p), self.prep.ptr(), self.wct.data_ptr(), self.E, c.hist1, o(self.pre, c.B * self.KD)]
        if noise:
            a.append(self.noise.data_ptr() + 4 * n * c.B * c.C)
        return a + [s["faces"].ptr(), self.T, START + n, nframes, n, s["h"].ptr(), s["cstate"].ptr() if c.lstm else None, self.p1ref(),
                    self.p1work.ptr() if p1work and self.p1work is not None else None]

    def state(self, s):
        c = self.c
        torch.cuda.synchronize()
        return s["h"].t.view(c.Ks, c.B, c.H).clone(), (s["cstate"].t.view(c.Ks, c.B, c.H).clone() if c.lstm else None)

    def run_of(self, s, states, cs, z=False, nll=True, x=True):
        """A run dict from the session's buffers. states: {frame: (h, cstate)}."""
        c = self.c
        full = torch.full((c.Ks, c.N, c.B, c.H), float("nan"), device=self.dev)
        h, cst = full.clone(), (full.clone() if c.lstm else None)
        for n, (hn, cn) in states.items():
            h[:, n] = hn
            if c.lstm:
                cst[:, n] = cn
        run = {"x": self.frames(s)[:, START:START + c.N].transpose(0, 1).clone() if x else None,
               "z": s["z"].t.view(c.N, c.B, c.C).clone() if z else None, "nll": s["nll"].t.view(c.N, c.B).clone() if nll else None,
               "h": h, "cstate": cst, "state_frames": sorted(states), "c": None}
        if cs and all(v is not None for v in cs):
            run["c"] = torch.cat(cs)
        return run


def run_case(c, dev, monkeypatch):
    from lets_face_it_amd import _lib
    L = _lib.lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    d = ref_dims(c)
    B, N, Ks, Cc = c.B, c.N, c.Ks, c.C
    # ---- the kernels these calls take, before anything is launched
    dims = flow_dims(c)
    plan = int(L.lfi_flow_frame_plan(C.byref(dims)))
    assert plan == c.expect, ("frame plan", plan, c.expect)
    chunk_ok = bool(L.lfi_flow_score_chunk_ok(C.byref(dims)))
    assert chunk_ok == bool(c.expect & 2), ("lfi_flow_score_chunk_ok", chunk_ok)
    assert Ks * -(-B // 16) <= 64, "the chains must be co-resident many times over"
    if c.enc in ("rnn", "lstm"):
        assert enc_variants(L, c) == [c.evar, c.evar], ("window-encoder kernel", enc_variants(L, c), c.evar)
    assert c.enc == "none" or c.front == GEMMS

    ref = references(c)
    flags = model_flags(c)
    S = Session(c, dev, ref)
    check = S.check
    all_rows, notes = [], []

    def judge(leg, tag, got):
        Lg = ref["legs"][leg]
        rows = fq.compare(got, Lg["exact"], model_run(ref, leg, d, flags), Lg["fp32"], d, Lg["roles"])
        assert rows, (tag, "nothing compared")
        all_rows.extend((tag + " " + name, e, a, ok) for name, e, a, ok in rows)

    def sentinel_behind(s, n_done, tag):
        assert bool((S.frames(s)[:, START + n_done:] == SENT).all()), tag + ": a frame slot behind the last generated frame was written"

    # ---- leg 1: generate frame by frame, with and without nll
    kept = {}
    for with_nll in (True, False):
        s, states, cs = S.fresh(), {}, []
        for n in range(N):
            S.upload()
            check(L.lfi_flow_sample_seq_nll(*S.args(s, n, 1, noise=True), S.work.ptr(), (s["nll"].ptr() + 4 * n * B) if with_nll else None,
                                            S.nll_work.ptr() if with_nll else None, S.st), "sample_seq_nll")
            cs.append(S.front_of(n, n + 1, c.front))
            states[n] = S.state(s)
            sentinel_behind(s, n + 1, "gen")
        kept[with_nll] = (s, states)
        if with_nll:
            gen_run = S.run_of(s, states, cs)
            judge("gen", "gen", gen_run)
        else:
            assert bool(torch.isnan(s["nll"].t).all()), "nll written without an nll array"
    (sa, sta), (sb, stb) = kept[True], kept[False]
    assert torch.equal(sa["faces"].t, sb["faces"].t), "frames differ between nll and nll = NULL"
    for n in range(N):
        assert torch.equal(sta[n][0], stb[n][0]) and (not c.lstm or torch.equal(sta[n][1], stb[n][1])), "state differs with nll = NULL"

    # ---- leg 2: the N frames in one call
    s = S.fresh()
    S.upload()
    check(L.lfi_flow_sample_seq_nll(*S.args(s, 0, N, noise=True), S.work.ptr(), s["nll"].ptr(), S.nll_work.ptr(), S.st), "sample_seq_nll N")
    cs = [S.front_of(0, N, c.front)]
    one = S.run_of(s, {N - 1: S.state(s)}, cs)
    sentinel_behind(s, N, "gen1")
    judge("gen", "gen1", one)
    notes.append("gen1%sgen" % ("==" if torch.equal(one["x"], gen_run["x"]) and torch.equal(one["nll"], gen_run["nll"]) else "!="))

    # ---- leg 3: observe the fp64 run's frames, frame by frame; once more in one call without z
    given = ref["legs"]["obs"]["given"]
    score_work = S.guarded("score_work", L.lfi_flow_score_work_floats(C.byref(dims)))
    s, states, cs = S.fresh(given), {}, []
    before = s["faces"].t.clone()
    for n in range(N):
        S.upload()
        check(L.lfi_flow_score_seq_from(*S.args(s, n, 1), S.work.ptr(), score_work.ptr(), s["z"].ptr() + 4 * n * B * Cc,
                                        s["nll"].ptr() + 4 * n * B, S.st), "score_seq_from")
        cs.append(S.front_of(n, n + 1, c.front))
        states[n] = S.state(s)
    judge("obs", "obs", S.run_of(s, states, cs, z=True, x=False))
    assert torch.equal(s["faces"].t, before), "observe wrote into faces"
    s = S.fresh(given)
    S.upload()
    check(L.lfi_flow_score_seq_from(*S.args(s, 0, N), S.work.ptr(), score_work.ptr(), None, s["nll"].ptr(), S.st), "score_seq_from N")
    cs = [S.front_of(0, N, c.front)]
    judge("obs", "obs1", S.run_of(s, {N - 1: S.state(s)}, cs, x=False))
    assert bool(torch.isnan(s["z"].t).all()), "z written without a z array"

    # ---- leg 4: the chunk chains (their front end is always the GEMMs: pre_static holds c afterwards)
    if chunk_ok:
        # (an encoded window: the chunk's own p1work lies inside chunk_work, so that starts as NaN too)
        cw_fill = 0.0 if c.enc == "none" else float("nan")
        cw = S.guarded("chunk_work", L.lfi_flow_score_chunk_work_floats(C.byref(dims), S.p1ref(), c.hist1), cw_fill)
        s = S.fresh(given)
        S.upload()
        check(L.lfi_flow_score_seq_chunk(*S.args(s, 0, N, p1work=False), None, cw.ptr(), s["z"].ptr(), s["nll"].ptr(), S.st), "score_seq_chunk")
        cs = [S.front_of(0, N, GEMMS)]
        judge("obs", "chunk", S.run_of(s, {N - 1: S.state(s)}, cs, z=True, x=False))
        if N >= 2:
            n0 = N // 2
            cw2 = S.guarded("chunk_work 2", L.lfi_flow_score_chunk_work_floats(C.byref(flow_dims(c, N - n0)), S.p1ref(), c.hist1), cw_fill)
            s, cs, states = S.fresh(given), [], {}
            for a, cnt in ((0, n0), (n0, N - n0)):
                S.upload()
                check(L.lfi_flow_score_seq_chunk(*S.args(s, a, cnt, N=N - n0, p1work=False), None, cw2.ptr(), s["z"].ptr() + 4 * a * B * Cc,
                                                 s["nll"].ptr() + 4 * a * B, S.st), "score_seq_chunk 2")
                cs.append(S.front_of(a, a + cnt, GEMMS))
                states[a + cnt - 1] = S.state(s)
            judge("obs", "chunk2", S.run_of(s, states, cs, z=True, x=False))
            # ragged: a dense first frame, then lengths 0 .. N - 1 over the frames behind it
            lengths = ragged_lengths(c)
            ldev = torch.tensor(lengths, dtype=torch.int32, device=dev)
            s, cs = S.fresh(given), []
            s["z"].t.fill_(SENT)
            s["nll"].t.fill_(SENT)
            S.upload()
            check(L.lfi_flow_score_seq_chunk(*S.args(s, 0, 1, p1work=False), None, cw.ptr(), s["z"].ptr(), s["nll"].ptr(), S.st), "score_seq_chunk first")
            cs.append(S.front_of(0, 1, GEMMS))
            h0, c0 = S.state(s)
            S.upload()
            check(L.lfi_flow_score_seq_chunk_rows(*S.args(s, 1, N - 1, p1work=False), None, cw.ptr(), s["z"].ptr() + 4 * B * Cc, s["nll"].ptr() + 4 * B,
                                                  ldev.data_ptr(), S.st), "score_seq_chunk_rows")
            cs.append(S.front_of(1, N, GEMMS))
            h1, c1 = S.state(s)
            judge("ragged", "ragged", S.run_of(s, {0: (h0, c0), N - 1: (h1, c1)}, cs, z=True, x=False))
            zero = ldev == 0
            assert bool(zero.any()) and N - 1 in lengths
            assert torch.equal(h1[:, zero], h0[:, zero]) and (not c.lstm or torch.equal(c1[:, zero], c0[:, zero])), \
                "a row of length 0 did not keep its state bit for bit"
            behind = torch.arange(1, N, device=dev).unsqueeze(1) > ldev.unsqueeze(0)         # frame n >= 1 + lengths[b]
            assert bool((s["z"].t.view(N, B, Cc)[1:][behind] == SENT).all()) and bool((s["nll"].t.view(N, B)[1:][behind] == SENT).all()), \
                "z / nll behind a row's length were written"

    # ---- leg 5: roles that change from frame to frame
    if c.roles:
        roles = ref["legs"]["roles"]["roles"]
        rows_work = S.guarded("rows_work", L.lfi_flow_step_rows_work_floats(C.byref(dims)))
        s, states, cs = S.fresh(), {}, []
        for n in range(N):
            obs = (roles[n] == fq.OBS).to(dev)
            S.frames(s)[obs, START + n] = given[n].to(dev)[obs]
            role = obs.to(torch.int32).contiguous()
            S.upload()
            check(L.lfi_flow_step_rows_from(*S.args(s, n, 1, noise=True), S.work.ptr(), s["nll"].ptr() + 4 * n * B, S.nll_work.ptr(),
                                            role.data_ptr(), rows_work.ptr(), S.st), "step_rows_from")
            cs.append(S.front_of(n, n + 1, c.front))
            states[n] = S.state(s)
            sentinel_behind(s, n + 1, "roles")
        judge("roles", "roles", S.run_of(s, states, cs))

    # ---- every write stayed inside
    torch.cuda.synchronize()
    for name, gb in S.guards:
        assert gb.intact(), "guard band of " + name

    summary = {}
    for name, e, a, ok in all_rows:
        fam = name.split(" ")[1].split("[")[0]
        ratio = (e / a) if a > 0 else (0.0 if e == 0 else float("inf"))
        if fam not in summary or ratio >= summary[fam][0]:
            summary[fam] = (ratio, e, a, name)
    report("frame-drivers %-16s plan %2d  %-5s %s  %s" % (c.id, plan, c.front, " ".join(notes), "  ".join(
        "%s %.1e/%.1e=%.2f" % (v[3], v[1], v[2], v[0]) for k, v in sorted(summary.items()))))
    assert not fr.failures(all_rows), (c.id, fr.failures(all_rows))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_frame_drivers_vs_fp64(gpu_device, monkeypatch, c):
    """One case of the list above: plan and front end asserted, writes in bounds, every part of every leg within 3 x model + 8 x fp32
    of the fp64 reference."""
    if _gpu_error:
        pytest.fail("not run: an earlier case ended in a GPU error (%s)" % _gpu_error[0])
    t0 = time.time()
    try:
        run_case(c, gpu_device, monkeypatch)
    except AssertionError:
        raise
    except Exception as e:      # a HIP error is sticky: launch nothing more on this device from this module
        _gpu_error.append("%s: %s" % (c.id, str(e)[:200]))
        raise
    finally:
        print("%s: %.2f s" % (c.id, time.time() - t0))


def test_case_list_covers_the_table():
    """The list itself: every plan-bit combination of the table and both front ends, both sizes of sc_cond_kernel, the LSTM cell in
    chain and per-step form, a one-row last tile behind full ones in both tile sizes, C = 64, padding hidden units, the clamp,
    additive, dense and N = 1 among the raw-window cases; among the encoded ones every kind, the three window-encoder kernels a
    frame driver can reach and both recurrences of the fused ones, a padded feature pitch, a column offset that is no multiple of 4,
    windows that start 16-byte aligned on some frames only, every gemm_precision, one-step and start-of-faces windows, one row."""
    assert {c.expect for c in RAW_CASES} >= {31, 23, 15, 3, 21, 20, 0} and {c.front for c in RAW_CASES} == {FUSED, GEMMS}
    assert {(3 + c.lstm) * c.H for c in RAW_CASES if c.front == FUSED} == {384, 512}
    assert any(c.lstm and c.expect & 2 for c in RAW_CASES) and any(c.lstm and not c.expect & 2 for c in RAW_CASES)
    assert any(c.B > 16 and c.B % 16 == 1 and c.B > 64 and c.B % 64 == 1 for c in RAW_CASES)
    assert any(c.C == 64 for c in RAW_CASES) and any(c.H % 16 for c in RAW_CASES) and any(c.clamp for c in RAW_CASES)
    assert any(not c.affine for c in RAW_CASES) and any(c.dense for c in RAW_CASES) and any(c.N == 1 for c in RAW_CASES)
    assert {c.id for c in RAW_CASES if c.roles} == {"final-9", "final-5", "final-9-steps", "lstm128", "tiles", "odd"}
    assert all(c.Ks * -(-c.B // 16) <= 64 for c in RAW_CASES)
    E = ENC_CASES
    assert len(RAW_CASES) == 21 and len(E) >= 15 and len({c.id for c in CASES}) == len(CASES)
    assert all(c.front == GEMMS and c.hist1 <= START for c in E) and all(c.enc == "none" and c.hist1 == HIST1 for c in RAW_CASES)
    assert {c.enc for c in E} == {"mlp", "rnn", "lstm"} and {c.p for c in E if c.enc == "mlp"} == {0, 1, 9}
    assert {(c.evar, c.p == 1) for c in E if c.enc == "rnn"} >= {(2, True), (1, True), (1, False), (0, False)}
    assert all((c.evar is None) == (c.enc == "mlp") and (c.enc != "lstm" or c.evar == 0) for c in E)
    for kind in ("mlp", "rnn", "lstm"):
        assert any(c.enc == kind and c.ehid % 4 and c.col % 4 for c in E), kind
    assert all(c.N >= 4 for c in E if c.C == 50 and c.B > 1) and any(c.C % 4 and c.C != 50 for c in E)
    assert {c.hist1 for c in E} >= {1, 3, 4} and any(c.hist1 == START for c in E) and any(c.B == 1 for c in E)
    assert any(c.lstm and c.expect & 2 for c in E) and any(c.lstm and not c.expect & 2 for c in E) and any(c.B > 128 for c in E)
    assert all(c.Ks * -(-c.B // 16) <= 64 for c in E)
