"""Streaming sampling sessions (SeqGlow.open_stream -> GlowEngine.open_stream): SampleStream, one generated frame per call, and
StreamRows, the live rows that move between sessions. A session takes the engine it borrows as an argument (this module does not import
engine.py); the steps it shares with the batch sampler GlowEngine.sample - the prev_p1_face descriptor, the static cond_transform
product, the per-frame arithmetic and its range limit, the guard word, the stream policy - are GlowEngine's, defined there once."""
import collections
import contextlib
import ctypes as C
import functools
import operator
import os
import types
import warnings
import weakref

import torch

from ._lib import check, ptr, translate_oom

# engine attributes that a streaming session owns while one of its steps runs (SampleStream._owned): the workspaces every launch of
# the static part and the chain writes, and the per-parameter-state preparation they read (run_prep's outputs)
_SESSION_ATTRS = ("_ws", "prep", "wct_f", "_wct_planes", "_wc_r", "_cond_planes", "_enc_stash_f16")
_PARAMS_CHANGED = ("SampleStream: the model's parameters changed since open_stream (optimiser step, parameter load or "
                   "ActNorm init): a session samples with the weights of its open; open a new one")
_ROW_FIELDS = ("C", "H", "Ks", "rnn_type", "use_frame_nb", "windows", "hist1", "R")
_ABSENT = object()       # (an argument a call does not take, where None is a value to refuse)
_MAX_CANDIDATES = 256    # candidates per row of one step_candidates() call
_PENDING = ("SampleStream: %d candidates per row are pending (step_candidates): commit() one of them, or reset(), before any other "
            "call of the session")
_PENDING_ROLLOUTS = ("SampleStream: %d candidate rollouts of %d frames per row are pending (rollout_candidates): commit() one of them, "
                     "discard() them, or reset(), before any other call of the session")
_MAX_VIRTUAL_ROWS = 1 << 22   # B * ncand of one rollout_candidates() call: the limit of lfi_flow_sample_cand_seq_work_floats


def _stream():
    return torch.cuda.current_stream().cuda_stream


def check_return_nll(value):
    """The return_nll argument of the samplers (inference / sample / open_stream): a bool, checked before any launch."""
    if not isinstance(value, bool):
        raise TypeError("return_nll: expected a bool, got %s %r" % (type(value).__name__, value))


def _host_ints(name, x, strict=False):
    """The host-data argument `name`: a sequence of ints or a CPU integer tensor -> a list of ints. A tensor may be 1-D or (not
    strict) a scalar, never torch.bool; strict also refuses bools in a sequence."""
    wrong = "%s: expected a sequence of ints or a 1-D CPU integer tensor, got %s"
    if torch.is_tensor(x):
        if x.is_cuda or x.is_floating_point() or x.is_complex() or x.dtype == torch.bool or x.dim() > 1 or (strict and x.dim() != 1):
            raise ValueError(wrong % (name, "%s %s on %s" % (tuple(x.shape), x.dtype, x.device)))
        return x.reshape(-1).tolist()
    try:
        vals = list(x)
        if strict and any(isinstance(v, bool) for v in vals):
            raise TypeError
        return [operator.index(v) for v in vals]
    except TypeError:
        raise ValueError(wrong % (name, repr(x))) from None


def _index_list(name, idx, bound, where, count=None, distinct=True):
    """The index-list argument `name` of reset_rows / save_rows / load_rows: a sequence of ints or a 1-D CPU integer tensor -> a list
    of ints in [0, bound); `where` words what lies beyond. count: as many as that are wanted (None: any number but none at all);
    distinct: none may be listed twice."""
    idx = _host_ints(name, idx)
    if count is None and not idx:
        raise ValueError("%s: empty list" % name)
    if count is not None and len(idx) != count:
        raise ValueError("%s: %d listed for %d rows" % (name, len(idx), count))
    bad = [i for i in idx if not 0 <= i < bound]
    if bad:
        raise ValueError("%s: %s outside %s (0 .. %d)" % (name, bad, where, bound - 1))
    if distinct and len(set(idx)) != len(idx):
        raise ValueError("%s: %s listed more than once" % (name, sorted(i for i, c in collections.Counter(idx).items() if c > 1)))
    return idx


_KEY_MASK = (1 << 64) - 1
_POSITION_MOVES = {"step": 1, "observe": 1, "step_rows": 1, "step_many": "n", "observe_many": "n", "step_rows_many": "n",
                   "step_candidates": 0, "rollout_candidates": 0, "commit": "n", "discard": 0, "reset": 0}
_UNKEYED = "row_seeds: the session was opened without row_seeds (it draws from the process generator): open it with open_stream(row_seeds=...)"


def key_to_word(key):
    """A row key in [0, 2**64) -> the int64 with the same bit pattern, what the (B, 2) int64 row state holds (2**63 -> -2**63)."""
    if isinstance(key, bool) or not isinstance(key, int):
        raise ValueError("row_seeds: expected ints in [0, 2**64), got %s %r" % (type(key).__name__, key))
    if not 0 <= key <= _KEY_MASK:
        raise ValueError("row_seeds: %d outside [0, 2**64)" % key)
    return key - (1 << 64) if key >> 63 else key


def word_to_key(word):
    """key_to_word's inverse: an int64 of the row state -> the key in [0, 2**64)."""
    return int(word) & _KEY_MASK


def row_keys(row_seeds, count):
    """The row_seeds argument (open_stream / reset / reset_rows / load_rows / inference), host data checked before any launch: a
    sequence of `count` ints in [0, 2**64) - bools and floats are refused - or a 1-D CPU integer tensor of `count` entries taken as
    bit patterns (an int64 -1 is the key 2**64 - 1). Keys may repeat. -> the keys as a list of ints in [0, 2**64)."""
    vals = _host_ints("row_seeds", row_seeds, strict=True)
    if len(vals) != count:
        raise ValueError("row_seeds: %d listed for %d rows" % (len(vals), count))
    if torch.is_tensor(row_seeds):
        return [v & _KEY_MASK for v in vals]
    for v in vals:
        key_to_word(v)
    return vals


def row_position_advance(kind, n=1, lengths=None):
    """The position rules of the keyed noise as one pure function: how far a call of `kind` moves a row's
    position - the number of frames the row has taken since it was seeded, observed or generated, whoever supplied the noise. step,
    observe, step_rows: 1; step_many, observe_many, step_rows_many: n, a ragged observe_many lengths[r] per row; step_candidates
    and rollout_candidates: 0 (their draws are at (p, k) and (p + i, k), nothing is taken yet); commit: n - 1 after
    step_candidates, the rollouts' frame count after rollout_candidates; discard and the pending draws a reset() drops: 0. -> an
    int for every row, or (ragged) a list with one int per row."""
    move = _POSITION_MOVES.get(kind)
    if move is None:
        raise ValueError("row_position_advance: %r is not a kind of session call (%s)" % (kind, ", ".join(_POSITION_MOVES)))
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError("row_position_advance: n = %r is not a frame count" % (n,))
    if lengths is not None:
        if kind != "observe_many":
            raise ValueError("row_position_advance: only observe_many takes lengths, not %s" % kind)
        lens = [operator.index(v) for v in lengths]
        bad = [v for v in lens if not 0 <= v <= n]
        if bad:
            raise ValueError("row_position_advance: lengths %s outside 0 .. %d" % (bad, n))
        return lens
    return n if move == "n" else move


def plan_rows_many(all_observe, min_run):
    """The plan of a step_rows_many() round, a pure function of the mask (no device): all_observe[i] is true where EVERY row observes
    frame i. Maximal runs of at least min_run such frames go to the chunk forward chain (n + Ks - 1 cell times and one front end for
    n frames), everything else to the rows chain (n Ks cell times, n front ends); min_run 0 never uses the chunk chain. ->
    [(kind, first, count), ...] with kind "observe" or "rows", in frame order, covering every frame once."""
    flags = [bool(v) for v in all_observe]
    plan, i, n = [], 0, len(flags)
    while i < n:
        j = i + 1
        while j < n and flags[j] == flags[i]:
            j += 1
        kind = "observe" if flags[i] and min_run > 0 and j - i >= min_run else "rows"
        if plan and kind == "rows" and plan[-1][0] == "rows":
            plan[-1] = ("rows", plan[-1][1], plan[-1][2] + j - i)
        else:
            plan.append((kind, i, j - i))
        i = j
    return plan


class StreamRows:
    """The live state of n conversations taken out of a streaming session (SampleStream.save_rows): `data`, one contiguous float32
    (n, R) tensor of records, and `signature`, the record layout (C, H, Ks, rnn_type, use_frame_nb, ((name, hist, dim), ...), hist1,
    R). A record is, in order: every conditioning window of SampleStream.mods (hist x in_dim each), the faces window ((hist1 + 1) x
    C), h (Ks x H), c (Ks x H, LSTM only), the frame counter (one float, only with use_frame_nb) - the layout lfi_stream_row_floats
    defines. Plain fp32 values: independent of the session's batch size and per-frame arithmetic. load_rows puts entries back into
    rows of any session of the same model; cpu() / to(device) pause and resume, state_dict() / from_state_dict() store.

    `rng`: the rows' keyed-noise state, an (n, 2) int64 tensor beside `data` - (key, position) per entry as bit patterns - from a
    keyed session (open_stream(row_seeds=...)); None from an unkeyed one and for rows stored before the keys existed. It is not part
    of the float record or of `signature`."""

    def __init__(self, data, signature, _engine=None, _param_version=None, rng=None):
        self.data = data
        self.signature = self._canonical(signature)
        self._engine, self._param_version = _engine, _param_version   # (same-process check only: not part of state_dict())
        if rng is not None and not (torch.is_tensor(rng) and rng.dtype == torch.int64 and rng.dim() == 2
                                    and tuple(rng.shape) == (int(data.shape[0]), 2)):
            raise ValueError("StreamRows: rng: expected an int64 tensor (%d, 2), (key, position) per entry, got %s %s"
                             % (int(data.shape[0]), tuple(getattr(rng, "shape", ())), getattr(rng, "dtype", type(rng))))
        self.rng = rng

    @staticmethod
    def _canonical(sig):
        sig = tuple(sig)
        if len(sig) != len(_ROW_FIELDS):
            raise ValueError("StreamRows: a layout signature has %d fields %s, got %d" % (len(_ROW_FIELDS), _ROW_FIELDS, len(sig)))
        C_, H, Ks, rnn, nb, wins, hist1, R = sig
        return (int(C_), int(H), int(Ks), str(rnn), bool(nb), tuple((str(n), int(h), int(d)) for n, h, d in wins), int(hist1), int(R))

    def __len__(self):
        return int(self.data.shape[0])

    def _like(self, data, rng=None):
        return StreamRows(data, self.signature, self._engine, self._param_version, rng=rng)

    def cpu(self):
        return self._like(self.data.cpu(), None if self.rng is None else self.rng.cpu())

    def to(self, device):
        return self._like(self.data.to(device).contiguous(), None if self.rng is None else self.rng.to(device).contiguous())

    def select(self, indices):
        """The listed entries (repeats allowed), as a new StreamRows."""
        idx = torch.as_tensor(indices, dtype=torch.long, device=self.data.device).reshape(-1)
        return self._like(self.data.index_select(0, idx), None if self.rng is None else self.rng.index_select(0, idx.to(self.rng.device)))

    def state_dict(self):
        """One tensor and plain Python values (torch.save-able), and the key "rng" only for rows that carry keyed-noise state.
        Whether the weights are the ones the rows were saved under is the caller's responsibility once the rows leave the process."""
        d = dict(zip(_ROW_FIELDS, self.signature))
        d["windows"] = [list(w) for w in d["windows"]]
        d["data"] = self.data
        if self.rng is not None:
            d["rng"] = self.rng
        return d

    @classmethod
    def from_state_dict(cls, d):
        """state_dict()'s inverse; "rng" may be absent (rows of an unkeyed session, rows stored before the keys existed)."""
        missing = [k for k in _ROW_FIELDS + ("data",) if k not in d]
        if missing:
            raise KeyError("StreamRows.from_state_dict: missing %s" % missing)
        return cls(d["data"], tuple(d[k] for k in _ROW_FIELDS), rng=d.get("rng"))


class SampleStream:
    """Streaming autoregressive sampling: SeqGlow.inference (models.py:567-596) one frame per call, for a live agent whose
    conditioning arrives frame by frame. Open with `start` seed frames, then step(frame) with frame t of every modality with
    history > 0 -> the generated p1_face frame t (B, C). Given the same inputs and noise it produces what inference() produces.
    Opened with return_nll=True a step returns (frame, nll): nll (B,) is the frame's NLL in bits under the model, what forward() reports
    for it teacher-forced - the model's own density (temperature 1) at the prior draw the step was given, not a density of the
    tempered sampling distribution. It is an output of the step, not state: rows reseeded or loaded between steps report their own
    next frame's, and the row record does not hold it.

    Per step: lfi_stream_advance (one eager launch: the session's conditioning windows, its window of generated faces, the noise and
    the frame counter move forward by one frame), then the static part for B windows (window encoders + the static cond_transform
    columns, as _sample's static()) and lfi_flow_sample_seq_from (lfi_flow_sample_seq_nll with return_nll) for one frame, whose recurrent state h / c carries across steps. Those
    two touch only session-owned memory at fixed addresses: from the second step on they are ONE captured hipGraph, replayed.
    Every workspace they write is the session's own (the engine's `_ws`, prep and folded weights are swapped for the session's while a
    step runs), so training, inference() and other sessions can run between steps. Weights are frozen: a parameter change after the
    open (GlowEngine.param_version) makes step() raise."""

    # what commit() has not installed yet: None, ncand (an int) of the one-frame candidates step_candidates() left, or the rollouts
    # rollout_candidates() left - a namespace of their kind, ncand, n and buffers
    _pending = None
    # a keyed session's noise state (row_seeds): one (B, 2) int64 device tensor, (key, position) per row as bit patterns, allocated at
    # the open and never reallocated; None: the session draws from the process generator through noise_fn
    rng = None
    eps = None

    def __init__(self, eng, seed, noise_fn, masks_fn=None, bound=None, return_nll=False, row_seeds=None, eps=None):
        check_return_nll(return_nll)
        self.return_nll = return_nll            # fixed for the session: part of what the captured graph launches
        s = eng.spec
        self.eng = eng
        self._noise_fn, self._masks_fn, self._bound = noise_fn, masks_fn, bound
        p1 = seed.get("p1_face") if isinstance(seed, dict) else None
        if p1 is None:
            raise KeyError("batch is missing modality 'p1_face'")
        self.B = B = int(p1.shape[0]) if p1.dim() == 3 else -1
        self.start = s.start
        self.mods = [e for e in s.encoders if e.name not in ("p1_face", "frame_nb")]
        self._check_seed(seed)
        keys = None
        if row_seeds is not None:
            keys = row_keys(row_seeds, B)
            if isinstance(eps, bool) or not isinstance(eps, (int, float)):
                raise TypeError("eps: a keyed session (row_seeds) scales its own draws: expected a number, got %s %r"
                                % (type(eps).__name__, eps))
            self.eps = float(eps)
        self.device = eng.device
        self.closed = False
        self.param_version = eng.param_version
        self.precision = eng.precision          # GEMM arithmetic of the static part, fixed at the open
        self.steps = 0                          # frames generated since the open / the last reset()
        self.replays = 0                        # steps that were graph replays
        self._graph, self._graph_key = None, None                    # step()'s captured graph and what it was captured for
        self._observe_graphs = {}                                    # observe()'s own, by key
        self._rows_graphs = {}                                       # step_rows()'s own, by key
        self.score_work = self.obs_z = self.obs_nll = None   # observe()'s buffers: allocated at the first observe
        self.role = self.rows_work = self.rows_nll = self.rows_nll_work = None   # step_rows()'s: at the first step_rows
        self._cand, self._cand_graphs = {}, {}  # step_candidates()'s buffers, per ncand (a graph holds their addresses), and its graphs
        self._chunk_ws = {}                     # observe_many()'s / step_many()'s workspaces, sized by the chunk (the graphs never address them)
        self.last_plan = None                   # diagnostic: the last step_rows_many() call's plan (plan_rows_many), offsets in the call
        self._stream = None
        self._guard_pending = None
        self._state = {"_ws": {}, "prep": None, "wct_f": torch.zeros_like(eng.wct_f), "_wct_planes": None, "_wc_r": None,
                       "_cond_planes": None, "_enc_stash_f16": {}}
        e1 = s.encoders[0]
        self.hist1 = e1.hist
        self.c1 = (e1.fdim + 3) // 4 * 4
        with self._owned():
            eng.run_prep(with_inverse=True)
            self._p1 = eng._p1_enc()
            self._wp = eng._static_wct_planes(self.c1)   # the static cond_transform columns' weight planes: once per session (frozen weights)
            f = self.B * s.C
            self.faces = eng._buf("stream_faces", f * (self.hist1 + 1))[:f * (self.hist1 + 1)].view(B, self.hist1 + 1, s.C)
            self.noise = eng._buf("stream_noise", f)[:f].view(B, s.C)
            self.windows = {e.name: eng._buf("stream_win." + e.name, B * e.hist * e.in_dim)[:B * e.hist * e.in_dim].view(B, e.hist, e.in_dim)
                            for e in self.mods}
            self.frame_nb = eng._buf("stream_frame_nb", B)[:B] if s.use_frame_nb else None
            self.mask_bufs = {e.name: eng._buf("stream_mask." + e.name, B * e.hist)[:B * e.hist].view(1, B, e.hist)
                              for e in s.encoders if e.dropout > 0}
            self.cond = eng._buf("stream_cond", B * s.ldf)
            self.pre = eng._buf("stream_pre", B * s.Ks * s.D)
            self.h = eng._buf("stream_h", s.Ks * B * s.H)
            self.cs = eng._buf("stream_c", s.Ks * B * s.H) if s.rnn_type == "lstm" else None
            dims = eng._flow_dims(B, 1)
            self.work = eng._buf("stream_chain_work", eng.L.lfi_flow_sample_work_floats(C.byref(dims)))
            self.p1work = eng._buf("stream_p1work", eng.L.lfi_flow_sample_p1_work_floats(C.byref(dims), C.byref(self._p1), self.hist1))
            self.nll = eng._buf("stream_nll", B)[:B] if return_nll else None
            self.nll_work = eng._buf("stream_nll_work", eng.L.lfi_flow_sample_nll_work_floats(C.byref(dims))) if return_nll else None
            self.guard = eng._buf_i32("stream_guard_word", 1)
            self._pinned = torch.zeros(1, dtype=torch.int32).pin_memory()
            # per-frame arithmetic, picked once (as _sample picks it per call): fp16 pieces (9) when the parameters and the seed sit inside
            # their range, else six bf16 products (5); exact f32 (0) in f32 engine mode; LFI_SAMPLE_FRAME_PRECISION overrides
            fp = eng._frame_precision()
            if fp is None:
                fp = eng._guarded_frame_precision(eng._launch_range_guard(([eng.params] + eng._guarded(seed))[:8]))
            self.frame_precision = int(fp)
            # the session's windows in record order (mods, then the faces window), as the four entry points pass them: pointer, hist
            # and dim are fixed at the open; step() fills the frame pointers (none for the faces window), reset_rows the seed's
            self._wins = [(e.name, self.windows[e.name], e.hist, e.in_dim, 0) for e in self.mods] + \
                         [("p1_face", self.faces, self.hist1 + 1, s.C, 1)]
            k = len(self._wins)
            self._row_win, self._row_hist, self._row_dim = (C.c_void_p * k)(), (C.c_int * k)(), (C.c_int * k)()
            self._src_p, self._seed_p, self._seed_ld, self._lead = (C.c_void_p * k)(), (C.c_void_p * k)(), (C.c_long * k)(), (C.c_int * k)()
            for i, (_, w, hi, d, z) in enumerate(self._wins):
                self._row_win[i], self._row_hist[i], self._row_dim[i], self._lead[i] = w.data_ptr(), hi, d, z
            # the row record of save_rows / load_rows and its signature
            R = eng.L.lfi_stream_row_floats(k, self._row_hist, self._row_dim, s.Ks, s.H, int(self.cs is not None),
                                            int(self.frame_nb is not None))
            if R < 0:
                check(-1, "lfi_stream_row_floats")
            self.row_signature = (s.C, s.H, s.Ks, s.rnn_type, bool(s.use_frame_nb), tuple((e.name, e.hist, e.in_dim) for e in self.mods),
                                  self.hist1, int(R))
            if keys is not None:
                # the keyed session's state and the one-frame draw's buffer (the other layouts' are sized by their calls)
                self.rng = torch.zeros(B, 2, dtype=torch.int64, device=self.device)
                self.draw = eng._buf("stream_noise_draw", f)[:f].view(B, s.C)
                self._seed_rng(None, keys)
            self._fill(seed)

    # ---- validation (before any launch; the wording of GlowEngine._check_input)
    def _check_seed(self, seed, B=None):
        s = self.eng.spec
        B = self.B if B is None else B
        p1 = seed.get("p1_face")
        self.eng._check_input(p1, "p1_face", B, s.start, s.C)
        for e in self.mods:
            x = seed.get(e.name)
            if x is None:
                raise KeyError("batch is missing modality %r" % e.name)
            self.eng._check_input(x, e.name, B, s.start, e.in_dim)
            if x.device != p1.device:
                raise ValueError("%s: on %s, the seed's p1_face on %s" % (e.name, x.device, p1.device))

    def _check_tensor(self, x, name, axes, note=""):
        """The one check of a tensor argument, before any launch: contiguous float32 on the session's device, one axis per entry of
        axes - (its wording in the message, which takes the size as %d; the size, None: any number from one). note: what the message
        adds about the layout. -> the size of the first axis."""
        if not (torch.is_tensor(x) and x.is_cuda and x.device == self.device and x.dtype == torch.float32 and x.is_contiguous()
                and x.dim() == len(axes) and all(got >= 1 if want is None else got == want for got, (_, want) in zip(x.shape, axes))):
            raise ValueError("%s: expected contiguous float32 GPU tensor (%s) on %s%s, got %s %s on %s"
                             % (name, ", ".join(text if want is None else text % want for text, want in axes), self.device, note,
                                tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x)), getattr(x, "device", None)))
        return int(x.shape[0])

    @staticmethod
    def _frames_axis(n):
        """The axis of a chunk's frames: n of them, or (None) any number from one."""
        return ("n>=1", None) if n is None else ("n=%d", n)

    def _check_matrix(self, x, name, cols, rows=None):
        """A step's frame / noise (rows = B) or the records of saved rows (rows None: any number from one)."""
        self._check_tensor(x, name, (("n>=1", None), ("R=%d", cols)) if rows is None else (("B=%d", rows), ("%d", cols)))

    def _check_usable(self, pending_ok=False):
        if self.closed:
            raise RuntimeError("SampleStream: the session is closed")
        if self.eng.param_version != self.param_version or (self._bound is not None and not self._bound()):
            raise RuntimeError(_PARAMS_CHANGED)
        if self._pending is not None and not pending_ok:
            raise RuntimeError(self._pending_message())

    def _pending_message(self):
        pend = self._pending
        if getattr(pend, "kind", None) == "rollouts":
            return _PENDING_ROLLOUTS % (pend.ncand, pend.n)
        return _PENDING % pend

    # ---- session-owned engine state, on a stream that is not the legacy default one (the session's private stream for a caller on it)
    @contextlib.contextmanager
    def _owned(self):
        eng = self.eng
        with eng._off_legacy_stream(self, "_stream"):
            saved = {k: eng.__dict__.get(k) for k in _SESSION_ATTRS}
            keep_precision = eng.precision
            eng.__dict__.update(self._state)
            eng.precision = self.precision
            try:
                yield
            finally:
                self._state = {k: eng.__dict__.get(k) for k in _SESSION_ATTRS}
                eng.__dict__.update(saved)
                eng.precision = keep_precision

    # ---- public surface
    def reset(self, seed, row_seeds=None):
        """Start a new sequence from `seed` (same batch size); the captured graph is kept. Pending candidates and pending rollouts
        are dropped (their draws moved no position). A keyed session (open_stream(row_seeds=...)): with row_seeds - B keys, as
        open_stream's - every row takes its new key at position 0; with None every row KEEPS its key and restarts at position 0,
        which REPLAYS the same draws: the rows generate what they generated after the open, given the same seed and conditioning. A
        new conversation should be given its own key. row_seeds on an unkeyed session is a ValueError."""
        self._check_usable(pending_ok=True)
        self._check_seed(seed)
        keys = self._check_row_seeds(row_seeds, self.B)
        with self._owned():
            if self.rng is not None:
                self._seed_rng(None, keys)
            self._fill(seed)

    def reset_rows(self, rows, seed, row_seeds=None):
        """Start new sequences in the listed batch rows only, between steps (a conversation joins a batched session in a row another
        one left). rows: a sequence of distinct ints in [0, B), or a CPU integer tensor; seed: as reset()'s, with batch len(rows) -
        entry j goes to session row rows[j]. Every other row carries on undisturbed. One launch (lfi_stream_reset_rows), no host wait;
        the captured graph, `steps` (frames since the open / reset(), which also index injected masks) and the per-frame arithmetic
        are kept. A seed beyond the fp16 pieces' range is reported by the next steps' range guard, as a frame's would be.

        A keyed session (open_stream(row_seeds=...)): with row_seeds - len(rows) keys, entry j for row rows[j] - the listed rows take
        those keys at position 0; with None a listed row KEEPS its key and restarts at position 0, which REPLAYS the same draws: the
        row draws again what it drew after it was first seeded. A new conversation that joins in the row should be given its own
        key. The other rows' (key, position) are undisturbed. One more small launch (lfi_row_rng_seed_rows, the keys in its
        arguments), no host wait. row_seeds on an unkeyed session is a ValueError."""
        s, eng = self.eng.spec, self.eng
        self._check_usable()
        rows = _index_list("rows", rows, self.B, "the session's batch")
        n = len(rows)
        keys = self._check_row_seeds(row_seeds, n)
        p1 = seed.get("p1_face") if isinstance(seed, dict) else None
        if p1 is None:
            raise KeyError("batch is missing modality 'p1_face'")
        self._check_seed(seed, n)
        if p1.device != self.device:
            raise ValueError("p1_face: on %s, the session on %s" % (p1.device, self.device))
        seeds = [seed[name] for name, _, _, _, _ in self._wins]
        for i, (x, (_, _, hi, d, z)) in enumerate(zip(seeds, self._wins)):
            # frames start - (hist - z) .. start - 1 of every seed entry; z = 1: the window's frame 0 is zeroed instead
            self._seed_p[i], self._seed_ld[i] = x.data_ptr() + 4 * (s.start - (hi - z)) * d, x.shape[1] * d
        row_a = (C.c_int * n)(*rows)
        with self._owned():
            check(eng.L.lfi_stream_reset_rows(self.B, n, row_a, len(self._row_win), self._row_win, self._seed_p, self._seed_ld,
                                              self._row_hist, self._row_dim, self._lead, self.h.data_ptr(), ptr(self.cs), s.Ks, s.H,
                                              ptr(self.frame_nb), self.guard.data_ptr(), _stream()), "lfi_stream_reset_rows")
            if self.rng is not None:
                self._seed_rng(rows, keys)
            if self._stream is not None and torch.cuda.current_stream(self.device) == self._stream:
                for x in seeds:
                    x.record_stream(self._stream)

    def save_rows(self, rows):
        """The live state of the listed rows, between steps -> StreamRows with len(rows) entries, entry j = session row rows[j] (rows:
        as reset_rows'). One launch per 256 rows (lfi_stream_save_rows) on the caller's stream, no host wait; the session is not
        changed. A session that has not stepped since its open / reset() saves zeros for h / c: its first step ignores what those
        buffers hold."""
        s, eng = self.eng.spec, self.eng
        self._check_usable()
        rows = _index_list("rows", rows, self.B, "the session's batch")
        n, R = len(rows), self.row_signature[-1]
        row_a = (C.c_int * n)(*rows)
        with self._owned():
            out = torch.empty(n, R, dtype=torch.float32, device=self.device)
            check(eng.L.lfi_stream_save_rows(self.B, n, row_a, len(self._row_win), self._row_win, self._row_hist, self._row_dim,
                                             self.h.data_ptr(), ptr(self.cs), s.Ks, s.H, ptr(self.frame_nb),
                                             1 - self._first_frame, out.data_ptr(), R, _stream()),
                  "lfi_stream_save_rows")
            rng = None
            if self.rng is not None:            # a keyed session: the rows' (key, position) travel beside their records
                rng = torch.empty(n, 2, dtype=torch.int64, device=self.device)
                check(eng.L.lfi_row_rng_save_rows(self.rng.data_ptr(), self.B, n, row_a, rng.data_ptr(), _stream()), "lfi_row_rng_save_rows")
        if self._stream is not None:
            out.record_stream(torch.cuda.current_stream(self.device))
            if rng is not None:
                rng.record_stream(torch.cuda.current_stream(self.device))
        return StreamRows(out, self.row_signature, weakref.ref(eng), self.param_version, rng=rng)

    def load_rows(self, rows, saved, entries=None, row_seeds=None):
        """Put saved conversations into the listed rows, between steps: entry entries[j] of `saved` (a StreamRows of this model, from
        any session, batch size or device round trip) goes to session row rows[j]; entries defaults to range(len(rows)) and may
        repeat (a branch). Only the listed rows are written; one launch per 256 rows (lfi_stream_load_rows), no host wait; `steps`,
        the captured graph and the per-frame arithmetic are kept, and a value beyond the fp16 pieces' range is reported by the next
        steps' range guard, as a reseed's would be. Everything is checked before the first launch: a refused call leaves the
        session as it was. Into a session that has not stepped yet, h / c of every row are zeroed first and the first step runs as
        a continuing one (a zeroed row is a first frame's state).

        A keyed session (open_stream(row_seeds=...)): key and position arrive with the entry (saved.rng), so a moved row draws on
        exactly what it would have drawn where it was, and two rows loaded from one entry draw the SAME noise. row_seeds - len(rows)
        keys, entry j for row rows[j] - gives row rows[j] the new key and the entry's position: a branch that draws differently
        from its sibling from the next frame on. Saved rows without rng (from an unkeyed session, or stored before the keys
        existed) need row_seeds and start at position 0; without it, ValueError. One more small launch (lfi_row_rng_load_rows /
        lfi_row_rng_seed_rows, lists and keys in its arguments). An unkeyed session ignores saved.rng and refuses row_seeds."""
        s, eng = self.eng.spec, self.eng
        self._check_usable()
        rows = _index_list("rows", rows, self.B, "the session's batch")
        n = len(rows)
        if not isinstance(saved, StreamRows):
            raise TypeError("saved: expected a StreamRows (SampleStream.save_rows), got %s" % type(saved).__name__)
        keys = self._check_row_seeds(row_seeds, n)
        srng = saved.rng if self.rng is not None else None
        if self.rng is not None and srng is None and keys is None:
            raise ValueError("saved: the rows carry no keyed-noise state (rng is None: saved by an unkeyed session, or stored before "
                             "the keys existed) and the session is keyed: give row_seeds, one key per listed row (position 0)")
        if srng is not None and not (srng.is_cuda and srng.device == self.device and srng.is_contiguous()):
            raise ValueError("saved.rng: expected a contiguous int64 tensor (%d, 2) on %s, got one on %s (StreamRows.to(device) moves "
                             "it with the records)" % (len(saved), self.device, srng.device))
        for name, mine, theirs in zip(_ROW_FIELDS, self.row_signature, saved.signature):
            if mine != theirs:
                raise ValueError("saved: layout signature differs in %s: the session's is %r, the saved rows' %r" % (name, mine, theirs))
        R, x = self.row_signature[-1], saved.data
        self._check_matrix(x, "saved.data", R)
        entries = _index_list("entries", range(n) if entries is None else entries, len(saved), "the saved rows", count=n, distinct=False)
        if saved._engine is not None and saved._engine() is eng and saved._param_version != self.param_version:
            raise RuntimeError(_PARAMS_CHANGED)
        row_a, ent_a = (C.c_int * n)(*rows), (C.c_int * n)(*entries)
        with self._owned():
            self._zero_state_if_fresh(resumed=False)        # (marked below, after the launch)
            check(eng.L.lfi_stream_load_rows(self.B, n, row_a, ent_a, len(saved), len(self._row_win), self._row_win, self._row_hist,
                                             self._row_dim, self.h.data_ptr(), ptr(self.cs), s.Ks, s.H, ptr(self.frame_nb),
                                             x.data_ptr(), R, self.guard.data_ptr(), _stream()), "lfi_stream_load_rows")
            if srng is not None:
                key_a = None if keys is None else (C.c_ulonglong * n)(*keys)
                check(eng.L.lfi_row_rng_load_rows(self.rng.data_ptr(), self.B, n, row_a, ent_a, len(saved), srng.data_ptr(), key_a,
                                                  _stream()), "lfi_row_rng_load_rows")
                if self._stream is not None and torch.cuda.current_stream(self.device) == self._stream:
                    srng.record_stream(self._stream)
            elif self.rng is not None:
                self._seed_rng(rows, keys)
            if self.steps == 0:
                self._resumed = True    # the session's first _launch then keeps h / c (first_frame = 1)
            if self._stream is not None and torch.cuda.current_stream(self.device) == self._stream:
                x.record_stream(self._stream)

    @property
    def _first_frame(self):
        """The first_frame argument of the chains: 0 = the launch ignores what h / c hold (nothing stepped or loaded since the open /
        reset()), 1 = it carries them on."""
        return 1 if self.steps > 0 or self._resumed else 0

    def _zero_state_if_fresh(self, resumed=True):
        """Before rows are put into a session that has not stepped yet: h / c of every row zeroed (stale after a reset(); the first
        launch would have ignored them - a zeroed row is a first frame's state), so that the first launch can run as a continuing
        one; resumed: mark it so now."""
        if self._first_frame:
            return
        self.h.zero_()
        if self.cs is not None:
            self.cs.zero_()
        if resumed:
            self._resumed = True

    # ---- keyed noise (row_seeds): eager launches on the step's stream inside _owned(), never inside a captured region; host lists go
    # to the device by value in the kernel arguments
    def _check_row_seeds(self, row_seeds, count):
        """The row_seeds argument of reset / reset_rows / load_rows, before any launch -> the keys as a list, or None."""
        if row_seeds is None:
            return None
        if self.rng is None:
            raise ValueError(_UNKEYED)
        return row_keys(row_seeds, count)

    def _seed_rng(self, rows, keys):
        """(key, position 0) into the listed rows (None: every row) of the row state; keys None: each row keeps its key."""
        n = self.B if rows is None else len(rows)
        row_a = None if rows is None else (C.c_int * n)(*rows)
        key_a = None if keys is None else (C.c_ulonglong * n)(*keys)
        check(self.eng.L.lfi_row_rng_seed_rows(self.rng.data_ptr(), self.B, n, row_a, key_a, None, _stream()), "lfi_row_rng_seed_rows")

    def _rng_advance(self, kind, n=1, lens=None, words=None):
        """A keyed session's positions move by row_position_advance(kind, n, lens) for frames taken WITHOUT a draw of the session's
        own (observed frames, a caller's noise=, a commit): lfi_row_rng_advance. words: the ragged lengths on the device."""
        if self.rng is None:
            return
        move = row_position_advance(kind, n, lens)
        if lens is None and move == 0:
            return
        check(self.eng.L.lfi_row_rng_advance(self.rng.data_ptr(), self.B, 0 if lens is not None else move,
                                             None if lens is None else words.data_ptr(), _stream()), "lfi_row_rng_advance")

    def _draw(self, kind, out, n=None, ncand=None):
        """A keyed session's own draw for a call of `kind`, already * eps: ONE lfi_row_noise launch into the session-owned `out` of the
        call's layout - (B, C), (B, ncand, C), (n, B, C) or (n, B, ncand, C) - at positions p .. p + n - 1, candidates 0 .. ncand - 1,
        that moves the positions by row_position_advance(kind, n) in the same launch. -> out."""
        return self.eng.row_noise(self.rng, n=n, ncand=ncand, eps=self.eps, advance=row_position_advance(kind, 1 if n is None else n),
                                  out=out)

    def row_rng(self):
        """The keyed session's row state -> a (B, 2) int64 CPU copy, (key, position) per row as bit patterns (word_to_key gives the key
        in [0, 2**64)). The one call of the keyed path that waits for the device: for tests and logging."""
        self._check_usable(pending_ok=True)
        if self.rng is None:
            raise ValueError(_UNKEYED)
        return self.rng.cpu()

    def _fill(self, seed):
        s, h1 = self.eng.spec, self.hist1
        self.faces[:, 0].zero_()    # (row 0 leaves with the first step's shift)
        self.faces[:, 1:].copy_(seed["p1_face"][:, s.start - h1:s.start])
        for e in self.mods:
            self.windows[e.name].copy_(seed[e.name][:, s.start - e.hist:s.start])
        if self.frame_nb is not None:
            self.frame_nb.fill_(-1.0)   # the first step's + 2 makes it inference's 1
        self.guard.zero_()
        self.steps = 0
        self._resumed = False           # load_rows into a session that has not stepped sets it: the first launch keeps h / c
        self._guard_pending = None
        self._pending = None

    def close(self):
        """Releases the session's buffers and graph; step() raises afterwards."""
        if self.closed:
            return
        if self._stream is not None:
            self._stream.synchronize()
        self.closed = True
        self._graph, self._observe_graphs, self._rows_graphs = None, {}, {}
        self._cand, self._cand_graphs, self._pending = None, {}, None
        self._state = self._chunk_ws = None
        self.faces = self.noise = self.windows = self.cond = self.pre = self.h = self.cs = self.work = self.p1work = self._wins = None
        self.nll = self.nll_work = self.score_work = self.obs_z = self.obs_nll = None
        self.role = self.rows_work = self.rows_nll = self.rows_nll_work = None
        self.rng = self.draw = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check_frame(self, frame):
        """The conditioning argument of step() / observe(), checked before any launch -> the new frames in the order of self.mods."""
        if not isinstance(frame, dict):
            raise TypeError("frame must be a dict {modality: (B, dim) tensor}")
        srcs = []
        for e in self.mods:
            x = frame.get(e.name)
            if x is None:
                raise KeyError("batch is missing modality %r" % e.name)
            self._check_matrix(x, e.name, e.in_dim, self.B)
            srcs.append(x)
        return srcs

    @translate_oom
    def step(self, frame, noise=None):
        """frame: {modality: (B, dim)} = frame t of every modality with history > 0 (extra keys are ignored). noise: (B, C) prior
        draw already * eps, or None (drawn with the session's eps). -> generated p1_face frame t, (B, C); a session opened with
        return_nll=True -> (frame, nll), nll (B,) float32: the frame's NLL in bits (see the class)."""
        s = self.eng.spec
        self._check_usable()
        srcs = self._check_frame(frame)
        if noise is not None:
            self._check_matrix(noise, "noise", s.C, self.B)
        with self._owned():
            self._check_guard()
            if noise is None:
                noise = self._noise_fn(self.B, s.C).contiguous() if self.rng is None else self._draw("step", self.draw)
            else:
                self._rng_advance("step")
            self._advance(srcs, noise, None)
            out = self.faces[:, self.hist1].clone()
            nll = self.nll.clone() if self.return_nll else None
            self.steps += 1
        self._record_out(out, nll)
        return (out, nll) if self.return_nll else out

    @translate_oom
    def observe(self, frame, face, return_z=False):
        """A teacher-forced step: frame t of p1_face is GIVEN (recorded, puppeteered, rendered by another system) instead of sampled.
        frame: as step()'s; face: (B, C) float32 GPU tensor, the observed p1_face frame t. -> nll (B,) float32, the frame's NLL in
        bits under the model - what forward() reports for it - or (nll, z) with return_z, z (B, C) its latent. The frame enters the
        session's faces window and the recurrent state h / c moves on exactly as a generated frame's does (the coupling cells see the
        pass-through half and the conditioning, the same in both directions), so step() and observe() alternate freely: warm a
        session up on real history, score faces live, hand over in either direction. Works whether return_nll is on or off.

        Per call: lfi_stream_advance with the observed frame as the faces window's source (it passes the range guard there), the
        static part as a step's, then lfi_flow_score_seq_from for one frame: the sampler's conditioning front end and ALL forward
        flow steps in one launch. From the second call on, one captured hipGraph of its own, keyed as the step graph is (and on return_z: the latent is
        written only when asked for). No host wait
        in steady state. `steps` counts both kinds of step."""
        s = self.eng.spec
        self._check_usable()
        if not isinstance(return_z, bool):
            raise TypeError("return_z: expected a bool, got %s %r" % (type(return_z).__name__, return_z))
        srcs = self._check_frame(frame)
        self._check_matrix(face, "face", s.C, self.B)
        with self._owned():
            self._check_guard()
            if self.obs_nll is None:     # the observe buffers: at the first observe, outside capture
                eng, dims = self.eng, self.eng._flow_dims(self.B, 1)
                self.score_work = eng._buf("stream_score_work", eng.L.lfi_flow_score_work_floats(C.byref(dims)))
                self.obs_z = eng._buf("stream_obs_z", self.B * s.C)[:self.B * s.C].view(self.B, s.C)
                self.obs_nll = eng._buf("stream_obs_nll", self.B)[:self.B]
            self._rng_advance("observe")
            self._advance(srcs, None, face, return_z)
            nll = self.obs_nll.clone()
            z = self.obs_z.clone() if return_z else None
            self.steps += 1
        self._record_out(nll, z)
        return (nll, z) if return_z else nll

    @staticmethod
    def _check_ncand(ncand):
        """The ncand argument of step_candidates() / step_best_of(): an int in 1 .. 256, checked before any launch."""
        if isinstance(ncand, bool) or not isinstance(ncand, int):
            raise TypeError("ncand: expected an int, got %s %r" % (type(ncand).__name__, ncand))
        if not 1 <= ncand <= _MAX_CANDIDATES:
            raise ValueError("ncand: %d outside 1 .. %d" % (ncand, _MAX_CANDIDATES))
        return ncand

    def _check_cand_noise(self, noise, ncand):
        """The candidates' prior draws, (B, ncand, C)."""
        B, C_ = self.B, self.eng.spec.C
        self._check_tensor(noise, "noise", (("B=%d", B), ("ncand=%d", ncand), ("%d", C_)))

    def _cand_buffers(self, ncand):
        """The buffers of step_candidates() for `ncand` candidates per row: at the first use of that ncand, outside capture, and kept -
        the graph of an ncand holds their addresses."""
        c = self._cand.get(ncand)
        if c is None:
            s, eng, B = self.eng.spec, self.eng, self.B
            V, tag = B * ncand, ".%d" % ncand
            dims = eng._flow_dims(B, 1)
            floats = eng.L.lfi_flow_sample_cand_work_floats(C.byref(dims), ncand)
            if floats <= 0:
                raise ValueError("ncand: %d candidates for each of %d rows are more than one call takes" % (ncand, B))
            c = self._cand[ncand] = types.SimpleNamespace(
                noise=eng._buf("stream_cand_noise" + tag, V * s.C)[:V * s.C].view(B, ncand, s.C),
                frames=eng._buf("stream_cand_frames" + tag, V * s.C)[:V * s.C].view(B, ncand, s.C),
                nll=eng._buf("stream_cand_nll" + tag, V)[:V].view(B, ncand),
                h=eng._buf("stream_cand_h" + tag, s.Ks * V * s.H),
                c=eng._buf("stream_cand_c" + tag, s.Ks * V * s.H) if self.cs is not None else None,
                work=eng._buf("stream_cand_work" + tag, floats),
                draw=eng._buf("stream_cand_draw" + tag, V * s.C)[:V * s.C].view(B, ncand, s.C) if self.rng is not None else None,
                choice=eng._buf_i32("stream_cand_choice" + tag, B)[:B])
        return c

    @translate_oom
    def step_candidates(self, frame, ncand, noise=None):
        """ncand CANDIDATES for frame t of every row (best-of-N on a live conversation), from which commit() installs one. frame: as
        step()'s; ncand: an int in 1 .. 256; noise: (B, ncand, C) contiguous float32 on the session's device, the candidates' prior
        draws already * eps - a temperature per candidate is the caller's choice - or None: ncand draws of the session's own, stacked
        on dim 1. -> (faces, nll): faces (B, ncand, C), nll (B, ncand) float32 in bits - both always, whatever return_nll the
        session was opened with. Candidate j of row r is what step(frame, noise[:, j]) generates and reports for row r, bit for bit
        on the one-launch chain (rows never mix inside a cell); where the per-step launches run instead - wide flows,
        LFI_SAMPLE_CHAIN=0, LFI_FLOW_GENERIC=1 - to the session's gates.

        Within one frame the candidates of a row share their conditioning windows, their faces window and their incoming h / c. Per
        call: lfi_stream_advance exactly as a step's (the windows and the frame counter move on; the candidates' noise goes to a
        session-owned buffer and passes the range guard), the static part for B windows, then lfi_flow_sample_cand_from: the
        conditioning front end for B rows and the reverse chain over B * ncand virtual rows that read their parent row's gic and
        state in place. In train mode the candidates share their row's dropout masks. From the second frame on, one captured
        hipGraph of its own per (per-frame arithmetic, masks injected, ncand), replayed; no host wait in steady state.

        The call leaves the session PENDING: the newest slot of the faces window and h / c are not written yet and `steps` has not
        moved. Until commit() - or reset(), which drops the candidates - every other call of the session raises RuntimeError."""
        s = self.eng.spec
        self._check_usable()
        ncand = self._check_ncand(ncand)
        srcs = self._check_frame(frame)
        if noise is not None:
            self._check_cand_noise(noise, ncand)
        with self._owned():
            self._check_guard()
            cand = self._cand_buffers(ncand)
            if noise is None and self.rng is not None:
                noise = self._draw("step_candidates", cand.draw, ncand=ncand)
            elif noise is None:
                noise = torch.stack([self._noise_fn(self.B, s.C) for _ in range(ncand)], 1).contiguous()
            self._advance(srcs, noise, None, ncand=ncand)
            faces, nll = cand.frames.clone(), cand.nll.clone()
            self._pending = ncand
        self._record_out(faces, nll)
        return faces, nll

    def _check_choice(self, choice, ncand):
        """commit()'s choice, checked before any launch -> (a (B,) integer tensor on the session's device, which the kernel clamps,
        or None; host data as a validated list of B ints in 0 .. ncand - 1, or None)."""
        if choice is None:
            return None, None
        if torch.is_tensor(choice) and choice.is_cuda:
            if choice.device != self.device:
                raise ValueError("choice: on %s, the session on %s" % (choice.device, self.device))
            if choice.dtype not in (torch.int32, torch.int64) or tuple(choice.shape) != (self.B,):
                raise ValueError("choice: expected %d entries (B,) of int32 / int64, got %s %s" % (self.B, tuple(choice.shape), choice.dtype))
            return choice, None
        return None, _index_list("choice", choice, ncand, "the row's candidates", count=self.B, distinct=False)

    def _upload_choice(self, buf, dev, host):
        """commit()'s choice (_check_choice's pair) into the (B,) int32 device buffer the commit kernel reads; neither: the kernel picks."""
        if dev is not None:
            buf.copy_(dev)
            dev.record_stream(torch.cuda.current_stream(self.device))
        elif host is not None:
            buf.copy_(torch.tensor(host, dtype=torch.int32).pin_memory(), non_blocking=True)

    @translate_oom
    def commit(self, choice=None):
        """Install one of the pending candidates of every row (step_candidates) as the row's frame t. choice: None - each row's
        candidate of least NLL, picked on the device (ties to the lowest index; a NaN never wins unless all are NaN, then 0) - or a
        (B,) int32 / int64 tensor on the session's device, clamped into 0 .. ncand - 1 by the kernel, or a host sequence / CPU
        integer tensor of B ints in that range, copied in asynchronously. -> (frame (B, C), nll (B,), choice (B,) int32): the
        installed candidates. One launch (lfi_stream_commit_cand), no host wait: the frame enters the newest slot of the faces window,
        the candidate's h / c become the row's, `steps` += 1 - the session is exactly where step(frame, noise[r, choice[r]]) per row
        would have left it, and no longer pending.

        With ROLLOUTS pending (rollout_candidates): the same three forms of choice; None picks, per row, the rollout of least SUMMED
        NLL on the device - the sum runs over the frames in ascending order in fp32, ties to the lowest index, a NaN sum never wins
        unless all are NaN, then 0. -> (out (B, n, C), nll (n, B), choice (B,) int32). The session is exactly where
        step_many(frames, noise[:, r, choice[r]]) per row would have left it: the conditioning windows advance by the n frames, the
        faces window holds the chosen sequence's last hist1 + 1 frames (old frames among them when n is small), h / c are the
        chosen candidate's after its last frame, the frame counter += 2 n, `steps` += n, and the committed frames are folded into
        the range guard. Two launches (lfi_stream_chunk_out for the conditioning windows, lfi_stream_commit_cand_seq), no host
        wait."""
        s, eng, B = self.eng.spec, self.eng, self.B
        self._check_usable(pending_ok=True)
        ncand = self._pending
        if ncand is None:
            raise RuntimeError("SampleStream: commit() without pending candidates (step_candidates comes first)")
        if getattr(ncand, "kind", None) == "rollouts":
            return self._commit_rollouts(ncand, choice)
        dev, host = self._check_choice(choice, ncand)
        with self._owned():
            cand = self._cand[ncand]
            self._upload_choice(cand.choice, dev, host)
            out = torch.empty(B, s.C, dtype=torch.float32, device=self.device)
            nll = torch.empty(B, dtype=torch.float32, device=self.device)
            picked = torch.empty(B, dtype=torch.int32, device=self.device)
            check(eng.L.lfi_stream_commit_cand(B, ncand, s.C, s.Ks, s.H, None if choice is None else cand.choice.data_ptr(),
                                               cand.frames.data_ptr(), cand.nll.data_ptr(), cand.h.data_ptr(), ptr(cand.c),
                                               self.faces.data_ptr(), self.hist1 + 1, self.h.data_ptr(), ptr(self.cs), out.data_ptr(),
                                               nll.data_ptr(), picked.data_ptr(), self.guard.data_ptr(), _stream()),
                  "lfi_stream_commit_cand")
            self._rng_advance("commit", 1)
            self._pending = None
            self.steps += 1
        self._record_out(out, nll, picked)
        return out, nll, picked

    def step_best_of(self, frame, ncand, noise=None):
        """step_candidates(frame, ncand, noise) followed by commit(): every row's candidate of least NLL becomes its frame t. ->
        commit()'s (frame, nll, choice)."""
        self.step_candidates(frame, ncand, noise)
        return self.commit()

    def _check_rollout_noise(self, noise, n, ncand):
        """The prior draws of rollout_candidates(), (n, B, ncand, C) frame-major with n >= 1 (None: whatever it has) -> n."""
        B, C_ = self.B, self.eng.spec.C
        return self._check_tensor(noise, "noise", (self._frames_axis(n), ("B=%d", B), ("ncand=%d", ncand), ("%d", C_)), ", frame-major")

    def _rollout_cap(self, ncand):
        """Frames one rollout_candidates() call takes for ncand candidates per row - a rollout is ONE round, its candidates live in
        the chunk workspaces until commit() / discard(). _chunk_cap()'s formula with the B * ncand virtual rows in place of B for
        everything that is per candidate (gic, the tiles, the hand-over words) and B for what the candidates share (the static
        pre-activations, the features); never more than _chunk_cap(); LFI_OBSERVE_CHUNK_FRAMES caps it as it caps a chunk round."""
        cap = self._chunk_cap()
        if os.environ.get("LFI_OBSERVE_CHUNK_FRAMES"):
            return cap
        s = self.eng.spec
        G = (4 if s.rnn_type == "lstm" else 3) * s.H
        per_frame = self.B * (s.Ks * s.D + s.ldf) + self.B * ncand * s.Ks * (G + s.C + 1)
        return min(cap, max(8, min(256, (64 << 20) // per_frame)))

    @translate_oom
    def rollout_candidates(self, frames, ncand, noise=None):
        """ncand candidate ROLLOUTS of n frames for every row (best-of-N over a short gesture, under conditioning known or
        hypothesised ahead), of which commit() installs one and discard() drops all. frames: as step_many()'s, {modality: (B, n,
        dim)}; ncand: an int in 1 .. 256; noise: (n, B, ncand, C) contiguous float32 on the session's device, the prior draws already
        * eps, or None: n * ncand draws of the session's own, frame-major, then candidate. -> (faces, nll): faces (B, ncand, n, C),
        nll (n, B, ncand) float32 in bits - both always, whatever return_nll the session was opened with. Candidate j of row r is
        the continuation step_many(frames, noise[:, :, j]) generates for row r: within a row the candidates share the conditioning
        frames, the dropout masks of a train-mode session (drawn once per call, as step_many draws them, before the noise) and the
        incoming windows and h / c; they differ in their prior draws and in everything those cause - from the second frame on each
        has its own faces window and its own h / c. Bit for bit where the fused front end and the one-launch chain run (rows never
        mix in either); with ncand = 1 on every path (the same launches on the same shapes); elsewhere to the session's gates (the
        front-end GEMMs run over B * ncand rows and may tile differently).

        THE SESSION DOES NOT MOVE - unlike step_candidates(), which advances the windows: a rollout under hypothesised conditioning
        must be droppable. Nothing the session owns is written: not the conditioning windows, not the faces window, h / c, the frame
        counter or `steps`. The call leaves the session PENDING: until commit(), discard() or reset() every other call raises
        RuntimeError.

        Per call: lfi_stream_chunk_gen_in (the windows as sequences in the chunk workspaces), the static part in sequence mode ONCE
        for the n frames of the B rows - not for B * ncand - lfi_stream_cand_seq_in (each row's faces sequence and h / c broadcast
        to its candidates, the noise through the range guard) and lfi_flow_sample_cand_seq: the sampler over B * ncand virtual rows
        that read their parent row's static pre-activations in place. Eager launches, no graph, no host wait; `replays` is untouched
        and the per-frame graphs stay valid. ONE round only: n is at most _rollout_cap(ncand) frames, and B * ncand at most 2^22 -
        beyond either, ValueError. Everything is checked before the first launch: a refused call leaves the session as it was."""
        s, eng, B = self.eng.spec, self.eng, self.B
        self._check_usable()
        ncand = self._check_ncand(ncand)
        srcs, n, _ = self._check_frames(frames)
        if noise is None and n is None:
            raise ValueError("noise: a model without conditioning windows takes its frame count from the noise, (n, B=%d, ncand=%d, %d)"
                             % (B, ncand, s.C))
        if noise is not None:
            n = self._check_rollout_noise(noise, n, ncand)
        V = B * ncand
        if V > _MAX_VIRTUAL_ROWS:
            raise ValueError("ncand: %d candidates for each of %d rows are %d virtual rows, more than one call takes (at most %d)"
                             % (ncand, B, V, _MAX_VIRTUAL_ROWS))
        cap = self._rollout_cap(ncand)
        if n > cap:
            raise ValueError("frames: %d frames of %d candidates for each of %d rows are more than the one round a rollout is (at most "
                             "%d frames)" % (n, ncand, B, cap))
        used = list(srcs)
        srcs.append(None)                       # (the faces window has no source: the chain writes the candidates' frames)
        with self._chunk_call(n, used) as rounds:
            (_, _, masks), = rounds             # (n <= _rollout_cap() <= _chunk_cap(): one round)
            L = eng.L
            if noise is None and self.rng is not None:
                f = n * V * s.C
                noise = self._draw("rollout_candidates", eng._buf("rollout_noise_draw", f)[:f].view(n, B, ncand, s.C), n=n, ncand=ncand)
            elif noise is None:
                noise = torch.stack([torch.stack([self._noise_fn(B, s.C) for _ in range(ncand)], 1) for _ in range(n)]).contiguous()
            used.append(noise)
            k, T = len(self._wins), s.start + n
            dims = eng._flow_dims(B, n)
            floats = L.lfi_flow_sample_cand_seq_work_floats(C.byref(dims), ncand)
            if floats <= 0:
                raise ValueError("ncand: %d candidates for each of %d rows are more than one call takes" % (ncand, B))
            seqs, seq_p, src_p = self._chunk_seqs(srcs, n)
            ev = eng._tic("stream_chunk_in")
            # (the guard fold of gen_in reads an (n, B, C) block: the first n * B * C of the candidates' draws, all of which
            # lfi_stream_cand_seq_in folds anyway)
            check(L.lfi_stream_chunk_gen_in(B, n, s.start, k, self._row_win, src_p, seq_p, self._row_hist, self._row_dim, self._lead,
                                            k - 1, noise.data_ptr(), s.C, self.guard.data_ptr(), _stream()), "lfi_stream_chunk_gen_in")
            eng._toc("stream_chunk_in", ev)
            pre = self._chunk_static(seqs, n, masks)
            dv = eng._flow_dims(V, n)
            dv.gemm_precision = self.frame_precision
            p = eng._flow_params()
            r = types.SimpleNamespace(
                kind="rollouts", ncand=ncand, n=n, seq_p=seq_p,
                seq=eng._buf("rollout_seq", V * T * s.C)[:V * T * s.C].view(B, ncand, T, s.C),
                nll=eng._buf("rollout_nll", n * V)[:n * V].view(n, B, ncand),
                h=eng._buf("rollout_h", s.Ks * V * s.H),
                c=eng._buf("rollout_c", s.Ks * V * s.H) if self.cs is not None else None,
                choice=eng._buf_i32("rollout_choice", B)[:B])
            work = eng._buf("rollout_work", floats)
            p1work = eng._buf("rollout_p1work", L.lfi_flow_sample_p1_work_floats(C.byref(dv), C.byref(self._p1), self.hist1))
            nll_work = eng._buf("rollout_nll_work", L.lfi_flow_sample_nll_work_floats(C.byref(dv)))
            ev = eng._tic("stream_rollout_in")
            check(L.lfi_stream_cand_seq_in(B, ncand, n, s.start, s.C, s.Ks, s.H, seqs["p1_face"].data_ptr(), r.seq.data_ptr(),
                                           self.h.data_ptr(), ptr(self.cs), r.h.data_ptr(), ptr(r.c), self._first_frame,
                                           noise.data_ptr(), self.guard.data_ptr(), _stream()), "lfi_stream_cand_seq_in")
            eng._toc("stream_rollout_in", ev)
            ev = eng._tic("stream_rollout_chain")
            check(L.lfi_flow_sample_cand_seq(C.byref(dv), C.byref(p), eng.prep.data_ptr(), eng.wct_f.data_ptr(), s.ldf, self.hist1,
                                             pre.data_ptr(), noise.data_ptr(), r.seq.data_ptr(), T, s.start, n, self._first_frame,
                                             r.h.data_ptr(), ptr(r.c), C.byref(self._p1), p1work.data_ptr(), work.data_ptr(),
                                             r.nll.data_ptr(), nll_work.data_ptr(), ncand, _stream()), "lfi_flow_sample_cand_seq")
            eng._toc("stream_rollout_chain", ev)
            faces, nll = r.seq[:, :, s.start:].contiguous(), r.nll.clone()
            self._pending = r
        self._record_out(faces, nll)
        return faces, nll

    def _commit_rollouts(self, r, choice):
        """commit() with rollouts pending: lfi_stream_chunk_out over the conditioning windows (they advance by the n frames the
        rollout was conditioned on) and lfi_stream_commit_cand_seq - the chosen candidate's frames, the tail of its faces sequence,
        its h / c, its NLL words, the frame counter += 2 n - then `steps` += n. -> (out (B, n, C), nll (n, B), choice (B,) int32)."""
        s, eng, B = self.eng.spec, self.eng, self.B
        n, ncand = r.n, r.ncand
        dev, host = self._check_choice(choice, ncand)
        with self._owned():
            L = eng.L
            self._upload_choice(r.choice, dev, host)
            out = torch.empty(B, n, s.C, dtype=torch.float32, device=self.device)
            nll = torch.empty(n, B, dtype=torch.float32, device=self.device)
            picked = torch.empty(B, dtype=torch.int32, device=self.device)
            k = len(self._wins) - 1             # the conditioning windows: every window but the last, the faces window
            ev = eng._tic("stream_rollout_commit")
            if k:
                check(L.lfi_stream_chunk_out(B, n, s.start, k, self._row_win, r.seq_p, self._row_hist, self._row_dim, self._lead, None,
                                             _stream()), "lfi_stream_chunk_out")
            check(L.lfi_stream_commit_cand_seq(B, ncand, n, s.start, s.C, s.Ks, s.H, None if choice is None else r.choice.data_ptr(),
                                               r.seq.data_ptr(), r.nll.data_ptr(), r.h.data_ptr(), ptr(r.c), self.faces.data_ptr(),
                                               self.hist1 + 1, self.h.data_ptr(), ptr(self.cs), ptr(self.frame_nb), out.data_ptr(),
                                               nll.data_ptr(), picked.data_ptr(), self.guard.data_ptr(), _stream()),
                  "lfi_stream_commit_cand_seq")
            eng._toc("stream_rollout_commit", ev)
            self._rng_advance("commit", n)
            self._publish_guard()
            self._pending = None
            self.steps += n
        self._record_out(out, nll, picked)
        return out, nll, picked

    def discard(self):
        """Drop the pending rollouts (rollout_candidates): the session stays exactly where it was before them - every row's
        save_rows record, `steps` and what the next call generates - and is no longer pending. No launch. One-frame candidates
        (step_candidates) cannot be discarded: their call has moved the windows already."""
        self._check_usable(pending_ok=True)
        pend = self._pending
        if pend is None:
            raise RuntimeError("SampleStream: discard() without pending rollouts (rollout_candidates comes first)")
        if getattr(pend, "kind", None) != "rollouts":
            raise RuntimeError("SampleStream: discard() with %d one-frame candidates per row pending (step_candidates): their call has "
                               "moved the session's windows already - commit() one of them, or reset()" % pend)
        self._pending = None

    def rollout_best_of(self, frames, ncand, noise=None):
        """rollout_candidates(frames, ncand, noise) followed by commit(): every row's rollout of least summed NLL becomes its next
        n frames. -> commit()'s (out, nll, choice)."""
        self.rollout_candidates(frames, ncand, noise)
        return self.commit()

    def _check_chunk(self, x, name, cols, n=None):
        """A chunk's frames of one modality, (B, n, cols) with n >= 1 (None: whatever it has) -> n."""
        self._check_tensor(x, name, (("B=%d", self.B), self._frames_axis(n), ("%d", cols)))
        return int(x.shape[1])

    def _check_lengths(self, lengths, n):
        """The lengths argument of observe_many(): a sequence of B ints or a 1-D CPU integer tensor of B entries, each in [0, n] -> a
        list of ints. Host data, as reset_rows' rows; the wording of _index_list."""
        vals = _host_ints("lengths", lengths, strict=True)
        if len(vals) != self.B:
            raise ValueError("lengths: %d listed for %d rows" % (len(vals), self.B))
        bad = [v for v in vals if not 0 <= v <= n]
        if bad:
            raise ValueError("lengths: %s outside the chunk's frames (0 .. %d)" % (bad, n))
        return vals

    def _check_frames(self, frames, faces=_ABSENT, lengths=None):
        """The tensor arguments of a chunk call in the order they are checked, before any launch: frames, {modality: (B, n, dim)};
        faces, (B, n, C), where the call takes them; lengths, where given. n is the first tensor's, the same in all the others. ->
        (the frames in the order of self.mods, n - None when no tensor has said it yet -, lengths as a list or None)."""
        if not isinstance(frames, dict):
            raise TypeError("frames must be a dict {modality: (B, n, dim) tensor}")
        n = None if faces is _ABSENT else self._check_chunk(faces, "faces", self.eng.spec.C)
        lens = None if lengths is None else self._check_lengths(lengths, n)
        srcs = []
        for e in self.mods:
            x = frames.get(e.name)
            if x is None:
                raise KeyError("batch is missing modality %r" % e.name)
            n = self._check_chunk(x, e.name, e.in_dim, n)
            srcs.append(x)
        return srcs, n, lens

    def _check_noise_many(self, noise, n):
        """The prior draws of a chunk call, (n, B, C) frame-major with n >= 1 (None: whatever it has) -> n."""
        B, C_ = self.B, self.eng.spec.C
        return self._check_tensor(noise, "noise", (self._frames_axis(n), ("B=%d", B), ("%d", C_)), ", frame-major")

    def _chunk_cap(self):
        """Frames one launch of the chunk chain takes: its hand-over slots are per frame and never reused inside a launch, and the
        front end's operands (pre-activations, gic, features) grow with the frames too, so a long chunk runs as several calls with
        the state carried. As many as fit 64 Mi floats of them, between 8 and 256; LFI_OBSERVE_CHUNK_FRAMES overrides (tests: 3)."""
        env = os.environ.get("LFI_OBSERVE_CHUNK_FRAMES")
        if env:
            cap = int(env)
            if cap < 1:
                raise ValueError("LFI_OBSERVE_CHUNK_FRAMES: %r is not a frame count" % env)
            return cap
        s = self.eng.spec
        G = (4 if s.rnn_type == "lstm" else 3) * s.H
        per_frame = self.B * (s.Ks * (s.D + G + s.C + 1) + s.ldf)
        return max(8, min(256, (64 << 20) // per_frame))

    @translate_oom
    def observe_many(self, frames, faces, return_z=False, lengths=None):
        """n teacher-forced steps in one call, for frames known up front (recorded history a conversation joins with, a clip to
        score): exactly what n successive observe(frame_i, face_i) calls do to the session - the conditioning windows, the faces
        window, h / c, the frame counter, `steps` += n - so step(), observe(), step_rows() and observe_many() alternate freely and
        save_rows / load_rows / reset_rows work as before. frames: {modality: (B, n, dim)} contiguous float32 on the session's
        device, frames t .. t + n - 1 of every modality with history > 0 (extra keys are ignored); faces: (B, n, C) likewise, the
        observed p1_face frames; n >= 1, the same in every tensor. -> nll (n, B) float32, every frame's NLL in bits as observe()
        reports it, or (nll, z) with return_z, z (n, B, C) the latents: frame-major, as forward() and inference(return_nll=True).

        Per call: lfi_stream_chunk_in (the windows as sequences, the chunk behind them; the new values pass the range guard), the
        static part in sequence mode for all n frames, lfi_flow_score_seq_chunk - the conditioning front end ONCE for n B windows and
        ONE chain launch that loops over the frames inside (n + Ks - 1 cell times end to end where n observe() calls take n Ks) -
        and lfi_stream_chunk_out. A chunk beyond the frames one launch takes (_chunk_cap) runs as several such rounds. Eager
        launches, amortised over the chunk: no graph is captured, `replays` does not count them, and the graphs of the per-frame calls
        stay valid (they address the same session buffers). Shapes outside the register-resident cells, LFI_SAMPLE_CHAIN=0 and
        LFI_FLOW_GENERIC=1: lfi_flow_score_seq_from with nframes = n, the per-frame kernels. Everything is checked before the first
        launch: a refused call leaves the session as it was.

        lengths (a ragged chunk: conversations that join with histories of different lengths, clips of different lengths to score):
        None, or a sequence of B ints / a 1-D CPU integer tensor of B entries with 0 <= lengths[r] <= n - host data, as reset_rows'
        rows. Row r takes its first lengths[r] frames and is left exactly where a dense observe_many of those lengths[r] frames
        leaves it: windows, h / c and the frame counter (+= 2 lengths[r]), bit for bit; a row of length 0 is not written at all, so
        joiners warm up in place while the other rows stay where they are. nll[i, r] and z[i, r] for i < lengths[r] are the dense
        call's; behind a row's length both are exact zeros (nll.sum(0) is each clip's total). What frames / faces hold behind a
        row's length is never read - anything, NaN included, and it does not reach the range guard. `steps` += n whatever the
        lengths (injected masks: mask frame steps + i belongs to chunk frame i in every row). Into a session that has not stepped
        yet, h / c are zeroed first and the call runs as a continuing one, as load_rows does. Launches: lfi_stream_chunk_in_rows,
        the static part and the front end dense over n B windows, lfi_flow_score_seq_chunk_rows - a 16-row tile loops to its
        longest row, a tile of length 0 leaves at once: keep rows of similar length in one tile where possible -
        lfi_stream_chunk_out_rows; a round in which every row has length 0 is skipped. Where the dense call falls back to the
        per-frame kernels this one does too, in segments between the distinct lengths."""
        s = self.eng.spec
        self._check_usable()
        if not isinstance(return_z, bool):
            raise TypeError("return_z: expected a bool, got %s %r" % (type(return_z).__name__, return_z))
        srcs, n, lens = self._check_frames(frames, faces, lengths)
        srcs.append(faces)
        with self._chunk_call(n, srcs) as rounds:
            new = torch.empty if lens is None else torch.zeros     # (a ragged chunk's launches write live entries only)
            nll = new(n, self.B, dtype=torch.float32, device=self.device)
            z = new(n, self.B, s.C, dtype=torch.float32, device=self.device) if return_z else None
            if lens is not None:
                self._zero_state_if_fresh()     # (as load_rows; rows of length 0 keep the zeroed state)
            for o, m, mk in rounds:
                rl = None if lens is None else [min(max(v - o, 0), m) for v in lens]
                if rl is not None and not any(rl):
                    self.steps += m             # (nothing to run in this round)
                    continue
                chain = functools.partial(self._forward_chain, nll=nll[o:o + m], z=None if z is None else z[o:o + m])
                self._round([x[:, o:o + m] for x in srcs], m, mk, chain, lens=rl)
        self._record_out(nll, z)
        return (nll, z) if return_z else nll

    @translate_oom
    def step_many(self, frames, noise=None):
        """n generated frames in one call, for conditioning known ahead (a look-ahead buffer over synthesised speech, a rollout under
        hypothesised conditioning, finishing a clip): exactly what n successive step(frame_i, noise_i) calls do to the session - the
        conditioning windows, the faces window, h / c, the frame counter, `steps` += n - so all five kinds of call alternate freely
        and save_rows / load_rows / reset_rows work as before. frames: {modality: (B, n, dim)} contiguous float32 on the session's
        device, frames t .. t + n - 1 of every modality with history > 0 (extra keys are ignored), n >= 1 the same in every tensor;
        noise: (n, B, C) contiguous float32 on the session's device, the prior draws already * eps, frame-major as inference()'s
        noise and observe_many()'s z, or None: n draws of the session's own, stacked - the random numbers n step() calls consume.
        -> out (B, n, C), the generated p1_face frames as inference() returns them; a session opened with return_nll=True ->
        (out, nll), nll (n, B) float32, every frame's NLL in bits as step() reports it.

        Per call: lfi_stream_chunk_gen_in (the windows as sequences, the conditioning behind them; the new values and the noise pass
        the range guard, the noise is read where the caller keeps it), the static part in sequence mode ONCE for all n frames - n
        step() calls run the window encoders n times over windows that overlap in all but one frame - then lfi_flow_sample_seq_nll
        with nframes = n on the faces sequence from the session's live h / c, and lfi_stream_chunk_gen_out (the windows back, the
        generated frames into `out` and through the range guard). Rounds, eager launches and graphs as observe_many()'s. The
        sampler entry point picks its kernels as it does for inference(): every shape and switch it handles works here. Train mode
        without injected masks: the masks of the n frames are drawn in one call, before the noise. Everything is checked before the
        first launch: a refused call leaves the session as it was."""
        s = self.eng.spec
        self._check_usable()
        srcs, n, _ = self._check_frames(frames)
        if noise is None and n is None:
            raise ValueError("noise: a model without conditioning windows takes its frame count from the noise, (n, B=%d, %d)"
                             % (self.B, s.C))
        if noise is not None:
            n = self._check_noise_many(noise, n)
        used = list(srcs)
        srcs.append(None)                       # (the faces window has no source: the chain writes its frames)
        with self._chunk_call(n, used) as rounds:
            if noise is None:
                noise = self._draw_noise(n, "step_many")
            else:
                self._rng_advance("step_many", n)
            used.append(noise)
            out = torch.empty(self.B, n, s.C, dtype=torch.float32, device=self.device)
            nll = torch.empty(n, self.B, dtype=torch.float32, device=self.device) if self.return_nll else None
            for o, m, mk in rounds:
                chain = functools.partial(self._reverse_chain, nll=None if nll is None else nll[o:o + m])
                self._round([x if x is None else x[:, o:o + m] for x in srcs], m, mk, chain, noise=noise[o:o + m], out=out, o=o)
        self._record_out(out, nll)
        return (out, nll) if self.return_nll else out

    def _check_observed_many(self, observed, n):
        """The role mask of step_rows_many(), checked before any launch: host data, an (n, B) CPU torch.bool tensor or a sequence of n
        sequences of B bools, frame-major -> an (n, B) CPU bool tensor."""
        B = self.B
        kind = "observed: expected an (n, B) CPU torch.bool tensor or a sequence of n sequences of B bools, frame-major, got %s"
        if torch.is_tensor(observed):
            if observed.is_cuda:
                raise ValueError("observed: on %s - step_rows_many() takes its role mask as host data (it plans the chunk's launches "
                                 "from it), as observe_many() takes lengths; step_rows() is the call for device-resident masks"
                                 % observed.device)
            if observed.dtype != torch.bool:
                raise TypeError(kind % ("a %s tensor" % observed.dtype))
            if observed.device.type != "cpu":
                raise ValueError("observed: on %s, expected host data" % observed.device)
            if tuple(observed.shape) != (n, B):
                raise ValueError("observed: expected (n, B) = (%d, %d), frame-major, got %s" % (n, B, tuple(observed.shape)))
            return observed.contiguous()
        try:
            rows = [list(r) for r in observed]
        except TypeError:
            raise TypeError(kind % type(observed).__name__) from None
        if len(rows) != n or any(len(r) != B for r in rows):
            raise ValueError("observed: expected (n, B) = (%d, %d), frame-major, got rows of %s entries"
                             % (n, B, [len(r) for r in rows]))
        if any(not isinstance(v, bool) for r in rows for v in r):
            raise TypeError(kind % repr(observed))
        return torch.tensor(rows, dtype=torch.bool).view(n, B)

    @staticmethod
    def _rows_many_min_run():
        """The shortest run of all-observe frames step_rows_many() gives to the chunk forward chain: 2, the smallest run for which n +
        Ks - 1 cell times and one front end beat n Ks and n; LFI_ROWS_MANY_OBSERVE_RUN overrides, 0 never uses the chunk chain."""
        env = os.environ.get("LFI_ROWS_MANY_OBSERVE_RUN")
        if not env:
            return 2
        run = int(env)
        if run < 0:
            raise ValueError("LFI_ROWS_MANY_OBSERVE_RUN: %r is not a frame count" % env)
        return run

    @translate_oom
    def step_rows_many(self, frames, faces, observed, noise=None):
        """n frames in one call in which every row takes its own role FRAME BY FRAME, for frames known ahead (a look-ahead buffer over
        a batch in which some conversations speak while others listen; prompt then continue: each row observes its own recorded
        history, of its own length, and generates the rest): exactly what n successive step_rows(frame_i, face_i, observed[i],
        noise_i) calls do to the session - the conditioning windows, the faces window, h / c, the frame counter (+= 2 n), `steps`
        += n - so all six kinds of call alternate freely and save_rows / load_rows / reset_rows work as before. frames: as
        step_many()'s, {modality: (B, n, dim)}; faces: as observe_many()'s, (B, n, C), read only where a row observes; noise: as
        step_many()'s, (n, B, C) or None (n draws of the session's own, stacked, whatever the mask says - as step_rows draws on
        every call), read only where a row generates; observed: HOST data, as lengths and rows are - an (n, B) CPU torch.bool tensor
        or a sequence of n sequences of B bools, frame-major like nll, True = the row observes that frame (a CUDA tensor is
        refused: step_rows() takes device-resident masks). The prompt-then-continue mask of per-row prompt lengths is
            observed = torch.arange(n)[:, None] < lengths[None, :]
        -> (out, nll), always both whatever return_nll the session was opened with, as step_rows: out (B, n, C) the frame that
        entered each row's faces window, given (a copy of `faces` there) or generated; nll (n, B) every frame's NLL in bits. `faces`
        at generating slots and `noise` at observing slots are never read into anything stored and do not reach the range guard:
        anything, NaN included.

        Per round of at most _chunk_cap() frames: the role words to a session-owned buffer (pinned host memory, asynchronously),
        lfi_stream_chunk_roles_in (the windows as sequences; given frames enter the faces sequence where their row observes), the
        static part in sequence mode ONCE for the round, then the round's plan (plan_rows_many; kept, rounds concatenated and with
        offsets in the call, in `last_plan` - a diagnostic): maximal runs of at least 2 frames that EVERY row observes go to
        lfi_flow_score_seq_chunk (LFI_ROWS_MANY_OBSERVE_RUN overrides the 2, 0 = never; never where that chain does not run),
        everything else - all-generate runs included: step_many() is for callers who know that nobody observes - to
        lfi_flow_step_rows_seq, the rows chain frame by frame; then lfi_stream_chunk_gen_out. Eager launches and graphs as
        observe_many()'s. With a fixed plan a row's values do not
        depend on the other rows' roles or inputs (rows never mix in a cell, and the dense static part runs the same shapes);
        across plans, and against the per-frame calls, values agree to the session's gates, not bit for bit (the batched front end
        and the sequence-mode static part sum in another order, as for step_many / observe_many). Everything is checked before the
        first launch: a refused call leaves the session as it was."""
        s = self.eng.spec
        self._check_usable()
        srcs, n, _ = self._check_frames(frames, faces)
        if noise is not None:
            self._check_noise_many(noise, n)
        roles = self._check_observed_many(observed, n)
        srcs.append(faces)
        min_run = self._rows_many_min_run()
        used = list(srcs)
        with self._chunk_call(n, used) as rounds:
            if noise is None:
                noise = self._draw_noise(n, "step_rows_many")
            else:
                self._rng_advance("step_rows_many", n)
            used.append(noise)
            out = torch.empty(self.B, n, s.C, dtype=torch.float32, device=self.device)
            nll = torch.empty(n, self.B, dtype=torch.float32, device=self.device)
            plan = []
            for o, m, mk in rounds:
                chain = functools.partial(self._planned_chain, nll=nll[o:o + m], min_run=min_run)
                plan += [(kind, o + f0, cnt) for kind, f0, cnt in
                         self._round([x[:, o:o + m] for x in srcs], m, mk, chain, noise=noise[o:o + m], roles=roles[o:o + m],
                                     out=out, o=o)]
            self.last_plan = plan
        self._record_out(out, nll)
        return out, nll

    @contextlib.contextmanager
    def _chunk_call(self, n, used):
        """The driver of a chunk call of n frames, once its arguments are checked: the session's engine state (_owned), the range guard
        of earlier calls and the mask draw - before anything the body draws; then the body, with the chunk's workspaces as the
        engine's (the session's own keep the addresses its graphs hold); behind it the guard's copy and record_stream of `used`, the
        caller's tensors the launches read (the body may add to the list). Yields the rounds, at most _chunk_cap() frames each:
        [(first frame, frames, the round's masks or None), ...]. A body that raises leaves the workspaces as they were."""
        cap = self._chunk_cap()
        with self._owned():
            self._check_guard()
            eng = self.eng
            masks = self._chunk_masks(n)
            keep, eng._ws = eng._ws, self._chunk_ws
            try:
                yield [(o, min(cap, n - o), None if masks is None else {k: v[o:o + cap].contiguous() for k, v in masks.items()})
                       for o in range(0, n, cap)]
            finally:
                self._chunk_ws, eng._ws = eng._ws, keep
            self._publish_guard()
            for x in used:
                x.record_stream(torch.cuda.current_stream(self.device))

    def _draw_noise(self, n, kind):
        """n prior draws of the session's own, stacked (n, B, C): the random numbers n one-frame calls consume. A keyed session: one
        launch into the chunk's own buffer, the positions move by the call's n in it."""
        if self.rng is not None:
            f = n * self.B * self.eng.spec.C
            return self._draw(kind, self.eng._buf("chunk_noise_draw", f)[:f].view(n, self.B, self.eng.spec.C), n=n)
        return torch.stack([self._noise_fn(self.B, self.eng.spec.C) for _ in range(n)]).contiguous()

    def _round(self, srcs, m, masks, chain, lens=None, noise=None, roles=None, out=None, o=0):
        """m frames of a chunk call, inside _chunk_call(): windows in, static part, chain, windows out, `steps` += m. srcs: the
        round's frames of self._wins' windows in their order (strided views of the caller's tensors; None for a window without a
        source). The options say what the call is and pick the window launches. lens (a ragged observe_many round): the B rows'
        frame counts, each in [0, m] and not all 0 - the _rows pair. noise (step_many, step_rows_many): (m, B, C), a contiguous
        slice of the call's - the faces window is the generated one (gen_in / gen_out), and its m frames go to out[:, o:o + m].
        roles (step_rows_many): (m, B) CPU bool - roles_in. chain(r) launches the middle from the session's live state, given the
        round r: dims, p, pre, faces (the faces sequence), m, noise, lens, roles and words, the round's lengths or role words on the
        device. -> what chain returns."""
        s, eng, B = self.eng.spec, self.eng, self.B
        k = len(self._wins)
        gen = k - 1                             # the prev_p1_face window: the last of self._wins
        seqs, seq_p, src_p = self._chunk_seqs(srcs, m)
        head, tabs = (B, m, s.start, k, self._row_win), (self._row_hist, self._row_dim, self._lead)
        ev = eng._tic("stream_chunk_in")
        words = None
        if lens is not None or roles is not None:
            # pinned host memory of their own (the copy is asynchronous), one session-owned device buffer
            host = torch.tensor(lens, dtype=torch.int32) if roles is None else roles.to(torch.int32).reshape(-1)
            words = eng._buf_i32("chunk_lengths" if roles is None else "chunk_roles", host.numel())
            words[:host.numel()].copy_(host.pin_memory(), non_blocking=True)
        if noise is None:
            name = "lfi_stream_chunk_in" if lens is None else "lfi_stream_chunk_in_rows"
            more = (self.guard.data_ptr(),) + (() if lens is None else (words.data_ptr(),))
        else:
            name = "lfi_stream_chunk_gen_in" if roles is None else "lfi_stream_chunk_roles_in"
            more = (gen, noise.data_ptr(), s.C) + (() if roles is None else (words.data_ptr(),)) + (self.guard.data_ptr(),)
        check(getattr(eng.L, name)(*head, src_p, seq_p, *tabs, *more, _stream()), name)
        eng._toc("stream_chunk_in", ev)
        pre = self._chunk_static(seqs, m, masks)
        dims, p = eng._flow_dims(B, m), eng._flow_params()
        dims.gemm_precision = self.frame_precision
        done = chain(types.SimpleNamespace(dims=dims, p=p, pre=pre, faces=seqs["p1_face"], m=m, noise=noise, lens=lens, roles=roles,
                                           words=words))
        if noise is None:
            name = "lfi_stream_chunk_out" if lens is None else "lfi_stream_chunk_out_rows"
            more = (ptr(self.frame_nb),) + (() if lens is None else (words.data_ptr(),))
        else:
            name = "lfi_stream_chunk_gen_out"
            more = (gen, out.data_ptr() + 4 * o * s.C, out.shape[1] * s.C, ptr(self.frame_nb), self.guard.data_ptr())
        check(getattr(eng.L, name)(*head, seq_p, *tabs, *more, _stream()), name)
        if noise is None:                       # (an observe_many round: frames taken without a draw)
            self._rng_advance("observe_many", m, lens, words)
        self.steps += m
        return done

    def _chain_args(self, r, f0=0, cnt=None, noise=False):
        """What every sequence chain's argument list starts with, for frames f0 .. f0 + cnt - 1 (default: to the end) of round r, from
        the session's live h / c: only the round's first frame can be the session's first. noise: the chain takes the prior draws."""
        s, eng, B = self.eng.spec, self.eng, self.B
        args = (C.byref(r.dims), C.byref(r.p), eng.prep.data_ptr(), eng.wct_f.data_ptr(), s.ldf, self.hist1,
                r.pre.data_ptr() + 4 * f0 * B * s.Ks * s.D)
        if noise:
            args += (r.noise.data_ptr() + 4 * f0 * B * s.C,)
        return args + (r.faces.data_ptr(), s.start + r.m, s.start + f0, r.m - f0 if cnt is None else cnt,
                       self._first_frame if f0 == 0 else 1, self.h.data_ptr(), ptr(self.cs), C.byref(self._p1))

    def _chunk_work(self, dims):
        eng = self.eng
        return eng._buf("chunk_work", eng.L.lfi_flow_score_chunk_work_floats(C.byref(dims), C.byref(self._p1), self.hist1))

    def _gen_work(self, dims, nll=True):
        """The work areas of the chains that generate (reverse, rows) -> (work, p1work, nll_work or None)."""
        eng, L = self.eng, self.eng.L
        return (eng._buf("chunk_gen_work", L.lfi_flow_sample_work_floats(C.byref(dims))),
                eng._buf("chunk_gen_p1work", L.lfi_flow_sample_p1_work_floats(C.byref(dims), C.byref(self._p1), self.hist1)),
                eng._buf("chunk_gen_nll_work", L.lfi_flow_sample_nll_work_floats(C.byref(dims))) if nll else None)

    def _forward_chain(self, r, nll, z):
        """observe_many's chain: the chunk forward chain (its _rows form for a ragged round), or the per-frame kernels on the same
        sequences where it does not run. nll (m, B) / z (m, B, C) or None: contiguous slices of the call's outputs, zeroed by the
        caller for a ragged round."""
        s, eng, L, B = self.eng.spec, self.eng, self.eng.L, self.B
        ev = eng._tic("stream_chunk_chain")
        if self.hist1 >= 1 and L.lfi_flow_score_chunk_ok(C.byref(r.dims)):     # (the chunk chain wants a faces window)
            outs = (None, None, self._chunk_work(r.dims).data_ptr(), ptr(z), nll.data_ptr())
            if r.lens is not None:
                check(L.lfi_flow_score_seq_chunk_rows(*self._chain_args(r), *outs, r.words.data_ptr(), _stream()),
                      "lfi_flow_score_seq_chunk_rows")
            else:
                check(L.lfi_flow_score_seq_chunk(*self._chain_args(r), *outs, _stream()), "lfi_flow_score_seq_chunk")
        else:
            # m front ends and m chains (or Ks cells each), one frame's work areas
            work = eng._buf("chunk_frame_work", L.lfi_flow_sample_work_floats(C.byref(r.dims)))
            p1work = eng._buf("chunk_frame_p1work", L.lfi_flow_sample_p1_work_floats(C.byref(r.dims), C.byref(self._p1), self.hist1))
            score = eng._buf("chunk_frame_score", L.lfi_flow_score_work_floats(C.byref(r.dims)))

            def run(f0, cnt):                   # frames f0 .. f0 + cnt - 1 of the round, every row
                check(L.lfi_flow_score_seq_from(*self._chain_args(r, f0, cnt), p1work.data_ptr(), work.data_ptr(), score.data_ptr(),
                                                None if z is None else z.data_ptr() + 4 * f0 * B * s.C, nll.data_ptr() + 4 * f0 * B,
                                                _stream()), "lfi_flow_score_seq_from")
            if r.lens is None:
                run(0, r.m)
            else:
                self._ragged_frames(run, r.lens, r.m, nll, z)
        eng._toc("stream_chunk_chain", ev)

    def _reverse_chain(self, r, nll):
        """step_many's chain: the sampler's, which writes the round's frames into the faces sequence. nll (m, B) or None."""
        eng = self.eng
        work, p1work, nll_work = self._gen_work(r.dims, nll is not None)
        ev = eng._tic("stream_chunk_gen_chain")
        check(eng.L.lfi_flow_sample_seq_nll(*self._chain_args(r, noise=True), p1work.data_ptr(), work.data_ptr(), ptr(nll), ptr(nll_work),
                                            _stream()), "lfi_flow_sample_seq_nll")
        eng._toc("stream_chunk_gen_chain", ev)

    def _planned_chain(self, r, nll, min_run):
        """step_rows_many's mix: the runs of the round's plan, chunk forward chain or rows chain, in frame order on the same
        sequences and the same pre. -> the plan [(kind, first, count), ...], offsets in the round."""
        eng, L, B = self.eng, self.eng.L, self.B
        # chunk-chain runs only where that chain runs (it wants a faces window and the register-resident cells)
        chunk_ok = self.hist1 >= 1 and bool(L.lfi_flow_score_chunk_ok(C.byref(r.dims)))
        plan = plan_rows_many(r.roles.all(1).tolist(), min_run if chunk_ok else 0)
        ev = eng._tic("stream_chunk_rows_chain")
        for kind, f0, cnt in plan:
            at = nll.data_ptr() + 4 * f0 * B
            if kind == "observe":
                check(L.lfi_flow_score_seq_chunk(*self._chain_args(r, f0, cnt), None, None, self._chunk_work(r.dims).data_ptr(), None, at,
                                                 _stream()), "lfi_flow_score_seq_chunk")
                continue
            work, p1work, nll_work = self._gen_work(r.dims)
            rows_work = eng._buf("chunk_rows_work", L.lfi_flow_step_rows_work_floats(C.byref(r.dims)))
            check(L.lfi_flow_step_rows_seq(*self._chain_args(r, f0, cnt, noise=True), p1work.data_ptr(), work.data_ptr(), at,
                                           nll_work.data_ptr(), r.words.data_ptr() + 4 * f0 * B, rows_work.data_ptr(), _stream()),
                  "lfi_flow_step_rows_seq")
        eng._toc("stream_chunk_rows_chain", ev)
        return plan

    def _drawn_masks(self, n):
        """Injected masks (masks_fn, tests only) for frames steps .. steps + n - 1, validated -> {name: (n, B, hist)}, views of what
        was drawn, or None without any; a one-frame mask repeats."""
        drawn = self._masks_fn(self.B, n) if self._masks_fn is not None else None
        self.eng.precision = self.precision      # (the module's mask draw re-applies its own mode to the engine)
        if not drawn:
            return None
        masks = {}
        for name, buf in self.mask_bufs.items():
            m = drawn.get(name)
            if m is None:
                continue
            if m.dim() != 3 or tuple(m.shape[1:]) != (self.B, buf.shape[2]):
                raise ValueError("mask for %s must be (N, B, hist) = (., %d, %d), got %s" % (name, self.B, buf.shape[2], tuple(m.shape)))
            if m.shape[0] != 1 and self.steps + n > m.shape[0]:
                raise ValueError("mask for %s holds %d frames; this is frame %d of the stream" % (name, m.shape[0], self.steps + n - 1))
            masks[name] = m.expand(n, -1, -1) if m.shape[0] == 1 else m[self.steps:self.steps + n]
        return masks

    def _chunk_masks(self, n):
        """The injected masks of a chunk's n frames on the session's device, or None."""
        drawn = self._drawn_masks(n)
        if not drawn:
            return None
        return {name: m.to(device=self.device, dtype=torch.float32).contiguous() for name, m in drawn.items()}

    def _chunk_seqs(self, srcs, m):
        """The sequence buffers of a round of m frames (B x (start + m) x dim per window of self._wins, in the chunk's workspaces) and
        the pointer tables the window launches take. srcs: the round's frames per window, in self._wins' order, None where a window
        has no source (step_many's faces); a strided view is made contiguous in place in the list, which keeps it alive until the
        launches that read it are queued. -> (seqs by name, seq_p, src_p)."""
        s, eng, B = self.eng.spec, self.eng, self.B
        T = s.start + m
        k = len(self._wins)
        seq_p, src_p = (C.c_void_p * k)(), (C.c_void_p * k)()
        seqs = {}
        for i, ((name, _, _, d, _), x) in enumerate(zip(self._wins, srcs)):
            if x is not None:
                x = x if x.is_contiguous() else x.contiguous()
                srcs[i] = x
            seqs[name] = eng._buf("chunk_seq." + name, B * T * d)[:B * T * d].view(B, T, d)
            seq_p[i], src_p[i] = seqs[name].data_ptr(), None if x is None else x.data_ptr()
        return seqs, seq_p, src_p

    def _chunk_static(self, seqs, m, masks):
        """The static part as _sample's static() makes it for a run of m frames, from the session's sequences and its per-row
        counter -> pre (m * B rows of Ks * D), what the chains consume."""
        s, eng, B = self.eng.spec, self.eng, self.B
        ev = eng._tic("stream_chunk_static")
        cond = eng._buf("chunk_cond", m * B * s.ldf)
        pre = eng._buf("chunk_pre", m * B * s.Ks * s.D)
        data = {name: t for name, t in seqs.items() if name != "p1_face"}
        if self.frame_nb is not None:
            data["frame_nb"] = self.frame_nb
        eng.build_features(data, None, B, s.start + m, masks, cond, with_stash=False, skip_p1=True, sampling=False, frame_nb_offset=2.0)
        eng._static_pre(cond, pre, m * B, self.c1, self._wp)
        eng._toc("stream_chunk_static", ev)
        return pre

    def _ragged_frames(self, run, lens, m, nll, z):
        """A ragged round on the per-frame kernels, which know no lengths: the frames in segments between the sorted distinct
        lengths, every row in every segment (a row behind its length runs on the zeros lfi_stream_chunk_in_rows left in the
        sequences). After a segment the h / c rows of the rows that end there are put aside; at the end they go back, with the
        rows of length 0 as they were before the round, and the outputs behind each length are zeroed."""
        s, B = self.eng.spec, self.B
        states = [t[:s.Ks * B * s.H].view(s.Ks, B, s.H) for t in (self.h, self.cs) if t is not None]
        rows_at = collections.defaultdict(list)
        for r, v in enumerate(lens):
            rows_at[v].append(r)
        index = {v: torch.tensor(rows, dtype=torch.long, device=self.device) for v, rows in rows_at.items()}
        kept = [(index[0], [t.index_select(1, index[0]) for t in states])] if 0 in index else []
        done = 0
        for cut in sorted(v for v in index if v > 0):
            run(done, cut - done)
            if cut < max(lens):                 # (the longest rows' state is where it belongs already)
                kept.append((index[cut], [t.index_select(1, index[cut]) for t in states]))
            done = cut
        for idx, saved in kept:
            for t, v in zip(states, saved):
                t.index_copy_(1, idx, v)
        behind = torch.arange(m).unsqueeze(1) >= torch.tensor(lens).unsqueeze(0)     # (m, B), built on the host
        behind = behind.to(self.device)
        nll.masked_fill_(behind, 0.0)
        if z is not None:
            z.masked_fill_(behind.unsqueeze(2), 0.0)

    def _check_observed(self, observed):
        """The role mask of step_rows(), checked before any launch -> a (B,) bool tensor, on the session's device or on the host (a
        host mask is copied in on the step's stream)."""
        B = self.B
        if torch.is_tensor(observed):
            if observed.dtype != torch.bool:
                raise TypeError("observed: expected a torch.bool tensor or a sequence of bools, got a %s tensor" % observed.dtype)
            if observed.dim() != 1 or observed.shape[0] != B:
                raise ValueError("observed: expected %d entries (B,), got %s" % (B, tuple(observed.shape)))
            if observed.is_cuda and observed.device != self.device:
                raise ValueError("observed: on %s, the session on %s" % (observed.device, self.device))
            if not observed.is_cuda and observed.device.type != "cpu":
                raise ValueError("observed: on %s, the session on %s" % (observed.device, self.device))
            return observed.contiguous()
        try:
            flags = list(observed)
        except TypeError:
            raise TypeError("observed: expected a torch.bool tensor or a sequence of bools, got %s" % type(observed).__name__) from None
        if any(not isinstance(v, bool) for v in flags):
            raise TypeError("observed: expected a torch.bool tensor or a sequence of bools, got %r" % (observed,))
        if len(flags) != B:
            raise ValueError("observed: expected %d entries (B,), got %d" % (B, len(flags)))
        return torch.tensor(flags, dtype=torch.bool)

    @translate_oom
    def step_rows(self, frame, face, observed, noise=None):
        """One frame in which every row either observes or generates: row r takes face[r] as its p1_face frame t where observed[r]
        is true (observe()'s step for that row) and generates it from noise[r] otherwise (step()'s). frame: as step()'s; face: (B, C)
        float32 GPU tensor, read only in observing rows (anything, NaN included, elsewhere; not in the range guard there); observed:
        (B,) torch.bool on the session's device - no host wait, and a mask that changes every call recaptures nothing: the roles are
        data at a session-owned address - or a host sequence / CPU tensor of B bools, copied in asynchronously; noise: as step()'s
        (None: B x C values are drawn on every call, whatever the mask), unused in observing rows. -> (out, nll): out (B, C) the frame
        that entered each row's faces window, generated or given; nll (B,) float32 its NLL in bits, as step(return_nll=True) and
        observe() report it - both always, whatever return_nll the session was opened with. Each row moves on exactly as the pure
        call of its role moves it (bit for bit), so step(), observe() and step_rows() alternate freely.

        Per call: lfi_stream_advance_rows (the face enters the faces window in observing rows only; the mask becomes the session's
        role words), the static part, then lfi_flow_step_rows_from: the conditioning front end once and BOTH chains in one launch
        with row-masked stores. A 16-row tile whose rows share a role costs one chain, a mixed tile both: keep speaking and
        listening conversations in separate tiles where possible. From the second call on, one captured hipGraph of its own, keyed
        as the others are."""
        s = self.eng.spec
        self._check_usable()
        srcs = self._check_frame(frame)
        observed = self._check_observed(observed)
        self._check_matrix(face, "face", s.C, self.B)
        if noise is not None:
            self._check_matrix(noise, "noise", s.C, self.B)
        with self._owned():
            self._check_guard()
            if self.role is None:        # the step_rows buffers: at the first step_rows, outside capture
                eng, dims = self.eng, self.eng._flow_dims(self.B, 1)
                self.rows_work = eng._buf("stream_rows_work", eng.L.lfi_flow_step_rows_work_floats(C.byref(dims)))
                self.rows_nll = eng._buf("stream_rows_nll", self.B)[:self.B]
                self.rows_nll_work = eng._buf("stream_rows_nll_work", eng.L.lfi_flow_sample_nll_work_floats(C.byref(dims)))
                self.role = eng._buf_i32("stream_role", self.B)
            if noise is None:
                noise = self._noise_fn(self.B, s.C).contiguous() if self.rng is None else self._draw("step_rows", self.draw)
            else:
                self._rng_advance("step_rows")
            if not observed.is_cuda:
                observed = observed.pin_memory().to(self.device, non_blocking=True)
            self._advance(srcs, noise, face, observed=observed)
            out = self.faces[:, self.hist1].clone()
            nll = self.rows_nll.clone()
            self.steps += 1
        self._record_out(out, nll)
        return out, nll

    def _record_out(self, *outs):
        if self._stream is not None:
            for x in outs:
                if x is not None and x.device == self.device:
                    x.record_stream(torch.cuda.current_stream(self.device))

    def _advance(self, srcs, noise, face, want_z=False, observed=None, ncand=None):
        """One frame forward, inside _owned(): masks, lfi_stream_advance, the guard's copy, then the launch or the replay. face None: a
        generating step with the prior draw `noise`; else an observing one - the frame is the faces window's source (and fills the
        noise slot, which an observing step does not read); want_z: the observing launch also writes the frame's latent. observed (a
        (B,) bool tensor on the device): a step_rows() step - both `noise` and `face`, each used in the rows of its role. ncand: a
        step_candidates() step - `noise` is (B, ncand, C) and moves into that ncand's own buffer, a row of ncand * C values."""
        s, eng, B = self.eng.spec, self.eng, self.B
        rows = observed is not None
        observe = face is not None and not rows
        masks = self._drawn_masks(1)
        if masks is not None:
            masks = {name: self.mask_bufs[name].copy_(m) for name, m in masks.items()}
        for i, x in enumerate(srcs):
            self._src_p[i] = x.data_ptr()
        self._src_p[len(srcs)] = face.data_ptr() if observe or rows else None
        moved = face if observe else noise
        ev = eng._tic("stream_advance")
        if rows:
            check(eng.L.lfi_stream_advance_rows(B, len(self._row_win), self._row_win, self._src_p, self._row_hist, self._row_dim,
                                                len(srcs), noise.data_ptr(), self.noise.data_ptr(), s.C, ptr(self.frame_nb),
                                                observed.data_ptr(), self.role.data_ptr(), self.guard.data_ptr(), _stream()),
                  "lfi_stream_advance_rows")
        else:
            slot, width = (self.noise, s.C) if ncand is None else (self._cand[ncand].noise, ncand * s.C)
            check(eng.L.lfi_stream_advance(B, len(self._row_win), self._row_win, self._src_p, self._row_hist, self._row_dim,
                                           moved.data_ptr(), slot.data_ptr(), width, ptr(self.frame_nb), self.guard.data_ptr(),
                                           _stream()), "lfi_stream_advance")
        eng._toc("stream_advance", ev)
        self._publish_guard()
        for x in srcs + ([noise, face, observed] if rows else [moved]):
            x.record_stream(torch.cuda.current_stream(self.device))
        launch = self._launch_rows if rows else functools.partial(self._launch_observe, want_z) if observe else self._launch
        if ncand is not None:
            launch = functools.partial(self._launch_cand, ncand)
        if self.steps == 0 or os.environ.get("LFI_NO_GRAPH") == "1":
            launch(masks, self._first_frame)
            return
        # a captured graph per kind of step, keyed on what its launches depend on. step(): one graph, recaptured when the key changes.
        # observe(): one per key met (with and without z, per arithmetic) - alternating kinds or return_z recaptures nothing
        # step_rows(): one per key met; the role mask is data at a session-owned address (self.role), not part of the key
        # step_candidates(): one per key met, ncand among it (the launch's grid and the buffers it addresses)
        key = (self.frame_precision, masks is not None) + ((want_z,) if observe else ()) + ((ncand,) if ncand is not None else ())
        own = self._rows_graphs if rows else self._observe_graphs if observe else self._cand_graphs if ncand is not None else None
        g = own.get(key) if own is not None else (self._graph if self._graph_key == key else None)
        if g is None:
            timers, eng.timers = eng.timers, None
            try:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    launch(masks, 1)
            finally:
                eng.timers = timers
            if own is not None:
                own[key] = g
            else:
                self._graph, self._graph_key = g, key
        ev = eng._tic("stream_graph")
        g.replay()
        eng._toc("stream_graph", ev)
        self.replays += 1

    def _static(self, masks):
        """The static part for the session's B windows (window encoders + the static cond_transform columns): session-owned memory."""
        eng, B = self.eng, self.B
        ev = eng._tic("stream_static")
        data = dict(self.windows)
        if self.frame_nb is not None:
            data["frame_nb"] = self.frame_nb
        # (sampling=False: the frame counter comes from the session's device counter, not from a host frame offset)
        eng.build_features(data, None, B, 0, masks, self.cond, with_stash=False, skip_p1=True, sampling=False, windows=True)
        eng._static_pre(self.cond, self.pre, B, self.c1, self._wp)
        eng._toc("stream_static", ev)
        dims = eng._flow_dims(B, 1)
        dims.gemm_precision = self.frame_precision
        return dims, eng._flow_params()

    def _frame_args(self, dims, p, first_frame, noise=None):
        """What every per-frame chain's argument list starts with (_chain_args' counterpart for the session's own one-frame buffers):
        the frame at slot hist1 of the hist1 + 1 frame faces window, from the session's live h / c. noise: the prior draws of a
        chain that generates."""
        s, eng = self.eng.spec, self.eng
        args = (C.byref(dims), C.byref(p), eng.prep.data_ptr(), eng.wct_f.data_ptr(), s.ldf, self.hist1, self.pre.data_ptr())
        if noise is not None:
            args += (noise.data_ptr(),)
        return args + (self.faces.data_ptr(), self.hist1 + 1, self.hist1, 1, first_frame, self.h.data_ptr(), ptr(self.cs),
                       C.byref(self._p1), self.p1work.data_ptr(), self.work.data_ptr())

    def _launch(self, masks, first_frame):
        """The static part, then the reverse chain for one frame: session-owned memory only."""
        eng = self.eng
        args = self._frame_args(*self._static(masks), first_frame, self.noise)
        ev = eng._tic("stream_chain")
        if self.return_nll:
            check(eng.L.lfi_flow_sample_seq_nll(*args, self.nll.data_ptr(), self.nll_work.data_ptr(), _stream()), "lfi_flow_sample_seq_nll")
        else:
            check(eng.L.lfi_flow_sample_seq_from(*args, _stream()), "lfi_flow_sample_seq_from")
        eng._toc("stream_chain", ev)

    def _launch_observe(self, want_z, masks, first_frame):
        """The static part, then the forward chain on the observed frame the faces window holds: session-owned memory only. The latent
        is written only when it is wanted (z = NULL otherwise)."""
        eng = self.eng
        args = self._frame_args(*self._static(masks), first_frame)
        ev = eng._tic("stream_observe_chain")
        check(eng.L.lfi_flow_score_seq_from(*args, self.score_work.data_ptr(), self.obs_z.data_ptr() if want_z else None,
                                            self.obs_nll.data_ptr(), _stream()), "lfi_flow_score_seq_from")
        eng._toc("stream_observe_chain", ev)

    def _launch_rows(self, masks, first_frame):
        """The static part, then both chains in one launch, each on the rows of its role (self.role): session-owned memory only."""
        eng = self.eng
        args = self._frame_args(*self._static(masks), first_frame, self.noise)
        ev = eng._tic("stream_rows_chain")
        check(eng.L.lfi_flow_step_rows_from(*args, self.rows_nll.data_ptr(), self.rows_nll_work.data_ptr(), self.role.data_ptr(),
                                            self.rows_work.data_ptr(), _stream()), "lfi_flow_step_rows_from")
        eng._toc("stream_rows_chain", ev)

    def _launch_cand(self, ncand, masks, first_frame):
        """The static part for B windows, then the front end for B rows and the candidate chain over B * ncand virtual rows: the
        session's faces window and h / c are read only, what the candidates leave goes to that ncand's buffers."""
        eng, cand = self.eng, self._cand[ncand]
        args = self._frame_args(*self._static(masks), first_frame, cand.noise)
        ev = eng._tic("stream_chain")
        check(eng.L.lfi_flow_sample_cand_from(*args, None, None, ncand, cand.frames.data_ptr(), cand.nll.data_ptr(), cand.h.data_ptr(),
                                              ptr(cand.c), cand.work.data_ptr(), _stream()), "lfi_flow_sample_cand_from")
        eng._toc("stream_chain", ev)

    def _publish_guard(self):
        """The guard word's copy to pinned memory behind the launches that folded into it, and the event _check_guard waits on."""
        self._pinned.copy_(self.guard, non_blocking=True)
        gev = torch.cuda.Event()
        gev.record()
        self._guard_pending = gev

    def _check_guard(self):
        """The range guard of earlier steps (lfi_stream_advance folds max |x| of every value it moves into the session's guard word,
        copied to pinned memory behind it): looked at once its copy has landed - never a host wait. A value beyond the fp16 pieces'
        range (or a non-finite one) is reported with a warning, and the session samples with six bf16 products from then on."""
        ev = self._guard_pending
        if ev is None or not ev.query():
            return
        self._guard_pending = None
        amax, limit = self.eng._guard_float(self._pinned), self.eng._fp16_piece_limit
        if self.frame_precision == 9 and not (amax <= limit):
            self.frame_precision = 5
            warnings.warn("SampleStream: an earlier step saw max |x| = %r, beyond the range of the fp16-piece per-frame arithmetic (%g): "
                          "this session samples with six bf16 products (no range caveat) from now on; frames since that input may be "
                          "inaccurate" % (amax, limit), RuntimeWarning)
