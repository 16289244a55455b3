"""GPU: per-row roles over a chunk of frames (SampleStream.step_rows_many -> lfi_stream_chunk_roles_in / the static part once per round
/ the round's plan: lfi_flow_score_seq_chunk for runs every row observes, lfi_flow_step_rows_seq for everything else /
lfi_stream_chunk_gen_out): agreement with the step_rows() loop down to the row records, rows that do not see each other, inputs that
are ignored, the all-generate and all-observe limits, prompt-then-continue against the fp64 oracle on every golden fixture, the state
carried into and out of the other five kinds of call, split rounds, the fallback kernels, and the housekeeping (injected masks, the
session's own noise, rollback, counters, streams, the range guard).

Gates, all the project's own: frames and row records FRAME_GATE = 1e-5 absolute, NLL max_rel(nll, expected, floor=1.0) < NLL_GATE =
1e-4 (tests/test_gpu_stream_observe.py); bit-exactness is torch.equal."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, report
from lets_face_it_amd.stream import plan_rows_many
from sample_nll_expected import fixture_expected
from test_gpu_parity import build
from test_gpu_stream import _frame, _seed
from test_gpu_stream_chunk import _chunk, _takes_the_chunk_chain
from test_gpu_stream_observe import _infer_case
from test_gpu_stream_step_many import CARRY, _guard_value
from test_gpu_stream_step_rows import _case, _final_case, _schedule, _spec_model

pytestmark = pytest.mark.gpu

FRAME_GATE = 1e-5
NLL_GATE = 1e-4
SWITCH = "LFI_ROWS_MANY_OBSERVE_RUN"


def _abs(a, b):
    return (a - b).abs().max().item()


def _mask(B, N, seed, runs=()):
    """_schedule's roles from its frame 2 on - the call's first frame then has a MIXED first tile - with the frames of `runs`
    ((first, count), ...) observed by every row: the runs the plan gives to the chunk chain."""
    obs = _schedule(B, N + 2, seed)[2:].clone()
    for first, count in runs:
        obs[first:first + count] = True
    return obs


def _many(st, data, given, noise, obs, start, first, n):
    """Frames first .. first + n - 1 after the seed in one step_rows_many() call; given (B, N, C), noise (N, B, C), obs (N, B) CPU."""
    return st.step_rows_many(_chunk(data, start, first, n), given[:, first:first + n].contiguous(), obs[first:first + n],
                             noise[first:first + n])


def _loop(st, data, given, noise, obs, start, first, last):
    """The step_rows() loop over frames first .. last - 1 -> (out, nll) as step_rows_many() orients them."""
    got = [st.step_rows(_frame(data, start + n), given[:, n].contiguous(), obs[n], noise[n]) for n in range(first, last)]
    return torch.stack([a for a, _ in got], 1), torch.stack([q for _, q in got])


def _synthetic(name, device, B, N):
    fx = Fixture(name)
    m = _spec_model(build(fx, device), device)
    data, faces, noise = _case(m, device, B, N, fx.start)
    return fx, m, data, faces.transpose(0, 1).contiguous(), noise


def _expected_plan(m, B, obs, min_run=2):
    return plan_rows_many(obs.all(1).tolist(), min_run if _takes_the_chunk_chain(m, B, obs.shape[0]) else 0)


# ---- 1. against the step_rows() loop, down to the row records
@pytest.mark.parametrize("name,n", (("tiny", 2), ("tiny", 9), ("mid", 10), ("tiny_lstm", 6), ("p1enc", 6), ("framenb", 6)))
def test_step_rows_many_agrees_with_the_step_rows_loop_down_to_the_row_records(name, n, gpu_device, monkeypatch):
    """B = 20: two tiles, the second partial; fresh sessions, so the first frame runs with first_frame = 0 in a mixed tile. n below and
    above the history (tiny: 4 frames), a long history (mid), an LSTM's c, an encoded faces window and the frame counter."""
    B = 20
    fx, m, data, given, noise = _synthetic(name, gpu_device, B, n)
    obs = _mask(B, n, 5, ((3, 2),) if n >= 6 else ())
    assert obs[0, :16].any() and not obs[0, :16].all()
    rows = list(range(B))
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as one:
            want, want_nll = _loop(one, data, given, noise, obs, fx.start, 0, n)
            a = one.save_rows(rows)
        for run in (None, "0"):
            with monkeypatch.context() as mp:
                if run is not None:
                    mp.setenv(SWITCH, run)
                with m.open_stream(_seed(data, fx.start)) as many:
                    out, nll = _many(many, data, given, noise, obs, fx.start, 0, n)
                    assert many.steps == n and many.replays == 0
                    assert many.last_plan == (_expected_plan(m, B, obs) if run is None else [("rows", 0, n)])
                    if run is None and n >= 6:
                        assert ("observe", 3, 2) in many.last_plan
                    b = many.save_rows(rows)
                    sig = many.row_signature
            assert tuple(out.shape) == (B, n, given.shape[2]) and out.is_contiguous() and tuple(nll.shape) == (n, B)
            assert out.dtype == nll.dtype == torch.float32
            ncond = sum(h * d for _, h, d in sig[5])
            err, nerr, serr = _abs(out, want), max_rel(nll, want_nll, floor=1.0), _abs(a.data, b.data)
            report("%s (%s), %d frames, step_rows_many (%s) vs %d step_rows() calls: frames max abs diff %.3e, NLL max rel diff %.3e, "
                   "row records max abs diff %.3e" % (name, precision, n, "default plan" if run is None else SWITCH + "=0", n, err, nerr,
                                                      serr))
            assert a.signature == b.signature == sig
            assert err < FRAME_GATE and nerr < NLL_GATE and serr < FRAME_GATE, (precision, run, err, nerr, serr)
            assert torch.equal(a.data[:, :ncond], b.data[:, :ncond])
            if sig[4]:      # the frame counter, the record's last float
                assert torch.equal(a.data[:, -1], b.data[:, -1])
            where = obs.t().to(gpu_device)
            assert torch.equal(out[where], given[where])


# ---- 2. rows do not see each other
@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_rows_do_not_see_each_other(precision, gpu_device, monkeypatch):
    B, N = 40, 8
    monkeypatch.setenv(SWITCH, "0")
    m, data, noise, faces = _final_case(gpu_device, B, N, precision)
    given = faces.transpose(0, 1).contiguous()
    obs = _mask(B, N, 7)
    changed = list(range(16, 32)) + [3, 4, 35]          # a whole other tile, neighbours inside a tile, one row of the partial tile
    same = [b for b in range(B) if b not in changed]
    obs2, given2, noise2 = obs.clone(), given.clone(), noise.clone()
    obs2[:, changed] = ~obs[:, changed]
    given2[changed] = given[changed] * -0.7 + 0.1
    noise2[:, changed] = noise[:, changed] * 1.1 - 0.05
    got = []
    for o, f, z in ((obs, given, noise), (obs2, given2, noise2)):
        with m.open_stream(_seed(data, 24)) as st:
            out, nll = _many(st, data, f, z, o, 24, 0, N)
            assert st.last_plan == [("rows", 0, N)]
            got.append((out, nll, st.save_rows(list(range(B))).data))
    (out, nll, rec), (out2, nll2, rec2) = got
    assert torch.equal(out[same], out2[same]) and torch.equal(nll[:, same], nll2[:, same]) and torch.equal(rec[same], rec2[same])
    assert not torch.equal(out[changed], out2[changed])


# ---- 3. ignored inputs
def test_ignored_inputs_change_nothing_and_do_not_trip_the_guard(gpu_device):
    B, N = 40, 8
    m, data, noise, faces = _final_case(gpu_device, B, N)
    given = faces.transpose(0, 1).contiguous()
    obs = _mask(B, N, 17, ((4, 2),))
    where = obs.to(gpu_device)
    nan = float("nan")
    with m.open_stream(_seed(data, 24)) as st:
        out, nll = _many(st, data, given, noise, obs, 24, 0, N)
        assert ("observe", 4, 2) in st.last_plan
    dirty_f = torch.where(where.t()[:, :, None], given, torch.full_like(given, nan))       # NaN faces at generating slots
    dirty_n = torch.where(where[:, :, None], torch.full_like(noise, nan), noise)          # NaN noise at observing slots
    with m.open_stream(_seed(data, 24)) as st, warnings.catch_warnings():
        warnings.simplefilter("error")
        a = _many(st, data, dirty_f, dirty_n, obs, 24, 0, 5)
        torch.cuda.synchronize()                      # (the guard's copy has landed: the next call reads it)
        b = _many(st, data, dirty_f, dirty_n, obs, 24, 5, N - 5)
        torch.cuda.synchronize()
        st._check_guard()
        assert st.frame_precision == 9
    got, got_nll = torch.cat([a[0], b[0]], 1), torch.cat([a[1], b[1]])
    with m.open_stream(_seed(data, 24)) as st:
        c = _many(st, data, given, noise, obs, 24, 0, 5)
        d = _many(st, data, given, noise, obs, 24, 5, N - 5)
    assert torch.equal(got, torch.cat([c[0], d[0]], 1)) and torch.equal(got_nll, torch.cat([c[1], d[1]]))
    assert torch.isfinite(got).all() and torch.isfinite(got_nll).all()
    assert _abs(got, out) < FRAME_GATE and max_rel(got_nll, nll, floor=1.0) < NLL_GATE      # (two calls against one)


def test_an_observed_face_beyond_the_fp16_range_trips_the_guard_and_a_generating_slot_does_not(gpu_device):
    B, N = 24, 6
    m, data, noise, faces = _final_case(gpu_device, B, N)
    given = faces.transpose(0, 1).contiguous()
    obs = _mask(B, N, 19)
    obs[1, 3], obs[1, 4] = True, False
    ignored, seen = given.clone(), given.clone()
    ignored[4, 1, 5] = 1.0e5                          # row 4 generates frame 1: never read
    seen[3, 1, 5] = 1.0e5                             # row 3 observes frame 1: trips the guard
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        _many(st, data, ignored, noise, obs, 24, 0, 3)
        torch.cuda.synchronize()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _many(st, data, ignored, noise, obs, 24, 3, 3)
        assert st.frame_precision == 9
    with m.open_stream(_seed(data, 24)) as st:
        _many(st, data, seen, noise, obs, 24, 0, 3)
        torch.cuda.synchronize()                      # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            out, nll = _many(st, data, seen, noise, obs, 24, 3, 3)
        assert st.frame_precision == 5
        clean = [b for b in range(B) if b != 3]
        assert torch.isfinite(out[clean]).all() and torch.isfinite(nll[:, clean]).all()


# ---- 4. the limits
@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_all_generate_is_step_many_and_all_observe_is_observe_many(precision, gpu_device):
    """Within the gates; bit-identity is reported, not asserted (all-generate runs on the rows chain, whose front end does not take the
    reverse chain's window-fragment hand-over)."""
    B, N = 24, 6
    m, data, noise, faces = _final_case(gpu_device, B, N, precision)
    given = faces.transpose(0, 1).contiguous()
    none = torch.zeros(N, B, dtype=torch.bool)
    with m.open_stream(_seed(data, 24), return_nll=True) as st:
        want, want_nll = st.step_many(_chunk(data, 24, 0, N), noise)
    with m.open_stream(_seed(data, 24)) as st:
        out, nll = _many(st, data, given * float("nan"), noise, none, 24, 0, N)
        assert st.last_plan == [("rows", 0, N)]
    err, nerr = _abs(out, want), max_rel(nll, want_nll, floor=1.0)
    report("final widths (%s): an all-False mask vs step_many: frames max abs diff %.3e, NLL max rel diff %.3e, bit-identical: %s"
           % (precision, err, nerr, torch.equal(out, want) and torch.equal(nll, want_nll)))
    assert err < FRAME_GATE and nerr < NLL_GATE
    with m.open_stream(_seed(data, 24)) as st:
        seen = st.observe_many(_chunk(data, 24, 0, N), given)
    with m.open_stream(_seed(data, 24)) as st:
        out, nll = _many(st, data, given, noise * float("nan"), ~none, 24, 0, N)
        assert st.last_plan == [("observe", 0, N)]
    nerr = max_rel(nll, seen, floor=1.0)
    report("final widths (%s): an all-True mask vs observe_many: NLL max rel diff %.3e, bit-identical: %s"
           % (precision, nerr, torch.equal(nll, seen)))
    assert torch.equal(out, given) and nerr < NLL_GATE


# ---- 5. prompt then continue, every fixture
@pytest.mark.parametrize("name", FIXTURES)
def test_prompt_then_continue_against_the_oracle(name, gpu_device):
    """Each row observes its own prompt of the fixture clip and generates the rest. The (B, N, C) sequence the call produced, scored
    teacher-forced by the fp64 oracle; and the frames generated behind the prompts against a session that observe_many(lengths=...)-ed
    the prompts - each row's state taken over at its prompt's end (save_rows -> load_rows, plain copies) - and ran the step_rows()
    loop over the rest."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).contiguous()                # (B, N, C)
    N, B = noise.shape[0], noise.shape[1]
    assert N >= 3
    lengths = torch.tensor([1 + (b * (N - 2)) // max(B - 1, 1) for b in range(B)])        # spread over 1 .. N - 1
    assert int(lengths.min()) == 1 and int(lengths.max()) == (N - 1 if B > 1 else 1)
    obs = torch.arange(N)[:, None] < lengths[None, :]
    where = obs.to(gpu_device)
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            out, nll = _many(st, data, given, noise, obs, fx.start, 0, N)
            assert st.steps == N
        assert torch.equal(out[where.t()], given[where.t()])
        _, expected = fixture_expected(fx, out.cpu())
        e_obs = max_rel(nll[where], expected[obs], floor=1.0)
        e_gen = max_rel(nll[~where], expected[~obs], floor=1.0)
        report("%s step_rows_many (%s), prompts of %s frames: NLL max rel err vs fp64 oracle: observed frames %.3e, generated frames "
               "%.3e" % (name, precision, lengths.tolist(), e_obs, e_gen))
        assert e_obs < NLL_GATE and e_gen < NLL_GATE, (precision, e_obs, e_gen)
        with m.open_stream(_seed(data, fx.start)) as st:
            st.observe_many(_chunk(data, fx.start, 0, N), given, lengths=lengths)
            prompts = st.save_rows(list(range(B)))
        with m.open_stream(_seed(data, fx.start)) as st:
            frames = []
            for n in range(N):
                ends = (lengths == n).nonzero().flatten().tolist()
                if ends:
                    st.load_rows(ends, prompts, ends)
                frames.append(st.step_rows(_frame(data, fx.start + n), given[:, n].contiguous(), obs[n], noise[n])[0])
        ref = torch.stack(frames, 1)
        err = _abs(out[~where.t()], ref[~where.t()])
        report("%s step_rows_many (%s): frames generated behind the prompts vs observe_many(lengths) + the step_rows() loop: max abs "
               "diff %.3e" % (name, precision, err))
        assert err < FRAME_GATE, (precision, err)


# ---- 6. the state carries
@pytest.mark.parametrize("name", CARRY)
def test_the_state_carries_into_and_out_of_the_other_calls(name, gpu_device):
    """A call, one of the other five kinds of call, a call again - against the step_rows() loop of the whole clip under the mask the
    three segments amount to."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).contiguous()
    N, B = noise.shape[0], noise.shape[1]
    k = 3
    assert N >= k + 5
    kinds = (("step", 1, False), ("observe", 1, True), ("step_rows", 1, None), ("step_many", 2, False), ("observe_many", 2, True))
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        worst = {}
        for kind, j, role in kinds:
            obs = _mask(B, N, 41, ((k + j + 1, 2),))
            if role is not None:
                obs[k:k + j] = role
            with m.open_stream(_seed(data, fx.start)) as st:
                want, want_nll = _loop(st, data, given, noise, obs, fx.start, 0, N)
            with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
                head, head_nll = _many(st, data, given, noise, obs, fx.start, 0, k)
                fr, ch = _frame(data, fx.start + k), _chunk(data, fx.start, k, j)
                if kind == "step":
                    mid = st.step(fr, noise[k])[0].unsqueeze(1)
                elif kind == "observe":
                    st.observe(fr, given[:, k].contiguous())
                    mid = given[:, k:k + 1]
                elif kind == "step_rows":
                    mid = st.step_rows(fr, given[:, k].contiguous(), obs[k], noise[k])[0].unsqueeze(1)
                elif kind == "step_many":
                    mid = st.step_many(ch, noise[k:k + j])[0]
                else:
                    st.observe_many(ch, given[:, k:k + j].contiguous())
                    mid = given[:, k:k + j]
                assert st.steps == k + j
                tail, tail_nll = _many(st, data, given, noise, obs, fx.start, k + j, N - k - j)
                assert st.steps == N
            out = torch.cat([head, mid, tail], 1)
            nerr = max(max_rel(head_nll, want_nll[:k], floor=1.0), max_rel(tail_nll, want_nll[k + j:], floor=1.0))
            assert nerr < NLL_GATE, (precision, kind, nerr)
            worst[kind] = _abs(out, want)
        report("%s (%s): step_rows_many, another call, step_rows_many vs the step_rows() loop, frames max abs diff: %s"
               % (name, precision, ", ".join("%s %.3e" % kv for kv in worst.items())))
        assert all(v < FRAME_GATE for v in worst.values()), (precision, worst)


# ---- 7. rounds
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_a_call_split_into_rounds_of_three_frames(name, gpu_device, monkeypatch):
    B, N = 20, 8
    fx, m, data, given, noise = _synthetic(name, gpu_device, B, N)
    obs = _mask(B, N, 43, ((2, 3),))                  # every row observes frames 2 .. 4: the run straddles the first round's end
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            whole = _many(st, data, given, noise, obs, fx.start, 0, N)
            assert st.last_plan == _expected_plan(m, B, obs) and ("observe", 2, 3) in st.last_plan
        monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "3")
        with m.open_stream(_seed(data, fx.start)) as st:
            assert st._chunk_cap() == 3 and N > 3 and N % 3 != 0
            split = _many(st, data, given, noise, obs, fx.start, 0, N)
            assert st.steps == N and st.replays == 0
            plan = st.last_plan
        monkeypatch.delenv("LFI_OBSERVE_CHUNK_FRAMES")
        at = 0
        for kind, first, count in plan:               # all N frames, no gap, no run across a round's end
            assert first == at and count >= 1 and first // 3 == (first + count - 1) // 3
            at += count
        assert at == N and ("observe", 3, 2) in plan and ("observe", 2, 3) not in plan
        err, nerr = _abs(split[0], whole[0]), max_rel(split[1], whole[1], floor=1.0)
        report("%s (%s), %d frames in rounds of 3 vs one round: frames max abs diff %.3e, NLL max rel diff %.3e, bit-identical: %s"
               % (name, precision, N, err, nerr, torch.equal(split[0], whole[0]) and torch.equal(split[1], whole[1])))
        assert err < FRAME_GATE and nerr < NLL_GATE, (precision, err, nerr)


# ---- 8. fallbacks
@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1"))
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_step_rows_many_on_the_fallback_kernels(name, switch, gpu_device, monkeypatch):
    B, N = 20, 6
    fx, m, data, given, noise = _synthetic(name, gpu_device, B, N)
    obs = _mask(B, N, 3, ((3, 2),))
    monkeypatch.setenv(*switch.split("="))
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            want, want_nll = _loop(st, data, given, noise, obs, fx.start, 0, N)
        with m.open_stream(_seed(data, fx.start)) as st:
            out, nll = _many(st, data, given, noise, obs, fx.start, 0, N)
            assert st.last_plan == [("rows", 0, N)]   # no chunk-chain run where that chain does not run
        err, nerr = _abs(out, want), max_rel(nll, want_nll, floor=1.0)
        report("%s step_rows_many (%s, %s) vs the step_rows() loop: frames max abs diff %.3e, NLL max rel diff %.3e"
               % (name, switch, precision, err, nerr))
        assert err < FRAME_GATE and nerr < NLL_GATE, (precision, err, nerr)


# ---- 9. housekeeping
def test_injected_masks_reach_the_frames_they_belong_to(gpu_device, monkeypatch):
    """Train mode with injected (N, B, hist) masks: frame steps + i of the masks goes to frame i of a call - after a per-frame call,
    across two calls and across the rounds of a split call - as the step_rows() loop gives frame n's row to step n."""
    fx = Fixture("p1enc")
    m = build(fx, gpu_device, train=True)
    data, noise, _ = _infer_case(fx, gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).contiguous()
    N, B = noise.shape[0], noise.shape[1]
    rows = list(range(B))
    obs = _mask(B, N, 47, ((4, 2),))
    g = torch.Generator().manual_seed(5)
    m.injected_masks = {e.name: ((torch.rand(N, B, e.hist, generator=g) < 0.6).float() / 0.6)
                        for e in m.spec.encoders if e.dropout > 0 and e.name != "p1_face"}
    assert m.injected_masks and N > 9
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start)) as st:
        want, want_nll = _loop(st, data, given, noise, obs, fx.start, 0, N)
    unmasked = m.injected_masks
    m.injected_masks = {k: torch.ones_like(v) for k, v in unmasked.items()}
    with m.open_stream(_seed(data, fx.start)) as st:
        plain, _ = _many(st, data, given, noise, obs, fx.start, 0, N)
    m.injected_masks = unmasked
    assert _abs(plain, want) > 10 * FRAME_GATE          # the masks matter: a wrong frame's row would show
    for cap in (None, "3"):
        if cap:
            monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", cap)
        with m.open_stream(_seed(data, fx.start)) as st:
            got = [_loop(st, data, given, noise, obs, fx.start, 0, 1), _many(st, data, given, noise, obs, fx.start, 1, 7),
                   _many(st, data, given, noise, obs, fx.start, 8, N - 8)]
            before = st.save_rows(rows).data.clone()
            with pytest.raises(ValueError, match="holds %d frames" % N):
                _many(st, data, given, noise, obs, fx.start, 0, 1)      # beyond the masks: refused, nothing moved
            assert st.steps == N and torch.equal(st.save_rows(rows).data, before)
        err = _abs(torch.cat([a for a, _ in got], 1), want)
        nerr = max_rel(torch.cat([q for _, q in got]), want_nll, floor=1.0)
        report("p1enc, injected dropout masks, step_rows / step_rows_many x 2 (frames per round: %s) vs the step_rows() loop: frames "
               "max abs diff %.3e, NLL max rel diff %.3e" % (cap or "all", err, nerr))
        assert err < FRAME_GATE and nerr < NLL_GATE


@pytest.mark.parametrize("name", ("tiny", "framenb"))
def test_without_noise_the_session_draws_what_the_step_rows_loop_draws(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).contiguous()
    B, n = noise.shape[1], 7
    obs = _mask(B, n, 53)
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start)) as st:
        torch.manual_seed(1234)
        want = torch.stack([st.step_rows(_frame(data, fx.start + i), given[:, i].contiguous(), obs[i])[0] for i in range(n)], 1)
    with m.open_stream(_seed(data, fx.start)) as st:
        torch.manual_seed(1234)
        out, _ = st.step_rows_many(_chunk(data, fx.start, 0, n), given[:, :n].contiguous(), obs)
    with m.open_stream(_seed(data, fx.start)) as st:
        other, _ = _many(st, data, given, noise, obs, fx.start, 0, n)
    err = _abs(out, want)
    report("%s: step_rows_many(noise=None) vs the step_rows() loop after the same seed, %d frames: max abs diff %.3e" % (name, n, err))
    assert err < FRAME_GATE and _abs(out, other) > 10 * FRAME_GATE      # (its own draw, not the clip's)


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "framenb"))
def test_a_call_rolled_back_and_made_again_is_bit_equal(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).contiguous()
    N, B = noise.shape[0], noise.shape[1]
    rows = list(range(B))
    obs = _mask(B, N, 59, ((3, 2),))
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start)) as st:
        _many(st, data, given, noise, obs, fx.start, 0, 2)
        saved = st.save_rows(rows)
        first = _many(st, data, given, noise, obs, fx.start, 2, N - 2)
        other = _many(st, data, given, (noise * 0.5).contiguous(), obs, fx.start, 2, N - 2)      # another candidate
        st.load_rows(rows, saved)
        again = _many(st, data, given, noise, obs, fx.start, 2, N - 2)
        assert st.steps == 2 + 3 * (N - 2)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert not torch.equal(first[0], other[0])


def test_counters_refusals_and_a_stale_session(gpu_device):
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).contiguous()
    N, B = noise.shape[0], noise.shape[1]
    rows = list(range(B))
    obs = _mask(B, N, 61)
    assert N > 9
    st = m.open_stream(_seed(data, fx.start))
    _loop(st, data, given, noise, obs, fx.start, 0, 2)
    assert (st.steps, st.replays) == (2, 1) and st.last_plan is None
    _many(st, data, given, noise, obs, fx.start, 2, 4)
    assert (st.steps, st.replays) == (6, 1) and sum(c for _, _, c in st.last_plan) == 4
    graphs = dict(st._rows_graphs)
    _loop(st, data, given, noise, obs, fx.start, 6, 7)                  # the per-frame graph still stands
    assert (st.steps, st.replays) == (7, 2) and st._rows_graphs == graphs
    before = st.save_rows(rows).data.clone()
    good, f, o, z = _chunk(data, fx.start, 7, 2), given[:, 7:9].contiguous(), obs[7:9], noise[7:9]
    with pytest.raises(ValueError, match=r"step_rows\(\)"):
        st.step_rows_many(good, f, o.to(gpu_device), z)                 # a device-resident mask
    with pytest.raises(ValueError, match="observed"):
        st.step_rows_many(good, f, o[:1], z)                            # one frame's roles for two frames
    with pytest.raises(TypeError, match="observed"):
        st.step_rows_many(good, f, o.int(), z)
    with pytest.raises(ValueError, match="noise"):
        st.step_rows_many(good, f, o, z.transpose(0, 1).contiguous())   # (B, n, C)
    with pytest.raises(ValueError, match="faces"):
        st.step_rows_many(good, given[:, 7:9], o, z)                    # not contiguous
    with pytest.raises(ValueError, match=r"n=2"):
        st.step_rows_many(_chunk(data, fx.start, 7, 3), f, o, z)
    with pytest.raises(KeyError, match="missing modality"):
        st.step_rows_many({}, f, o, z)
    assert st.steps == 7 and torch.equal(st.save_rows(rows).data, before)
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_rows_many(good, f, o, z)
    assert st.steps == 7
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.step_rows_many(good, f, o, z)


def test_step_rows_many_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    B, N = 24, 5
    m, data, noise, faces = _final_case(gpu_device, B, N)
    given = faces.transpose(0, 1).contiguous()
    obs = _mask(B, N, 31, ((2, 2),))
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        on_default = _many(st, data, given, noise, obs, 24, 0, N)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with m.open_stream(_seed(data, 24)) as st:
            on_side = _many(st, data, given, noise, obs, 24, 0, N)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default[0], on_side[0]) and torch.equal(on_default[1], on_side[1])


def test_a_generated_frame_beyond_the_fp16_range_reaches_the_guard(gpu_device):
    """The fold of lfi_stream_chunk_gen_out behind the rows chain, with everything the session is GIVEN in range: one row generates
    among observing ones, every channel of one of its noise rows sits just below the fp16 pieces' limit, the reverse flow's mixing
    carries it beyond the limit, and the guard word then holds max |generated value| - above every input - and trips at the next
    call."""
    B, N = 8, 6
    m, data, noise, faces = _final_case(gpu_device, B, N)
    given = faces.transpose(0, 1).contiguous()
    eng = m._ensure_engine(gpu_device)
    limit = eng._fp16_piece_limit
    obs = torch.ones(N, B, dtype=torch.bool)
    obs[:, 0] = False                                               # row 0 generates, the others observe
    big = noise.clone()
    big[1, 0] = torch.sign(big[1, 0]) * 0.98 * limit               # row 0, frame 1: every channel just inside the range
    big[1, 1:] = float("nan")                                       # (observing rows' noise: never read)
    given_max = max(float(big[:3, 0].abs().max()), float(given.abs().max()),
                    max(float(v.abs().max()) for v in _chunk(data, 24, 0, 3).values()))
    assert given_max < limit
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9 and _guard_value(st) == 0.0
        out, _ = _many(st, data, given, big, obs, 24, 0, 3)
        top = float(out.abs().max())
        report("final widths: noise up to %.1f (limit %g) generates values up to %.1f in the one generating row; guard word %.1f"
               % (given_max, limit, top, _guard_value(st)))
        assert top > limit and float(out[1:].abs().max()) < limit      # (the premise: only a generated value is out of range)
        assert _guard_value(st) == top
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            _many(st, data, given, noise, obs, 24, 3, 3)
        assert st.frame_precision == 5
