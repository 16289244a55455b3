"""GPU: several generated frames per call (SampleStream.step_many -> lfi_stream_chunk_gen_in / the static part once for the chunk /
lfi_flow_sample_seq_nll from the session's live state / lfi_stream_chunk_gen_out): whole reference clips in one call against
inference(), the golden fixtures and the fp64 oracle's NLL, agreement with the step() loop down to the row records, the state carried
into and out of the other kinds of call, the observe_many -> step_many round trip, split rounds and the fallback kernels, two batch
tiles at final widths, injected masks, the session's own noise, rollback, and the housekeeping (counters, refusals, streams, the
range guard).

Gates, all the project's own (tests/test_gpu_stream_observe.py): generated frames FRAME_GATE = 1e-5 absolute against inference(), the
fixture clip or the step() loop; NLL max_rel(nll, expected, floor=1.0) < NLL_GATE = 1e-4."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, report
from sample_nll_expected import fixture_expected
from test_gpu_parity import build
from test_gpu_stream import _frame, _seed
from test_gpu_stream_chunk import _case, _chunk
from test_gpu_stream_observe import FRAME_GATE, NLL_GATE, _final_case, _infer_case

pytestmark = pytest.mark.gpu

CARRY = ("tiny", "tiny_lstm", "tiny_additive", "p1enc", "framenb")


def _many(st, data, noise, start, first, n):
    """Frames first .. first + n - 1 after the seed in one step_many() call."""
    return st.step_many(_chunk(data, start, first, n), noise[first:first + n])


def _loop(st, data, noise, start, first, last):
    """The step() loop over frames first .. last - 1 -> what step() returns, stacked as step_many() orients it."""
    got = [st.step(_frame(data, start + n), noise[n]) for n in range(first, last)]
    if st.return_nll:
        return torch.stack([f for f, _ in got], 1), torch.stack([q for _, q in got])
    return torch.stack(got, 1)


def _abs(a, b):
    return (a - b).abs().max().item()


@pytest.mark.parametrize("name", FIXTURES)
def test_one_call_generates_the_whole_clip_as_inference_does(name, gpu_device):
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    _, expected = fixture_expected(fx)
    N, C = noise.shape[0], frames.shape[2]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        with m.open_stream(_seed(data, fx.start)) as st:
            out = st.step_many(_chunk(data, fx.start, 0, N), noise)
            assert torch.is_tensor(out) and st.steps == N and st.replays == 0
        with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
            out2, nll = st.step_many(_chunk(data, fx.start, 0, N), noise)
            assert st.steps == N and st.replays == 0
        assert tuple(out.shape) == tuple(out2.shape) == (fx.B, N, C) and out.dtype == torch.float32 and out.is_contiguous()
        assert tuple(nll.shape) == (N, fx.B) and nll.dtype == torch.float32
        err_inf, err_fx = max(_abs(out, inf), _abs(out2, inf)), max(_abs(out, frames), _abs(out2, frames))
        err_nll = max_rel(nll, expected, floor=1.0)
        report("%s step_many (%s), %d frames in one call: max abs err vs inference() %.3e, vs the fixture clip %.3e; NLL max rel err "
               "vs fp64 oracle %.3e" % (name, precision, N, err_inf, err_fx, err_nll))
        assert err_inf < FRAME_GATE and err_fx < FRAME_GATE and err_nll < NLL_GATE, (precision, err_inf, err_fx, err_nll)


@pytest.mark.parametrize("name,n", (("tiny", 2), ("tiny", 9), ("mid", 10), ("tiny_lstm", 6), ("p1enc", 6), ("framenb", 6)))
def test_step_many_agrees_with_the_step_loop_down_to_the_row_records(name, n, gpu_device):
    """n below and above the history (tiny: 4 frames), against a long one (mid: 24), an LSTM's c, an encoded faces window and the
    frame counter: the conditioning windows and the counter a call leaves are copies of the same values - bit for bit - and the
    faces window and h / c agree to the generated-frame gate."""
    fx, m, data, noise, _, _ = _case(name, gpu_device)
    rows = list(range(fx.B))
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start), return_nll=True) as one, m.open_stream(_seed(data, fx.start), return_nll=True) as many:
            want, want_nll = _loop(one, data, noise, fx.start, 0, n)
            out, nll = _many(many, data, noise, fx.start, 0, n)
            assert one.steps == many.steps == n
            a, b = one.save_rows(rows), many.save_rows(rows)
            sig = many.row_signature
        ncond = sum(h * d for _, h, d in sig[5])
        err, nerr, serr = _abs(out, want), max_rel(nll, want_nll, floor=1.0), _abs(a.data, b.data)
        report("%s (%s), %d frames, step_many vs %d step() calls: frames max abs diff %.3e, NLL max rel diff %.3e, row records max abs "
               "diff %.3e" % (name, precision, n, n, err, nerr, serr))
        assert a.signature == b.signature == sig
        assert err < FRAME_GATE and nerr < NLL_GATE and serr < FRAME_GATE
        assert torch.equal(a.data[:, :ncond], b.data[:, :ncond])
        if sig[4]:      # the frame counter, the record's last float
            assert torch.equal(a.data[:, -1], b.data[:, -1])


@pytest.mark.parametrize("name", CARRY)
def test_the_state_carries_into_and_out_of_the_other_calls(name, gpu_device):
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    N, Ks = noise.shape[0], m.spec.Ks
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        for k in sorted({1, 2, min(Ks + 1, N - 1), N - 1}):
            worst = {}
            with m.open_stream(_seed(data, fx.start)) as st:
                out = torch.cat([_many(st, data, noise, fx.start, 0, k), _loop(st, data, noise, fx.start, k, N)], 1)
                assert st.steps == N
            worst["step_many, then step()"] = _abs(out, inf)
            with m.open_stream(_seed(data, fx.start)) as st:
                out = torch.cat([_loop(st, data, noise, fx.start, 0, k), _many(st, data, noise, fx.start, k, N - k)], 1)
                assert st.steps == N
            worst["step(), then step_many"] = _abs(out, inf)
            with m.open_stream(_seed(data, fx.start)) as st:
                st.observe_many(_chunk(data, fx.start, 0, k), frames[:, :k].contiguous())
                out = _many(st, data, noise, fx.start, k, N - k)
                assert st.steps == N
            worst["observe_many, then step_many"] = _abs(out, frames[:, k:])
            report("%s (%s), split at %d: %s" % (name, precision, k, ", ".join("%s %.3e" % kv for kv in worst.items())))
            assert all(v < FRAME_GATE for v in worst.values()), (precision, k, worst)


@pytest.mark.parametrize("name", CARRY)
def test_the_latents_of_an_observed_clip_regenerate_it(name, gpu_device):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            _, z = st.observe_many(_chunk(data, fx.start, 0, N), frames.contiguous(), return_z=True)
        with m.open_stream(_seed(data, fx.start)) as st:
            out = st.step_many(_chunk(data, fx.start, 0, N), z)
        err = _abs(out, frames)
        report("%s (%s): observe_many's z through step_many regenerates the clip: max abs err %.3e" % (name, precision, err))
        assert err < FRAME_GATE, (precision, err)


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_a_call_split_into_rounds_of_three_frames(name, gpu_device, monkeypatch):
    """Reported, not asserted: whether the split call is bit-identical to the unsplit one (the fused conditioning's fragment
    hand-over differs at a round's first frame)."""
    fx, m, data, noise, _, _ = _case(name, gpu_device)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
            whole = st.step_many(_chunk(data, fx.start, 0, N), noise)
            assert st.steps == N
        monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "3")
        with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
            assert st._chunk_cap() == 3 and N > 3 and N % 3 != 0
            split = st.step_many(_chunk(data, fx.start, 0, N), noise)
            assert st.steps == N and st.replays == 0
        monkeypatch.delenv("LFI_OBSERVE_CHUNK_FRAMES")
        err, nerr = _abs(split[0], whole[0]), max_rel(split[1], whole[1], floor=1.0)
        report("%s (%s), %d frames in rounds of 3 vs one round: frames max abs diff %.3e, NLL max rel diff %.3e, bit-identical: %s"
               % (name, precision, N, err, nerr, torch.equal(split[0], whole[0]) and torch.equal(split[1], whole[1])))
        assert err < FRAME_GATE and nerr < NLL_GATE, (precision, err, nerr)


@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1"))
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_step_many_on_the_fallback_kernels(name, switch, gpu_device, monkeypatch):
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    _, expected = fixture_expected(fx)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        with monkeypatch.context() as mp:
            mp.setenv(*switch.split("="))
            with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
                out, nll = st.step_many(_chunk(data, fx.start, 0, N), noise)
                assert st.steps == N and st.replays == 0
        err_inf, err_fx, err_nll = _abs(out, inf), _abs(out, frames), max_rel(nll, expected, floor=1.0)
        report("%s step_many (%s, %s): max abs err vs inference() %.3e, vs the fixture clip %.3e; NLL max rel err vs fp64 oracle %.3e"
               % (name, switch, precision, err_inf, err_fx, err_nll))
        assert err_inf < FRAME_GATE and err_fx < FRAME_GATE and err_nll < NLL_GATE, (precision, err_inf, err_fx, err_nll)


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_two_batch_tiles_at_final_widths(precision, gpu_device):
    """B = 20: two 16-row tiles, the second partial. Against the step() loop, and observe_many over the generated frames scores
    the NLL step_many reported for them."""
    N = 8
    m, data, noise, ref, ref_nll = _final_case(gpu_device, 20, N, precision)
    with m.open_stream(_seed(data, 24), return_nll=True) as st:
        out, nll = st.step_many(_chunk(data, 24, 0, N), noise)
        assert st.steps == N and tuple(out.shape) == (20, N, 50) and tuple(nll.shape) == (N, 20)
    with m.open_stream(_seed(data, 24)) as st:
        scored = st.observe_many(_chunk(data, 24, 0, N), out)
    err, nerr, serr = _abs(out, ref), max_rel(nll, ref_nll, floor=1.0), max_rel(scored, nll, floor=1.0)
    report("final widths (%s), B = 20, %d frames: step_many vs the step() loop: frames max abs diff %.3e, NLL max rel diff %.3e; "
           "observe_many over the generated frames vs the NLL reported: max rel diff %.3e" % (precision, N, err, nerr, serr))
    assert err < FRAME_GATE and nerr < NLL_GATE and serr < NLL_GATE


def test_injected_masks_reach_the_frames_they_belong_to(gpu_device, monkeypatch):
    """Train mode with injected (N, B, hist) masks: frame steps + i of the masks goes to frame i of a call - after a per-frame call,
    across two calls and across the rounds of a split call - as the step() loop gives frame n's row to step n."""
    fx = Fixture("p1enc")
    m = build(fx, gpu_device, train=True)
    data, noise, _ = _infer_case(fx, gpu_device)
    N, B = noise.shape[0], noise.shape[1]
    rows = list(range(B))
    g = torch.Generator().manual_seed(5)
    m.injected_masks = {e.name: ((torch.rand(N, B, e.hist, generator=g) < 0.6).float() / 0.6)
                        for e in m.spec.encoders if e.dropout > 0 and e.name != "p1_face"}
    assert m.injected_masks and N > 9
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start)) as st:
        want = _loop(st, data, noise, fx.start, 0, N)
    unmasked = m.injected_masks
    m.injected_masks = {k: torch.ones_like(v) for k, v in unmasked.items()}
    with m.open_stream(_seed(data, fx.start)) as st:
        plain = st.step_many(_chunk(data, fx.start, 0, N), noise)
    m.injected_masks = unmasked
    assert _abs(plain, want) > 10 * FRAME_GATE          # the masks matter: a wrong frame's row would show
    for cap in (None, "3"):
        if cap:
            monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", cap)
        with m.open_stream(_seed(data, fx.start)) as st:
            got = [st.step(_frame(data, fx.start), noise[0]).unsqueeze(1), _many(st, data, noise, fx.start, 1, 7),
                   _many(st, data, noise, fx.start, 8, N - 8)]
            before = st.save_rows(rows).data.clone()
            with pytest.raises(ValueError, match="holds %d frames" % N):
                _many(st, data, noise, fx.start, 0, 1)                 # beyond the masks: refused, nothing moved
            assert st.steps == N and torch.equal(st.save_rows(rows).data, before)
        err = _abs(torch.cat(got, 1), want)
        report("p1enc, injected dropout masks, step / step_many x 2 (frames per round: %s) vs the step() loop: max abs diff %.3e"
               % (cap or "all", err))
        assert err < FRAME_GATE


@pytest.mark.parametrize("name", ("tiny", "framenb"))
def test_without_noise_the_session_draws_what_the_step_loop_draws(name, gpu_device):
    fx, m, data, noise, _, _ = _case(name, gpu_device)
    n = 7
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start)) as st:
        torch.manual_seed(1234)
        want = torch.stack([st.step(_frame(data, fx.start + i)) for i in range(n)], 1)
    with m.open_stream(_seed(data, fx.start)) as st:
        torch.manual_seed(1234)
        out = st.step_many(_chunk(data, fx.start, 0, n))
        again = st.step_many(_chunk(data, fx.start, n, 2))
    err = _abs(out, want)
    report("%s: step_many(noise=None) vs the step() loop after the same seed, %d frames: max abs diff %.3e" % (name, n, err))
    assert tuple(out.shape) == (fx.B, n, want.shape[2]) and tuple(again.shape) == (fx.B, 2, want.shape[2])
    assert err < FRAME_GATE and _abs(out, _many_with(m, fx, data, noise, n)) > 10 * FRAME_GATE     # (its own draw, not the clip's)


def _many_with(m, fx, data, noise, n):
    with m.open_stream(_seed(data, fx.start)) as st:
        return _many(st, data, noise, fx.start, 0, n)


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "framenb"))
def test_a_rollout_rolled_back_and_run_again_is_bit_equal(name, gpu_device):
    fx, m, data, noise, _, _ = _case(name, gpu_device)
    N, rows = noise.shape[0], list(range(fx.B))
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
        _many(st, data, noise, fx.start, 0, 2)
        saved = st.save_rows(rows)
        first = _many(st, data, noise, fx.start, 2, N - 2)
        other = st.step_many(_chunk(data, fx.start, 2, N - 2), (noise[2:] * 0.5).contiguous())     # another candidate
        st.load_rows(rows, saved)
        again = _many(st, data, noise, fx.start, 2, N - 2)
        assert st.steps == 2 + 3 * (N - 2)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert not torch.equal(first[0], other[0])


def test_counters_refusals_and_a_stale_session(gpu_device):
    fx, m, data, noise, _, _ = _case("tiny", gpu_device)
    N, rows = noise.shape[0], list(range(fx.B))
    assert N > 9
    st = m.open_stream(_seed(data, fx.start))
    st.step(_frame(data, fx.start), noise[0])
    st.step(_frame(data, fx.start + 1), noise[1])
    assert (st.steps, st.replays) == (2, 1)
    _many(st, data, noise, fx.start, 2, 4)
    assert (st.steps, st.replays) == (6, 1)
    graph = st._graph
    st.step(_frame(data, fx.start + 6), noise[6])                       # the per-frame graph still stands
    assert (st.steps, st.replays) == (7, 2) and st._graph is graph
    before = st.save_rows(rows).data.clone()
    good = _chunk(data, fx.start, 7, 2)
    with pytest.raises(ValueError, match="noise"):
        st.step_many(good, noise[7:9].transpose(0, 1).contiguous())     # (B, n, C)
    with pytest.raises(ValueError, match=r"n=2"):
        st.step_many(good, noise[7:10])
    with pytest.raises(ValueError, match="noise"):
        st.step_many(good, noise[7:9, :, :3])                           # not contiguous, too narrow
    with pytest.raises(ValueError, match="expected contiguous"):
        st.step_many({k: v[:, :, :-1] for k, v in good.items()}, noise[7:9])
    with pytest.raises(KeyError, match="missing modality"):
        st.step_many({}, noise[7:9])
    with pytest.raises(TypeError, match="frames must be a dict"):
        st.step_many(noise[7:9])
    assert st.steps == 7 and torch.equal(st.save_rows(rows).data, before)
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_many(good, noise[7:9])
    assert st.steps == 7
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.step_many(good, noise[7:9])


def test_step_many_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    m, data, noise, _, _ = _final_case(gpu_device, 8, 5)
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    with m.open_stream(_seed(data, 24), return_nll=True) as st:
        on_default = st.step_many(_chunk(data, 24, 0, 5), noise)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with m.open_stream(_seed(data, 24), return_nll=True) as st:
            on_side = st.step_many(_chunk(data, 24, 0, 5), noise)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default[0], on_side[0]) and torch.equal(on_default[1], on_side[1])


def _guard_value(st):
    """The session's guard word as the float it holds (max |v| of everything folded since the open)."""
    torch.cuda.synchronize()
    return st.guard[:1].view(torch.float32).item()


def test_a_noise_row_beyond_the_fp16_range_trips_the_guard(gpu_device):
    """The noise fold of lfi_stream_chunk_gen_in: a noise row of 1e5 in the first call is reported at the next call, the session
    goes on with six bf16 products, and the rows that never left the range give what a session opened with six bf16 products gives.
    (The fold of the generated frames, lfi_stream_chunk_gen_out's, is the next test's.)"""
    N = 10
    m, data, noise, _, _ = _final_case(gpu_device, 8, N)
    bad = noise.clone()
    bad[2, 0] *= 1.0e5 / float(bad[2, 0].abs().max())      # row 0, frame 2: inside the first call, sampled with fp16 pieces
    eng = m._ensure_engine(gpu_device)
    eng.sample_frame_precision = 5
    try:
        with m.open_stream(_seed(data, 24)) as st:
            assert st.frame_precision == 5
            want = st.step_many(_chunk(data, 24, 0, N), bad)
    finally:
        eng.sample_frame_precision = None
    clean = [b for b in range(8) if b != 0]
    assert torch.isfinite(want[clean]).all()
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        got = [_many(st, data, bad, 24, 0, 4)]
        torch.cuda.synchronize()                   # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            got.append(_many(st, data, bad, 24, 4, 3))
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got.append(_many(st, data, bad, 24, 7, N - 7))
    got = torch.cat(got, 1)
    assert torch.isfinite(got[clean]).all()
    err = _abs(got[clean], want[clean])
    report("final widths: step_many with a noise row of 1e5 in the first call, rows that never left the range vs a session opened "
           "with six bf16 products: max abs diff %.3e" % err)
    assert err < FRAME_GATE


def test_a_generated_frame_beyond_the_fp16_range_reaches_the_guard(gpu_device):
    """The fold of lfi_stream_chunk_gen_out, with everything the session is GIVEN in range: every channel of one noise row sits just
    below the fp16 pieces' limit, the reverse flow's mixing carries it beyond the limit, and the guard word then holds max |generated value| -
    above every input - and trips at the next call."""
    N = 6
    m, data, noise, _, _ = _final_case(gpu_device, 8, N)
    eng = m._ensure_engine(gpu_device)
    limit = eng._fp16_piece_limit
    big = noise.clone()
    big[1, 0] = torch.sign(big[1, 0]) * 0.98 * limit               # row 0, frame 1: every channel just inside the range
    given = max(float(big[:3].abs().max()), max(float(v.abs().max()) for v in _chunk(data, 24, 0, 3).values()))
    assert given < limit
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9 and _guard_value(st) == 0.0
        out = _many(st, data, big, 24, 0, 3)
        top = float(out.abs().max())
        report("final widths: noise up to %.1f (limit %g) generates values up to %.1f; guard word %.1f" % (given, limit, top,
                                                                                                            _guard_value(st)))
        assert top > limit                         # (the premise: only a generated value is out of range)
        assert _guard_value(st) == top
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            _many(st, data, noise, 24, 3, 3)
        assert st.frame_precision == 5
