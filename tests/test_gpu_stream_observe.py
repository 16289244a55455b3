"""GPU: teacher-forced steps of streaming sessions (SampleStream.observe -> lfi_flow_score_seq_from, the forward chain): the NLL and
the latent of observed frames against the fp64 oracle on every golden fixture, sessions that mix observed and generated frames
against inference() and against a session's own reported NLL, graph replay against eager launches, rows moved and reseeded, no host
synchronisation in steady state, the range guard, refusals, and the caller's stream.

Gates, all the project's own: NLL max_rel(nll, expected, floor=1.0) < 1e-4 (tests/test_gpu_sample_nll.py); z rel_err < 1e-5
(tests/test_gpu_parity.py, forward()'s z); generated frames of a session against inference() 1e-5 absolute (tests/test_gpu_stream.py)."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, rel_err, report
from sample_nll_expected import fixture_expected
from test_gpu_parity import build, to_dev
from test_gpu_stream import _final_setup, _frame, _seed

pytestmark = pytest.mark.gpu

NLL_GATE = 1e-4
Z_GATE = 1e-5
FRAME_GATE = 1e-5


def _infer_case(fx, device):
    data = to_dev(fx.group("infer/data/"), device)
    noise = fx.get("infer/noise", torch.float32).to(device)
    return data, noise, int(fx.get("infer/seq_len"))


def _face(frames, n):
    return frames[:, n].contiguous()


def _final_case(device, B, frames, precision="bf16x3"):
    """_final_setup's model with a reference session: its generated frames and their NLL (a return_nll session, step by step)."""
    _, m, _, data, noise, _ = _final_setup(device, B, frames)
    m.precision = precision
    data, noise = to_dev(data, device), noise.to(device)
    with m.open_stream(_seed(data, 24), return_nll=True) as st:
        steps = [st.step(_frame(data, 24 + n), noise[n]) for n in range(frames)]
    return m, data, noise, torch.stack([f for f, _ in steps], 1), torch.stack([q for _, q in steps])


@pytest.mark.parametrize("name", FIXTURES)
def test_observe_scores_the_reference_frames_as_the_oracle_does(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    frames = fx.get("infer/out", torch.float32).to(gpu_device)
    _, expected = fixture_expected(fx)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            got = [st.observe(_frame(data, fx.start + n), _face(frames, n), return_z=True) for n in range(N)]
            assert st.steps == N and st.replays == N - 1
        nll, z = torch.stack([q for q, _ in got]), torch.stack([v for _, v in got])
        assert all(tuple(q.shape) == (fx.B,) and q.dtype == torch.float32 and tuple(v.shape) == (fx.B, frames.shape[2]) for q, v in got)
        err, zerr = max_rel(nll, expected, floor=1.0), rel_err(z, fx.get("infer/noise"))
        report("%s observe (%s): NLL max rel err vs fp64 oracle %.3e; z rel err vs infer/noise %.3e" % (name, precision, err, zerr))
        assert err < NLL_GATE and zerr < Z_GATE, (precision, err, zerr)


@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1", "LFI_PIPE_X3=0", "LFI_SAMPLE_FUSED=0"))
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_observe_on_the_per_step_launches_and_the_other_cell_forms(name, switch, gpu_device, monkeypatch):
    """Ks launches of the streaming forward cell + the finish (LFI_SAMPLE_CHAIN=0, LFI_FLOW_GENERIC=1), the chain's exact-f32 cell in
    bf16x3 mode (LFI_PIPE_X3=0) and the unfused conditioning: the same gates, and generation carries on from the state they leave."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, seq_len = _infer_case(fx, gpu_device)
    frames = fx.get("infer/out", torch.float32).to(gpu_device)
    _, expected = fixture_expected(fx)
    N, split = noise.shape[0], noise.shape[0] // 2
    m.precision = "bf16x3"
    inf = m.inference(seq_len, data, noise=noise)
    monkeypatch.setenv(*switch.split("="))
    with m.open_stream(_seed(data, fx.start)) as st:
        # (every other frame without z: the entry point's z = NULL form of these paths)
        got = [st.observe(_frame(data, fx.start + n), _face(frames, n), return_z=True) if n % 2 == 0
               else (st.observe(_frame(data, fx.start + n), _face(frames, n)), None) for n in range(split)]
        out = torch.stack([st.step(_frame(data, fx.start + n), noise[n]) for n in range(split, N)], 1)
    nll, z = torch.stack([q for q, _ in got]), torch.stack([v for _, v in got[::2]])
    err, zerr = max_rel(nll, expected[:split], floor=1.0), rel_err(z, fx.get("infer/noise")[:split:2])
    ferr = (out - inf[:, split:]).abs().max().item()
    report("%s observe (%s): NLL max rel err %.3e, z rel err %.3e, generation afterwards max abs err vs inference() %.3e"
           % (name, switch, err, zerr, ferr))
    assert err < NLL_GATE and zerr < Z_GATE and ferr < FRAME_GATE


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "tiny_additive", "p1enc", "framenb"))
def test_observed_prefix_then_generation_matches_inference(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, seq_len = _infer_case(fx, gpu_device)
    frames = fx.get("infer/out", torch.float32).to(gpu_device)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        for split in sorted({1, N // 2, N - 1}):
            with m.open_stream(_seed(data, fx.start)) as st:
                for n in range(split):
                    st.observe(_frame(data, fx.start + n), _face(frames, n))
                out = torch.stack([st.step(_frame(data, fx.start + n), noise[n]) for n in range(split, N)], 1)
            err = (out - inf[:, split:]).abs().max().item()
            report("%s (%s): %d observed frames, then generation: max abs err vs inference() %.3e" % (name, precision, split, err))
            assert err < FRAME_GATE, (precision, split, err)


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_mixed_sessions_at_final_model_widths(precision, gpu_device):
    N = 8
    m, data, noise, ref, ref_nll = _final_case(gpu_device, 8, N, precision)
    for split in (1, N // 2, N - 1):
        # observed, then generated
        with m.open_stream(_seed(data, 24)) as st:
            for n in range(split):
                st.observe(_frame(data, 24 + n), _face(ref, n))
            out = torch.stack([st.step(_frame(data, 24 + n), noise[n]) for n in range(split, N)], 1)
        err = (out - ref[:, split:]).abs().max().item()
        # generated, then the session's own output observed
        with m.open_stream(_seed(data, 24)) as st:
            for n in range(split):
                st.step(_frame(data, 24 + n), noise[n])
            nll = torch.stack([st.observe(_frame(data, 24 + n), _face(ref, n)) for n in range(split, N)])
        nerr = max_rel(nll, ref_nll[split:], floor=1.0)
        report("final widths (%s), split %d: observed then generated max abs err %.3e; generated then observed NLL max rel diff %.3e"
               % (precision, split, err, nerr))
        assert err < FRAME_GATE and nerr < NLL_GATE, (split, err, nerr)
    # strict alternation: even frames generated, odd frames observed
    with m.open_stream(_seed(data, 24)) as st:
        worst_f = worst_q = 0.0
        for n in range(N):
            if n % 2 == 0:
                worst_f = max(worst_f, (st.step(_frame(data, 24 + n), noise[n]) - ref[:, n]).abs().max().item())
            else:
                worst_q = max(worst_q, max_rel(st.observe(_frame(data, 24 + n), _face(ref, n)), ref_nll[n], floor=1.0))
    report("final widths (%s), alternating: frames max abs err %.3e, NLL max rel diff %.3e" % (precision, worst_f, worst_q))
    assert worst_f < FRAME_GATE and worst_q < NLL_GATE


def _observe_all(st, data, ref, first, last):
    got = [st.observe(_frame(data, 24 + n), _face(ref, n), return_z=True) for n in range(first, last)]
    return torch.stack([q for q, _ in got]), torch.stack([v for _, v in got])


def _alternate(st, data, noise, ref, N):
    return [st.step(_frame(data, 24 + n), noise[n]) if n % 2 == 0 else st.observe(_frame(data, 24 + n), _face(ref, n))
            for n in range(N)]


def test_observe_graph_replay_is_bit_identical_to_eager(gpu_device, monkeypatch):
    N = 7
    for precision in ("bf16x3", "f32"):
        m, data, noise, ref, _ = _final_case(gpu_device, 8, N, precision)
        with m.open_stream(_seed(data, 24)) as st:
            nll, z = _observe_all(st, data, ref, 0, N)
            assert st.steps == N and st.replays == N - 1     # observe 1 eager, observes 2.. one replayed graph
            assert st._graph is None and len(st._observe_graphs) == 1
        with m.open_stream(_seed(data, 24)) as st:
            mixed = _alternate(st, data, noise, ref, N)
            assert st.steps == N and st.replays == N - 1     # both kinds of replay are counted
            graphs = (st._graph, dict(st._observe_graphs))
            assert graphs[0] is not None and len(graphs[1]) == 1
            more = _alternate(st, data, noise, ref, 4)
            assert (st._graph, st._observe_graphs) == graphs and st.replays == N + 3     # nothing recaptured
            # with and without z are two graphs (z = NULL when it is not wanted): flipping return_z recaptures nothing either
            st.observe(_frame(data, 24 + 4), _face(ref, 4), return_z=True)
            both = dict(st._observe_graphs)
            assert len(both) == 2
            for flag in (False, True, False, True):
                st.observe(_frame(data, 24 + 5), _face(ref, 5), return_z=flag)
            assert st._observe_graphs == both and st._graph is graphs[0]
        monkeypatch.setenv("LFI_NO_GRAPH", "1")
        with m.open_stream(_seed(data, 24)) as st:
            e_nll, e_z = _observe_all(st, data, ref, 0, N)
            assert st.replays == 0
        with m.open_stream(_seed(data, 24)) as st:
            e_mixed = _alternate(st, data, noise, ref, N)
            assert st.replays == 0 and st._graph is None and not st._observe_graphs
        monkeypatch.delenv("LFI_NO_GRAPH")
        assert torch.equal(nll, e_nll) and torch.equal(z, e_z), precision
        assert all(torch.equal(a, b) for a, b in zip(mixed, e_mixed)), precision
        assert len(more) == 4


def test_observed_rows_move_between_sessions_and_reseeded_rows_start_afresh(gpu_device):
    N, at = 8, 3
    m, data, noise, ref, _ = _final_case(gpu_device, 8, N)
    rows = [1, 6]
    sub = {k: v[rows].contiguous() for k, v in data.items()}
    # warm-up session -> save_rows -> a serving session of another batch size
    with m.open_stream(_seed(data, 24)) as warm, m.open_stream(_seed(sub, 24)) as serve:
        for n in range(at):
            warm.observe(_frame(data, 24 + n), _face(ref, n))
        serve.load_rows([1, 0], warm.save_rows(rows))           # entry 0 (row 1) -> serving row 1, entry 1 (row 6) -> serving row 0
        sub_sw = {k: v[[rows[1], rows[0]]].contiguous() for k, v in data.items()}
        moved = torch.stack([serve.step(_frame(sub_sw, 24 + n), noise[n][[rows[1], rows[0]]].contiguous()) for n in range(at, N)], 1)
        stay = torch.stack([warm.step(_frame(data, 24 + n), noise[n]) for n in range(at, N)], 1)
    err = (moved - stay[[rows[1], rows[0]]]).abs().max().item()
    report("final widths: rows observed for %d frames, moved into a session of batch 2, then generated: max abs diff %.3e" % (at, err))
    assert err < FRAME_GATE
    # reset_rows, then observe: the row reports what a fresh session on that seed reports; the others carry on bit for bit
    r = 2
    with m.open_stream(_seed(data, 24)) as st:
        undisturbed, _ = _observe_all(st, data, ref, 0, N)
    with m.open_stream(_seed(data, 24)) as st:
        got = []
        for n in range(N):
            fr, face = _frame(data, 24 + n), _face(ref, n).clone()
            if n == at:
                st.reset_rows([r], {k: v[r:r + 1].contiguous() for k, v in _seed(data, 24).items()})
            if n >= at:       # row r lives its sequence again from the start
                for k, v in _frame(data, 24 + n - at).items():
                    fr[k][r] = v[r]
                face[r] = ref[r, n - at]
            got.append(st.observe(fr, face))
        got = torch.stack(got)
    others = [b for b in range(8) if b != r]
    err = max_rel(got[at:, r], undisturbed[:N - at, r], floor=1.0)
    report("final widths: NLL of a row reseeded after %d observed frames vs a fresh session on its seed: max rel diff %.3e" % (at, err))
    assert err < NLL_GATE
    assert torch.equal(got[:, others], undisturbed[:, others]) and torch.equal(got[:at], undisturbed[:at])


def test_steady_state_observes_do_not_synchronise(gpu_device):
    m, data, noise, ref, _ = _final_case(gpu_device, 8, 10)
    frames = [_frame(data, 24 + n) for n in range(10)]
    faces = [_face(ref, n) for n in range(10)]
    with m.open_stream(_seed(data, 24)) as st:
        st.observe(frames[0], faces[0])
        st.observe(frames[1], faces[1])                     # (a capture synchronises once: observe without z,
        st.observe(frames[2], faces[2], return_z=True)      # with z,
        st.step(frames[3], noise[3])                        # and the step graph)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for n in range(4, 7):
                st.observe(frames[n], faces[n], return_z=n % 2 == 0)
            st.step(frames[7], noise[7])
            st.observe(frames[8], faces[8])
            st.step(frames[9])                              # noise drawn by the session
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 9


def test_observed_face_beyond_the_fp16_range_falls_back_to_six_bf16_products(gpu_device):
    """A face beyond the fp16 pieces' range trips the guard: the warning, and the session observes with the range-free arithmetic
    (per-frame precision 5: six bf16 products in the conditioning GEMMs, the exact-f32 forward cell) from then on. What it reports
    afterwards is finite and what a session opened at precision 5 reports - also for a face beyond the range observed AFTER the
    fallback. The row whose out-of-range face was observed with fp16 pieces is the one the warning speaks of ("frames since that
    input may be inaccurate"): it is compared only in the session that never used them."""
    N = 10
    m, data, noise, ref, _ = _final_case(gpu_device, 8, N)
    bad = ref.clone()
    bad[0, 2, 5] = 1.0e5                           # beyond fp16's range, row 0, observed with fp16 pieces: trips the guard
    bad[3, 6, 7] = -3.0e5                          # row 3, observed after the fallback
    bad[0, 7, 1] = 2.0e5                           # (and row 0 again)
    eng = m._ensure_engine(gpu_device)
    eng.sample_frame_precision = 5
    try:
        with m.open_stream(_seed(data, 24)) as st:     # precision 5 from the open
            assert st.frame_precision == 5
            want = torch.stack([st.observe(_frame(data, 24 + n), _face(bad, n)) for n in range(N)])
    finally:
        eng.sample_frame_precision = None
    assert torch.isfinite(want).all()               # no range caveat: every row, the out-of-range frames included
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        got = [st.observe(_frame(data, 24 + n), _face(bad, n)) for n in range(3)]
        torch.cuda.synchronize()                   # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            got.append(st.observe(_frame(data, 27), _face(bad, 3)))
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got += [st.observe(_frame(data, 24 + n), _face(bad, n)) for n in range(4, N)]
            tail = st.step(_frame(data, 24 + N - 1), noise[N - 1])      # generation carries on from that state
    got = torch.stack(got)
    clean = [b for b in range(8) if b != 0]
    assert torch.isfinite(got[3:, clean]).all() and torch.isfinite(tail[clean]).all()
    err = max_rel(got[3:, clean], want[3:, clean], floor=1.0)
    report("final widths: NLL observed after the range guard's fallback (an out-of-range face among them) vs a session opened with six "
           "bf16 products: max rel diff %.3e" % err)
    assert err < NLL_GATE
    assert float(got[6, 3]) > 1e6                   # the out-of-range face is scored, not dropped: an enormous NLL, finite


def test_observe_is_refused_after_a_parameter_change_and_after_close(gpu_device):
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data, _, _ = _infer_case(fx, gpu_device)
    frames = fx.get("infer/out", torch.float32).to(gpu_device)
    st = m.open_stream(_seed(data, fx.start))
    st.observe(_frame(data, fx.start), _face(frames, 0))
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.observe(_frame(data, fx.start + 1), _face(frames, 1))
    st = m.open_stream(_seed(data, fx.start))
    st.observe(_frame(data, fx.start), _face(frames, 0))
    with pytest.raises(ValueError, match="face"):
        st.observe(_frame(data, fx.start + 1), frames[:, 1])          # not contiguous
    with pytest.raises(ValueError, match="face"):
        st.observe(_frame(data, fx.start + 1), _face(frames, 1)[:, :3].contiguous())
    assert st.steps == 1
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.observe(_frame(data, fx.start + 1), _face(frames, 1))


def test_observe_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    m, data, noise, ref, _ = _final_case(gpu_device, 8, 5)
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        on_default = _observe_all(st, data, ref, 0, 5)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with m.open_stream(_seed(data, 24)) as st:
            on_side = _observe_all(st, data, ref, 0, 5)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default[0], on_side[0]) and torch.equal(on_default[1], on_side[1])
