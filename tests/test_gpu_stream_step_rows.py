"""GPU: the per-row step of streaming sessions (SampleStream.step_rows -> lfi_stream_advance_rows, lfi_flow_step_rows_from, both chains
in one launch with row-masked stores): every row bit for bit what the pure call of its role gives it, the all-generate and
all-observe limits, graph replay and a changing mask, the per-step launches and the other cell forms, inputs that are ignored, the
fp64 oracle on every golden fixture, and the session contract (no host wait, the caller's stream, rows moved and reseeded, refusals).

Exactness is torch.equal on fp32 bits. Gates against the oracle are the project's own: NLL max_rel(nll, expected, floor=1.0) < 1e-4
(tests/test_gpu_sample_nll.py), generated frames of a session 1e-5 absolute (tests/test_gpu_stream.py)."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, report
from sample_nll_expected import fixture_expected
from test_gpu_parity import build, to_dev
from test_gpu_stream import _final_setup, _frame, _seed

pytestmark = pytest.mark.gpu

NLL_GATE = 1e-4
FRAME_GATE = 1e-5


def _schedule(B, N, seed):
    """(N, B) bool roles, True = the row observes. Per 16-row tile and frame one of three modes, cycling with frame + tile: every row
    generates, every row observes, rows interleaved at random (both roles present when the tile has two rows) - so every tile is
    all-generate, all-observe and mixed at some frame, and rows change role mid-sequence."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.zeros(N, B, dtype=torch.bool)
    for t in range(N):
        for tile, b0 in enumerate(range(0, B, 16)):
            n = min(16, B - b0)
            mode = (t + tile) % 3
            if mode == 1:
                obs[t, b0:b0 + n] = True
            elif mode == 2:
                r = torch.rand(n, generator=g) < 0.5
                if n > 1:
                    r[0], r[1] = True, False
                obs[t, b0:b0 + n] = r
    return obs


def _case(m, device, B, N, start, seed=11):
    """Random conditioning, seed, faces and noise for the model `m`: N frames after `start` seed frames."""
    g = torch.Generator().manual_seed(seed)
    C = m.spec.C
    data = {"p1_face": torch.randn(B, start, C, generator=g)}
    for e in m.spec.encoders:
        if e.name not in ("p1_face", "frame_nb"):
            data[e.name] = torch.randn(B, start + N, e.in_dim, generator=g)
    faces = torch.randn(N, B, C, generator=g) * 0.5
    noise = torch.randn(N, B, C, generator=g) * 0.8
    return to_dev(data, device), faces.to(device), noise.to(device)


def _spec_model(m, device):
    m._ensure_engine(device)
    return m


def _against_pure_calls(m, data, faces, noise, obs, start, label):
    """Session M takes step_rows(); two reference sessions of the same batch, opened with return_nll, take step() and observe() of
    the same frame and are then put back on M's state (save_rows -> load_rows, plain copies), so both hold M's history bit for bit
    before every frame. Row r of frame t is compared against exactly one pure call: the one of its role."""
    N, B = obs.shape
    dev = faces.device
    every = list(range(B))
    mism = 0
    with m.open_stream(_seed(data, start)) as M, m.open_stream(_seed(data, start), return_nll=True) as G, \
            m.open_stream(_seed(data, start), return_nll=True) as O:
        for t in range(N):
            fr = _frame(data, start + t)
            o = obs[t].to(dev)
            out, nll = M.step_rows(fr, faces[t], o, noise[t])
            assert tuple(out.shape) == (B, faces.shape[2]) and tuple(nll.shape) == (B,) and nll.dtype == torch.float32
            g_out, g_nll = G.step(fr, noise[t])
            o_nll = O.observe(fr, faces[t])
            rec, g_rec, o_rec = M.save_rows(every), G.save_rows(every), O.save_rows(every)
            assert rec.signature == g_rec.signature == M.row_signature
            want_out = torch.where(o[:, None], faces[t], g_out)
            want_nll = torch.where(o, o_nll, g_nll)
            want_rec = torch.where(o[:, None], o_rec.data, g_rec.data)
            ok = torch.equal(out, want_out) and torch.equal(nll, want_nll) and torch.equal(rec.data, want_rec)
            if not ok:
                mism += 1
                report("%s: frame %d: out differs in rows %s, nll in rows %s, record in rows %s" % (
                    label, t, (out != want_out).any(1).nonzero().flatten().tolist(), (nll != want_nll).nonzero().flatten().tolist(),
                    (rec.data != want_rec).any(1).nonzero().flatten().tolist()))
            G.load_rows(every, rec)
            O.load_rows(every, rec)
        assert M.steps == N and M.replays == N - 1 and len(M._rows_graphs) == 1
    report("%s: %d frames x %d rows of step_rows against the pure call of each row's role: %d frames differ" % (label, N, B, mism))
    assert mism == 0


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "tiny_additive", "p1enc", "framenb"))
def test_every_row_is_bit_identical_to_the_pure_call_of_its_role(name, gpu_device):
    fx = Fixture(name)
    m = _spec_model(build(fx, gpu_device), gpu_device)
    B, N = 20, 12                                     # two tiles, the second partial
    obs = _schedule(B, N, 5)
    data, faces, noise = _case(m, gpu_device, B, N, fx.start)
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        _against_pure_calls(m, data, faces, noise, obs, fx.start, "%s (%s)" % (name, precision))


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_every_row_is_bit_identical_at_final_model_widths(precision, gpu_device):
    B, N = 40, 12                                     # three tiles, the last partial
    _, m, _, data, noise, _ = _final_setup(gpu_device, B, N)
    m.precision = precision
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    g = torch.Generator().manual_seed(2)
    faces = (torch.randn(N, B, 50, generator=g) * 0.5).to(gpu_device)
    obs = _schedule(B, N, 7)
    tiles = [obs[:, b0:b0 + 16] for b0 in (0, 16, 32)]
    assert all((~tl).all(1).any() and tl.all(1).any() and (tl.any(1) & ~tl.all(1)).any() for tl in tiles)
    assert (obs[1:] != obs[:-1]).any(0).all()         # every row changes role mid-sequence
    _against_pure_calls(m, data, faces, noise, obs, 24, "final widths (%s)" % precision)


def _final_case(device, B, N, precision="bf16x3"):
    _, m, _, data, noise, _ = _final_setup(device, B, N)
    m.precision = precision
    g = torch.Generator().manual_seed(4)
    faces = (torch.randn(N, B, 50, generator=g) * 0.5).to(device)
    return m, to_dev(data, device), noise.to(device), faces


def _rows_run(st, data, faces, noise, obs, first=0, last=None):
    last = obs.shape[0] if last is None else last
    got = [st.step_rows(_frame(data, 24 + n), faces[n], obs[n], noise[n]) for n in range(first, last)]
    return torch.stack([a for a, _ in got]), torch.stack([q for _, q in got])


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_all_generate_is_step_and_all_observe_is_observe(precision, gpu_device, monkeypatch):
    B, N = 24, 6
    m, data, noise, faces = _final_case(gpu_device, B, N, precision)
    none = torch.zeros(N, B, dtype=torch.bool, device=gpu_device)
    for eager in (False, True):
        if eager:
            monkeypatch.setenv("LFI_NO_GRAPH", "1")
        with m.open_stream(_seed(data, 24), return_nll=True) as st:
            steps = [st.step(_frame(data, 24 + n), noise[n]) for n in range(N)]
        with m.open_stream(_seed(data, 24)) as st:
            out, nll = _rows_run(st, data, faces * float("nan"), noise, none)
            assert st.replays == (0 if eager else N - 1)
        assert torch.equal(out, torch.stack([f for f, _ in steps])) and torch.equal(nll, torch.stack([q for _, q in steps])), eager
        with m.open_stream(_seed(data, 24)) as st:
            seen = torch.stack([st.observe(_frame(data, 24 + n), faces[n]) for n in range(N)])
        with m.open_stream(_seed(data, 24), return_nll=True) as st:
            out, nll = _rows_run(st, data, faces, noise, ~none)
        assert torch.equal(out, faces) and torch.equal(nll, seen), eager
        if eager:
            monkeypatch.delenv("LFI_NO_GRAPH")


def test_replay_is_bit_identical_to_eager_and_a_changing_mask_captures_one_graph(gpu_device, monkeypatch):
    B, N = 40, 9
    for precision in ("bf16x3", "f32"):
        m, data, noise, faces = _final_case(gpu_device, B, N, precision)
        obs = _schedule(B, N, 13).to(gpu_device)
        assert all(not torch.equal(obs[n], obs[n + 1]) for n in range(N - 1))      # the mask changes at every call
        with m.open_stream(_seed(data, 24)) as st:
            out, nll = _rows_run(st, data, faces, noise, obs)
            assert st.steps == N and st.replays == N - 1
            assert len(st._rows_graphs) == 1 and st._graph is None and not st._observe_graphs
            graphs = dict(st._rows_graphs)
            # the other kinds of step in between keep their own graphs; nothing of step_rows is recaptured
            st.step(_frame(data, 24), noise[0])
            st.observe(_frame(data, 24), faces[0])
            st.step_rows(_frame(data, 24), faces[0], obs[3].tolist(), noise[0])     # a host mask
            st.step_rows(_frame(data, 24), faces[0], obs[4].cpu(), None)            # a CPU tensor, noise drawn by the session
            assert st._rows_graphs == graphs and st.replays == N + 3
        monkeypatch.setenv("LFI_NO_GRAPH", "1")
        with m.open_stream(_seed(data, 24)) as st:
            e_out, e_nll = _rows_run(st, data, faces, noise, obs)
            assert st.replays == 0 and not st._rows_graphs
        monkeypatch.delenv("LFI_NO_GRAPH")
        assert torch.equal(out, e_out) and torch.equal(nll, e_nll), precision


@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1", "LFI_SAMPLE_FUSED=0", "LFI_PIPE_X3=0"))
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_rows_on_the_per_step_launches_and_the_other_cell_forms(name, switch, gpu_device, monkeypatch):
    fx = Fixture(name)
    m = _spec_model(build(fx, gpu_device), gpu_device)
    B, N = 20, 6
    obs = _schedule(B, N, 3)
    data, faces, noise = _case(m, gpu_device, B, N, fx.start)
    m.precision = "bf16x3"
    monkeypatch.setenv(*switch.split("="))
    _against_pure_calls(m, data, faces, noise, obs, fx.start, "%s (%s)" % (name, switch))


def test_ignored_inputs_change_nothing_and_do_not_trip_the_guard(gpu_device):
    B, N = 40, 8
    m, data, noise, faces = _final_case(gpu_device, B, N)
    obs = _schedule(B, N, 17).to(gpu_device)
    nan = float("nan")
    with m.open_stream(_seed(data, 24)) as st:
        out, nll = _rows_run(st, data, faces, noise, obs)
    dirty_f = torch.where(obs[:, :, None], faces, torch.full_like(faces, nan))      # NaN face in generating rows
    dirty_n = torch.where(obs[:, :, None], torch.full_like(noise, nan), noise)      # NaN noise in observing rows
    with m.open_stream(_seed(data, 24)) as st, warnings.catch_warnings():
        warnings.simplefilter("error")
        got = []
        for n in range(N):
            got.append(st.step_rows(_frame(data, 24 + n), dirty_f[n], obs[n], dirty_n[n]))
            torch.cuda.synchronize()                  # (the guard's copy has landed: the next call reads it)
        assert st.frame_precision == 9
    assert torch.equal(out, torch.stack([a for a, _ in got])) and torch.equal(nll, torch.stack([q for _, q in got]))
    assert torch.isfinite(out).all() and torch.isfinite(nll).all()


def test_observed_face_beyond_the_fp16_range_trips_the_guard_as_observe_does(gpu_device):
    B, N = 24, 6
    m, data, noise, faces = _final_case(gpu_device, B, N)
    obs = _schedule(B, N, 19).to(gpu_device)
    obs[1, 3], obs[1, 4] = True, False
    bad = faces.clone()
    bad[1, 3, 5] = 1.0e5                              # an observing row: trips the guard
    bad[1, 4, 5] = 1.0e5                              # a generating row: never read
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        st.step_rows(_frame(data, 24), bad[0], obs[0], noise[0])
        st.step_rows(_frame(data, 25), torch.where(obs[1, :, None], faces[1], bad[1]), obs[1], noise[1])    # only the ignored one
        torch.cuda.synchronize()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            st.step_rows(_frame(data, 26), bad[2], obs[2], noise[2])
        assert st.frame_precision == 9
    with m.open_stream(_seed(data, 24)) as st:
        st.step_rows(_frame(data, 24), bad[0], obs[0], noise[0])
        st.step_rows(_frame(data, 25), bad[1], obs[1], noise[1])
        torch.cuda.synchronize()                      # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            st.step_rows(_frame(data, 26), bad[2], obs[2], noise[2])
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out, nll = _rows_run(st, data, bad, noise, obs, 3, N)
        clean = [b for b in range(B) if b != 3]
        assert torch.isfinite(out[:, clean]).all() and torch.isfinite(nll[:, clean]).all()
        assert len(st._rows_graphs) == 2              # one per per-frame arithmetic met


@pytest.mark.parametrize("name", FIXTURES)
def test_mixed_sessions_against_the_oracle(name, gpu_device):
    """The (B, N, C) sequence a mixed session produced, scored teacher-forced by the fp64 oracle: step_rows's nll agrees within the NLL
    gate for observed and generated frames alike. Then generation after a mixed prefix against a pure session that observed that
    prefix (which tests/test_gpu_stream_observe.py holds against inference() at the same gate)."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    noise = fx.get("infer/noise", torch.float32).to(gpu_device)
    given = fx.get("infer/out", torch.float32).to(gpu_device).transpose(0, 1).contiguous()       # (N, B, C)
    N, B = noise.shape[0], noise.shape[1]
    obs = _schedule(B, N, 23).to(gpu_device)
    split = max(1, N // 2)
    tail = obs.clone()
    tail[split:] = False
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            got = [st.step_rows(_frame(data, fx.start + n), given[n], obs[n], noise[n]) for n in range(N)]
        out, nll = torch.stack([a for a, _ in got], 1), torch.stack([q for _, q in got])
        _, expected = fixture_expected(fx, out.cpu())
        e_obs = max_rel(nll[obs], expected[obs.cpu()], floor=1.0) if obs.any() else 0.0
        e_gen = max_rel(nll[~obs], expected[~obs.cpu()], floor=1.0) if (~obs).any() else 0.0
        report("%s step_rows (%s): NLL max rel err vs fp64 oracle: observed frames %.3e, generated frames %.3e"
               % (name, precision, e_obs, e_gen))
        assert e_obs < NLL_GATE and e_gen < NLL_GATE, (precision, e_obs, e_gen)
        with m.open_stream(_seed(data, fx.start)) as st:
            mixed = [st.step_rows(_frame(data, fx.start + n), given[n], tail[n], noise[n])[0] for n in range(N)]
        with m.open_stream(_seed(data, fx.start)) as st:
            for n in range(split):
                st.observe(_frame(data, fx.start + n), mixed[n])
            pure = [st.step(_frame(data, fx.start + n), noise[n]) for n in range(split, N)]
        err = max((a - b).abs().max().item() for a, b in zip(mixed[split:], pure)) if pure else 0.0
        report("%s step_rows (%s): generation after a mixed prefix of %d frames vs a session that observed it: max abs diff %.3e"
               % (name, precision, split, err))
        assert err < FRAME_GATE, (precision, err)


def test_steady_state_step_rows_do_not_synchronise(gpu_device):
    B, N = 24, 10
    m, data, noise, faces = _final_case(gpu_device, B, N)
    obs = _schedule(B, N, 29).to(gpu_device)
    frames = [_frame(data, 24 + n) for n in range(N)]
    with m.open_stream(_seed(data, 24)) as st:
        st.step_rows(frames[0], faces[0], obs[0], noise[0])
        st.step_rows(frames[1], faces[1], obs[1], noise[1])      # (a capture synchronises once: step_rows,
        st.step(frames[2], noise[2])                             # the step graph,
        st.observe(frames[3], faces[3])                          # and observe's)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for n in range(4, 7):
                st.step_rows(frames[n], faces[n], obs[n], noise[n])
            st.step(frames[7], noise[7])
            st.step_rows(frames[8], faces[8], obs[8])            # noise drawn by the session
            st.observe(frames[9], faces[9])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 9


def test_step_rows_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    B, N = 24, 5
    m, data, noise, faces = _final_case(gpu_device, B, N)
    obs = _schedule(B, N, 31).to(gpu_device)
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        on_default = _rows_run(st, data, faces, noise, obs)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with m.open_stream(_seed(data, 24)) as st:
            on_side = _rows_run(st, data, faces, noise, obs)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default[0], on_side[0]) and torch.equal(on_default[1], on_side[1])


def test_reset_rows_and_load_rows_between_step_rows_touch_only_the_listed_rows(gpu_device):
    B, N, at = 24, 8, 3
    m, data, noise, faces = _final_case(gpu_device, B, N)
    obs = _schedule(B, N, 37).to(gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        out, nll = _rows_run(st, data, faces, noise, obs)
    listed, others = [2, 17], [b for b in range(B) if b not in (2, 17)]
    seed = {k: v[listed].contiguous() for k, v in _seed(data, 24).items()}
    with m.open_stream(_seed(data, 24)) as st:
        a_out, a_nll = _rows_run(st, data, faces, noise, obs, 0, at)
        st.reset_rows(listed, seed)
        b_out, b_nll = _rows_run(st, data, faces, noise, obs, at, N)
    assert torch.equal(a_out, out[:at]) and torch.equal(a_nll, nll[:at])
    assert torch.equal(b_out[:, others], out[at:, others]) and torch.equal(b_nll[:, others], nll[at:, others])
    assert not torch.equal(b_nll[:, listed], nll[at:, listed])
    # load_rows: the listed rows go back to their state after `at` frames and live frames at .. again; the others carry on
    with m.open_stream(_seed(data, 24)) as st:
        _rows_run(st, data, faces, noise, obs, 0, at)
        saved = st.save_rows(listed)
        c_out, c_nll = _rows_run(st, data, faces, noise, obs, at, at + 2)
        st.load_rows(listed, saved)
        fr = _frame(data, 24 + at + 2)
        for k, v in _frame(data, 24 + at).items():
            fr[k][listed] = v[listed]
        o, f, z = obs[at + 2].clone(), faces[at + 2].clone(), noise[at + 2].clone()
        o[listed], f[listed], z[listed] = obs[at, listed], faces[at, listed], noise[at, listed]
        d_out, d_nll = st.step_rows(fr, f, o, z)
    assert torch.equal(c_out, out[at:at + 2]) and torch.equal(c_nll, nll[at:at + 2])
    assert torch.equal(d_out[others], out[at + 2, others]) and torch.equal(d_nll[others], nll[at + 2, others])
    assert torch.equal(d_out[listed], out[at, listed]) and torch.equal(d_nll[listed], nll[at, listed])


def test_step_rows_is_refused_after_a_parameter_change_and_after_close(gpu_device):
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    frames = fx.get("infer/out", torch.float32).to(gpu_device)
    B = frames.shape[0]
    mask = [b % 2 == 0 for b in range(B)]
    face = frames[:, 0].contiguous()
    st = m.open_stream(_seed(data, fx.start))
    st.step_rows(_frame(data, fx.start), face, mask)
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_rows(_frame(data, fx.start + 1), face, mask)
    st = m.open_stream(_seed(data, fx.start))
    st.step_rows(_frame(data, fx.start), face, mask)
    with pytest.raises(ValueError, match="observed"):
        st.step_rows(_frame(data, fx.start + 1), face, mask + [True])
    with pytest.raises(TypeError, match="observed"):
        st.step_rows(_frame(data, fx.start + 1), face, torch.zeros(B, device=gpu_device))
    with pytest.raises(ValueError, match="face"):
        st.step_rows(_frame(data, fx.start + 1), frames[:, 1], mask)          # not contiguous
    assert st.steps == 1
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.step_rows(_frame(data, fx.start + 1), face, mask)
