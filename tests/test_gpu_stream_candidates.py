"""GPU: N candidates per frame of streaming sessions (SampleStream.step_candidates -> lfi_flow_sample_cand_from, the reverse chain over
B * ncand virtual rows that read their parent row's gic and state in place; commit -> lfi_stream_commit_cand; step_best_of): every
candidate bit for bit the step() it stands for, commit leaves the session where that step would, the commit kernel alone on crafted
buffers, graphs, no host wait, the pending rule, the range guard, and the per-step launches and the other cell forms.

Exactness is torch.equal on fp32 bits wherever the one-launch chain runs: rows never mix inside a cell, so a candidate's values do
not depend on which tile row it sits in or who its neighbours are. Where the per-step launches run instead (LFI_SAMPLE_CHAIN=0,
LFI_FLOW_GENERIC=1) the gates are the stream tests' own: frames 1e-5 absolute, NLL max_rel(nll, expected, floor=1.0) < 1e-4."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, report
from lets_face_it_amd import _lib
from test_gpu_parity import build, to_dev
from test_gpu_stream import _final_setup, _frame, _seed

pytestmark = pytest.mark.gpu

NLL_GATE = 1e-4
FRAME_GATE = 1e-5
SHAPES = ((3, 5), (5, 7), (1, 17), (16, 1))     # (B, ncand): one partial tile with parents of unequal share; V = 35, parents straddle
                                                # tile boundaries, 3 rows in the last tile; one parent across two tiles, 1 row in the
                                                # last; one candidate per row (= step)


def _case(m, device, B, N, start, seed=11):
    """Random conditioning and seed for the model `m`: N frames after `start` seed frames."""
    g = torch.Generator().manual_seed(seed)
    data = {"p1_face": torch.randn(B, start, m.spec.C, generator=g)}
    for e in m.spec.encoders:
        if e.name not in ("p1_face", "frame_nb"):
            data[e.name] = torch.randn(B, start + N, e.in_dim, generator=g)
    return to_dev(data, device)


def _noise(B, ncand, C, N, device, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, B, ncand, C, generator=g) * 0.8).to(device)


def _candidates_against_steps(m, data, start, B, ncand, warm, label, exact=True, frames=2):
    """Session S takes `warm` step()s (0: the candidates are the session's very first frame), then `frames` rounds of: save every row,
    step_candidates, and - for every j - a reference session R of the same batch, loaded from the saved rows, takes step(frame,
    noise[:, j]) with return_nll; then S commits a fixed choice and R, loaded again, takes that step, and both records must agree.
    -> the largest differences seen (frames, nll relative)."""
    dev = next(iter(data.values())).device
    Cc, every = m.spec.C, list(range(B))
    noise = _noise(B, ncand, Cc, warm + frames, dev)
    worst_f = worst_q = 0.0
    with m.open_stream(_seed(data, start)) as S, m.open_stream(_seed(data, start), return_nll=True) as R:
        for t in range(warm):
            S.step(_frame(data, start + t), noise[t, :, 0].contiguous())
        for t in range(warm, warm + frames):
            fr, z = _frame(data, start + t), noise[t]
            before = S.save_rows(every)
            faces, nll = S.step_candidates(fr, ncand, z)
            assert tuple(faces.shape) == (B, ncand, Cc) and tuple(nll.shape) == (B, ncand) and nll.dtype == torch.float32
            assert S._pending == ncand and S.steps == t
            if ncand > 1:                               # (different draws: different candidates)
                assert not torch.equal(faces[:, 0], faces[:, 1]) and torch.isfinite(faces).all() and torch.isfinite(nll).all()
            for j in range(ncand):
                if t == 0:
                    R.reset(_seed(data, start))         # (a first frame: zero state, has_prev = 0)
                else:
                    R.load_rows(every, before)
                out, q = R.step(fr, z[:, j].contiguous())
                if exact:
                    assert torch.equal(out, faces[:, j]) and torch.equal(q, nll[:, j]), (label, t, j)
                else:
                    worst_f = max(worst_f, (out - faces[:, j]).abs().max().item())
                    worst_q = max(worst_q, max_rel(nll[:, j], q, floor=1.0))
            choice = [(3 * r + t) % ncand for r in range(B)]
            frame, q, picked = S.commit(choice)
            assert S._pending is None and S.steps == t + 1 and picked.tolist() == choice and picked.dtype == torch.int32
            rows = torch.arange(B, device=dev)
            pick = torch.tensor(choice, device=dev)
            assert torch.equal(frame, faces[rows, pick]) and torch.equal(q, nll[rows, pick])
            if t == 0:
                R.reset(_seed(data, start))
            else:
                R.load_rows(every, before)
            R.step(fr, z[rows, pick].contiguous())
            a, b = S.save_rows(every).data, R.save_rows(every).data
            if exact:
                assert torch.equal(a, b), (label, t)
            else:
                worst_f = max(worst_f, (a - b).abs().max().item())
    if not exact:
        report("%s: candidates on the per-step launches vs step(): frames / records max abs diff %.3e, NLL max rel diff %.3e"
               % (label, worst_f, worst_q))
    return worst_f, worst_q


@pytest.mark.parametrize("name", FIXTURES)
def test_each_candidate_is_the_step_it_stands_for(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    m._ensure_engine(gpu_device)
    B, ncand = 5, 7                                   # V = 35: three tiles, parents straddle their boundaries
    data = _case(m, gpu_device, B, 4, fx.start)
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        _candidates_against_steps(m, data, fx.start, B, ncand, 2, "%s (%s)" % (name, precision))
        _candidates_against_steps(m, data, fx.start, B, ncand, 0, "%s (%s), first frame" % (name, precision), frames=1)


def test_candidates_share_their_rows_dropout_masks_in_train_mode(gpu_device):
    """Train mode with injected masks (one frame's, which repeats for every step): the static part runs once per row, so a row's
    candidates see the masks its step() would."""
    fx = Fixture("p1enc")
    m = build(fx, gpu_device, train=True)
    m._ensure_engine(gpu_device)
    B = 5
    g = torch.Generator().manual_seed(5)
    m.injected_masks = {e.name: ((torch.rand(1, B, e.hist, generator=g) < 0.6).float() / 0.6)
                        for e in m.spec.encoders if e.dropout > 0 and e.name != "p1_face"}
    assert m.injected_masks
    data = _case(m, gpu_device, B, 4, fx.start)
    _candidates_against_steps(m, data, fx.start, B, 7, 2, "p1enc, train mode")


@pytest.mark.parametrize("precision", ("bf16x3", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-n%d" % s)
def test_each_candidate_is_the_step_at_final_model_widths(shape, precision, gpu_device):
    B, ncand = shape
    _, m, _, data, _, _ = _final_setup(gpu_device, B, 4)
    m.precision = precision
    data = to_dev(data, gpu_device)
    _candidates_against_steps(m, data, 24, B, ncand, 2, "final widths %s (%s)" % (shape, precision))
    _candidates_against_steps(m, data, 24, B, ncand, 0, "final widths %s (%s), first frame" % (shape, precision), frames=1)


@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1", "LFI_SAMPLE_WFRAG16=0", "LFI_PIPE_X3=0", "LFI_SAMPLE_FUSED=0"))
def test_candidates_on_the_per_step_launches_and_the_other_cell_forms(switch, gpu_device, monkeypatch):
    B, ncand = 5, 7
    _, m, _, data, _, _ = _final_setup(gpu_device, B, 4)
    m.precision = "bf16x3"
    data = to_dev(data, gpu_device)
    monkeypatch.setenv(*switch.split("="))
    exact = switch not in ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1")
    for warm in (2, 0):
        f, q = _candidates_against_steps(m, data, 24, B, ncand, warm, "final widths (%s), %d warm" % (switch, warm), exact=exact, frames=1)
        assert f < FRAME_GATE and q < NLL_GATE, (switch, warm, f, q)


def _final_case(device, B, ncand, N, precision="bf16x3"):
    _, m, _, data, _, _ = _final_setup(device, B, N)
    m.precision = precision
    return m, to_dev(data, device), _noise(B, ncand, 50, N, device)


@pytest.mark.parametrize("how", ("host", "device", "none"))
def test_commit_leaves_the_session_where_the_step_would(how, gpu_device):
    B, ncand, N = 5, 7, 12
    m, data, noise = _final_case(gpu_device, B, ncand, N)
    every, rows = list(range(B)), torch.arange(B, device=gpu_device)
    plain = noise[:, :, 0].contiguous()
    with m.open_stream(_seed(data, 24)) as S, m.open_stream(_seed(data, 24), return_nll=True) as R:
        S.step(_frame(data, 24), plain[0])
        R.step(_frame(data, 24), plain[0])
        faces, nll = S.step_candidates(_frame(data, 25), ncand, noise[1])
        want = [6, 0, 3, 3, 1]
        if how == "none":
            want = nll.argmin(1).tolist()
            frame, q, picked = S.commit()
        else:
            frame, q, picked = S.commit(want if how == "host" else torch.tensor(want, device=gpu_device))
        assert picked.tolist() == want and picked.dtype == torch.int32
        pick = torch.tensor(want, device=gpu_device)
        assert torch.equal(frame, faces[rows, pick]) and torch.equal(q, nll[rows, pick])
        ref, ref_q = R.step(_frame(data, 25), noise[1][rows, pick].contiguous())
        assert torch.equal(frame, ref) and torch.equal(q, ref_q)
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data) and S.steps == R.steps == 2
        for n in range(2, N):
            assert torch.equal(S.step(_frame(data, 24 + n), plain[n]), R.step(_frame(data, 24 + n), plain[n])[0]), n
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data)
    # a device choice outside the candidates is clamped by the kernel, int64 as int32
    with m.open_stream(_seed(data, 24)) as S:
        faces, nll = S.step_candidates(_frame(data, 24), ncand, noise[0])
        _, _, picked = S.commit(torch.tensor([-3, 0, 6, 7, 1 << 20], device=gpu_device, dtype=torch.int64))
        assert picked.tolist() == [0, 0, 6, 6, 6]


@pytest.mark.parametrize("lstm", (False, True))
def test_commit_kernel_alone_on_crafted_buffers(lstm, gpu_device):
    B, ncand, Ks, H, Cc, hist, G = 5, 3, 2, 7, 6, 4, 11      # G: guard floats around every output buffer
    L, V, dev = _lib.lib(), 5 * 3, gpu_device
    g = torch.Generator().manual_seed(1)
    nan = float("nan")
    cand_frames = torch.randn(V, Cc, generator=g).to(dev)
    cand_h, cand_c = torch.randn(Ks, V, H, generator=g).to(dev), torch.randn(Ks, V, H, generator=g).to(dev)
    # row 0: a tie of the first two; row 1: a NaN in front; row 2: all NaN; row 3: the last wins; row 4: a NaN behind a tie of 0 and 1
    cand_nll = torch.tensor([[2.0, 2.0, 3.0], [nan, 5.0, 4.0], [nan, nan, nan], [9.0, 8.0, -7.0], [1.0, 1.0, nan]]).to(dev)

    def guarded(*shape, dtype=torch.float32):
        n = 1
        for v in shape:
            n *= v
        buf = torch.full((n + 2 * G,), -77.0, device=dev).to(dtype)
        return buf, buf[G:G + n].view(*shape)

    def run(choice):
        bufs = {k: guarded(*shape) for k, shape in (("win", (B, hist, Cc)), ("h", (Ks, B, H)), ("c", (Ks, B, H)), ("frame", (B, Cc)),
                                                    ("nll", (B,)))}
        bufs["pick"] = guarded(B, dtype=torch.int32)
        guard = torch.zeros(1, dtype=torch.int32, device=dev)
        cs = bufs["c"][1] if lstm else None
        rc = L.lfi_stream_commit_cand(B, ncand, Cc, Ks, H, None if choice is None else choice.data_ptr(), cand_frames.data_ptr(),
                                      cand_nll.data_ptr(), cand_h.data_ptr(), cand_c.data_ptr() if lstm else None,
                                      bufs["win"][1].data_ptr(), hist, bufs["h"][1].data_ptr(), None if cs is None else cs.data_ptr(),
                                      bufs["frame"][1].data_ptr(), bufs["nll"][1].data_ptr(), bufs["pick"][1].data_ptr(),
                                      guard.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.lfi_last_error()
        torch.cuda.synchronize()
        return bufs, guard

    for choice, want in ((None, [0, 2, 0, 2, 0]),
                         (torch.tensor([2, -1, 3, 1, 100], dtype=torch.int32, device=dev), [2, 0, 2, 1, 2])):
        bufs, guard = run(choice)
        rows, pick = torch.arange(B, device=dev), torch.tensor(want, device=dev)
        v = rows * ncand + pick
        assert bufs["pick"][1].tolist() == want
        assert torch.equal(bufs["frame"][1], cand_frames[v])
        got, exp = bufs["nll"][1], cand_nll[rows, pick]
        assert torch.equal(got.isnan(), exp.isnan()) and torch.equal(got[~exp.isnan()], exp[~exp.isnan()])
        win = bufs["win"][1]
        assert torch.equal(win[:, hist - 1], cand_frames[v]) and bool((win[:, :hist - 1] == -77.0).all())
        assert torch.equal(bufs["h"][1], cand_h[:, v])
        assert torch.equal(bufs["c"][1], cand_c[:, v]) if lstm else bool((bufs["c"][1] == -77.0).all())
        for name, (whole, _) in bufs.items():
            assert bool((whole[:G] == -77).all()) and bool((whole[-G:] == -77).all()), name
        # the guard word holds max |frame| of what entered the windows, as bits
        assert guard.view(torch.float32).item() == cand_frames[v].abs().max().item()


def test_step_best_of_is_step_candidates_and_commit(gpu_device):
    B, ncand, N = 5, 7, 4
    m, data, noise = _final_case(gpu_device, B, ncand, N)
    every = list(range(B))
    with m.open_stream(_seed(data, 24)) as A, m.open_stream(_seed(data, 24)) as Bs:
        for n in range(N):
            faces, nll = A.step_candidates(_frame(data, 24 + n), ncand, noise[n])
            a = A.commit()
            b = Bs.step_best_of(_frame(data, 24 + n), ncand, noise[n])
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[2].long(), nll.argmin(1))
            assert torch.equal(A.save_rows(every).data, Bs.save_rows(every).data)
        assert A.steps == Bs.steps == N
    # the session's own draws: ncand per call, and a finite result
    with m.open_stream(_seed(data, 24)) as A:
        frame, q, picked = A.step_best_of(_frame(data, 24), 3)
        assert tuple(frame.shape) == (B, 50) and torch.isfinite(frame).all() and torch.isfinite(q).all() and int(picked.max()) < 3


def _best_of_run(st, data, noise, ncand, first, last):
    got = [st.step_best_of(_frame(data, 24 + n), ncand, noise[n][:, :ncand].contiguous()) for n in range(first, last)]
    return [torch.stack([g[i] for g in got]) for i in range(3)]


def test_replay_is_bit_identical_to_eager_and_a_second_ncand_captures_a_second_graph(gpu_device, monkeypatch):
    B, ncand, N = 5, 7, 8
    for precision in ("bf16x3", "f32"):
        m, data, noise = _final_case(gpu_device, B, ncand, N, precision)
        with m.open_stream(_seed(data, 24)) as st:
            a = _best_of_run(st, data, noise, 7, 0, 4)
            assert st.steps == 4 and st.replays == 3 and len(st._cand_graphs) == 1 and st._graph is None
            first = dict(st._cand_graphs)
            b = _best_of_run(st, data, noise, 3, 4, 6)
            assert len(st._cand_graphs) == 2 and st.replays == 5
            c = _best_of_run(st, data, noise, 7, 6, 8)          # the first graph keeps working
            assert len(st._cand_graphs) == 2 and st.replays == 7 and all(st._cand_graphs[k] is g for k, g in first.items())
        monkeypatch.setenv("LFI_NO_GRAPH", "1")
        with m.open_stream(_seed(data, 24)) as st:
            e = _best_of_run(st, data, noise, 7, 0, 4), _best_of_run(st, data, noise, 3, 4, 6), _best_of_run(st, data, noise, 7, 6, 8)
            assert st.replays == 0 and not st._cand_graphs
        monkeypatch.delenv("LFI_NO_GRAPH")
        for got, eager in zip((a, b, c), e):
            assert all(torch.equal(x, y) for x, y in zip(got, eager)), precision


def test_steady_state_candidates_do_not_synchronise(gpu_device):
    B, ncand, N = 5, 7, 9
    m, data, noise = _final_case(gpu_device, B, ncand, N)
    frames = [_frame(data, 24 + n) for n in range(N)]
    pick = torch.tensor([1, 0, 6, 2, 9], device=gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        st.step_best_of(frames[0], ncand, noise[0])
        st.step_best_of(frames[1], ncand, noise[1])              # (a capture synchronises once: the candidates' graph,
        st.step(frames[2], noise[2][:, 0].contiguous())          # and the step graph)
        torch.cuda.set_sync_debug_mode("error")
        try:
            st.step_candidates(frames[3], ncand, noise[3])
            st.commit()                                          # the arg-min on the device
            st.step_candidates(frames[4], ncand, noise[4])
            st.commit(pick)                                      # a device choice
            st.step_best_of(frames[5], ncand)                    # noise drawn by the session
            st.step(frames[6], noise[6][:, 0].contiguous())
            st.step_best_of(frames[7], ncand, noise[7])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 7 and st.steps == 8


def test_pending_candidates_refuse_every_other_call_and_leave_the_session_as_it_was(gpu_device):
    B, ncand, N = 5, 7, 4
    m, data, noise = _final_case(gpu_device, B, ncand, N)
    every, rows = list(range(B)), torch.arange(B, device=gpu_device)
    plain = noise[:, :, 0].contiguous()
    seed = _seed(data, 24)
    face = torch.zeros(B, 50, device=gpu_device)
    with m.open_stream(seed) as S, m.open_stream(seed) as R:
        for st in (S, R):
            st.step(_frame(data, 24), plain[0])
        saved = S.save_rows(every)
        with pytest.raises(RuntimeError, match="without pending candidates"):
            S.commit()
        faces, nll = S.step_candidates(_frame(data, 25), ncand, noise[1])
        fr = _frame(data, 26)
        calls = (lambda: S.step(fr, plain[2]), lambda: S.observe(fr, face), lambda: S.step_rows(fr, face, [True] * B),
                 lambda: S.step_candidates(fr, ncand, noise[2]), lambda: S.step_best_of(fr, ncand),
                 lambda: S.step_many({k: v[:, None].contiguous() for k, v in fr.items()}, plain[2:3]),
                 lambda: S.observe_many({k: v[:, None].contiguous() for k, v in fr.items()}, face[:, None].contiguous()),
                 lambda: S.save_rows(every), lambda: S.load_rows(every, saved), lambda: S.reset_rows([0], {k: v[:1] for k, v in seed.items()}))
        for call in calls:
            with pytest.raises(RuntimeError, match="candidates per row are pending"):
                call()
        assert S._pending == ncand and S.steps == 1
        choice = [2, 2, 0, 6, 5]
        frame, q, _ = S.commit(choice)
        pick = torch.tensor(choice, device=gpu_device)
        assert torch.equal(frame, faces[rows, pick]) and torch.equal(q, nll[rows, pick])
        R.step(_frame(data, 25), noise[1][rows, pick].contiguous())
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data)
        # reset() drops pending candidates and starts the sequence again
        S.step_candidates(_frame(data, 26), ncand, noise[2])
        S.reset(seed)
        R.reset(seed)
        assert S._pending is None and S.steps == 0
        with pytest.raises(RuntimeError, match="without pending candidates"):
            S.commit()
        assert torch.equal(S.step(_frame(data, 24), plain[0]), R.step(_frame(data, 24), plain[0]))
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data)


def test_candidates_are_refused_after_a_parameter_change_and_after_close(gpu_device):
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    B = data["p1_face"].shape[0]
    st = m.open_stream(_seed(data, fx.start))
    st.step_candidates(_frame(data, fx.start), 3)
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.commit()
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step_candidates(_frame(data, fx.start + 1), 3)
    st = m.open_stream(_seed(data, fx.start))
    st.step_best_of(_frame(data, fx.start), 3)
    with pytest.raises(ValueError, match="ncand"):
        st.step_candidates(_frame(data, fx.start + 1), 0)
    with pytest.raises(ValueError, match="noise"):
        st.step_candidates(_frame(data, fx.start + 1), 3, torch.zeros(B, 2, fx.C, device=gpu_device))
    st.step_candidates(_frame(data, fx.start + 1), 3)
    with pytest.raises(ValueError, match="choice"):
        st.commit([0] * (B + 1))
    with pytest.raises(ValueError, match="choice"):
        st.commit(torch.zeros(B, device=gpu_device))            # not an integer tensor
    assert st.steps == 1 and st._pending == 3
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.commit()
    with pytest.raises(RuntimeError, match="closed"):
        st.step_candidates(_frame(data, fx.start + 1), 3)
    assert st._cand is None and not st._cand_graphs


def test_candidate_noise_beyond_the_fp16_range_trips_the_guard_as_steps_does(gpu_device):
    B, ncand, N = 5, 7, 4
    m, data, noise = _final_case(gpu_device, B, ncand, N)
    bad = noise.clone()
    bad[1, 3, 5, 2] = 1.0e5                           # one candidate of one row
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        st.step_best_of(_frame(data, 24), ncand, noise[0])
        torch.cuda.synchronize()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            st.step_best_of(_frame(data, 25), ncand, noise[1])
        assert st.frame_precision == 9
    with m.open_stream(_seed(data, 24)) as st:
        st.step_best_of(_frame(data, 24), ncand, bad[0])
        st.step_best_of(_frame(data, 25), ncand, bad[1])
        torch.cuda.synchronize()                      # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            st.step_best_of(_frame(data, 26), ncand, bad[2])
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            frame, q, _ = st.step_best_of(_frame(data, 27), ncand, bad[3])
        assert torch.isfinite(frame).all() and torch.isfinite(q).all()
        assert len(st._cand_graphs) == 2              # one per per-frame arithmetic met
    # step() itself, the same warning for the same value
    with m.open_stream(_seed(data, 24)) as st:
        st.step(_frame(data, 24), bad[0][:, 0].contiguous())
        st.step(_frame(data, 25), bad[1][:, 5].contiguous())
        torch.cuda.synchronize()
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            st.step(_frame(data, 26), bad[2][:, 0].contiguous())
