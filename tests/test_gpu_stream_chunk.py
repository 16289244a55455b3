"""GPU: a chunk of recorded frames per call (SampleStream.observe_many -> lfi_stream_chunk_in / lfi_flow_score_seq_chunk /
lfi_stream_chunk_out: the conditioning front end once, the forward chain with the frame loop inside one launch): the NLL and the
latents of whole reference clips against the fp64 oracle on every golden fixture, the state a chunk leaves against inference(),
agreement with the per-frame observe() loop down to the row records, split chunks and the per-frame fallback kernels, two batch tiles
at final widths, mixing with step_rows / reset_rows, and the housekeeping (counters, refusals, streams, the range guard).

Gates, all the project's own: NLL max_rel(nll, expected, floor=1.0) < 1e-4; z rel_err < 1e-5; generated frames against inference()
1e-5 absolute (tests/test_gpu_stream_observe.py has the same three)."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, rel_err, report
from sample_nll_expected import fixture_expected
from test_gpu_parity import build, to_dev
from test_gpu_stream import _final_setup, _frame, _seed
from test_gpu_stream_observe import FRAME_GATE, NLL_GATE, Z_GATE, _face, _final_case, _infer_case

pytestmark = pytest.mark.gpu


def _chunk(data, start, first, n):
    """Frames first .. first + n - 1 after the seed of every conditioning modality, (B, n, dim) each."""
    return {k: v[:, start + first:start + first + n].contiguous() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}


def _faces(frames, first, n):
    return frames[:, first:first + n].contiguous()


def _case(name, device):
    fx = Fixture(name)
    m = build(fx, device)
    data, noise, seq_len = _infer_case(fx, device)
    frames = fx.get("infer/out", torch.float32).to(device)
    return fx, m, data, noise, seq_len, frames


def _takes_the_chunk_chain(m, B, n=1):
    """Whether a session of this model runs lfi_flow_score_seq_chunk (1) or falls back to the per-frame kernels (0)."""
    from lets_face_it_amd import _lib
    eng = m.engine
    return eng.L.lfi_flow_score_chunk_ok(_lib.C.byref(eng._flow_dims(B, n)))


def _generate(st, data, noise, start, first, N):
    return torch.stack([st.step(_frame(data, start + n), noise[n]) for n in range(first, N)], 1)


@pytest.mark.parametrize("name", FIXTURES)
def test_one_chunk_scores_the_whole_reference_clip_as_the_oracle_does(name, gpu_device):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    _, expected = fixture_expected(fx)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            nll, z = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True)
            assert st.steps == N and st.replays == 0
            # the new chain, not the fallback; its work area is what the size query says for these frames
            assert _takes_the_chunk_chain(m, fx.B, N) == 1 and st.hist1 >= 1
            assert "chunk_work" in st._chunk_ws and "chunk_frame_work" not in st._chunk_ws
        assert tuple(nll.shape) == (N, fx.B) and nll.dtype == torch.float32 and tuple(z.shape) == (N, fx.B, frames.shape[2])
        err, zerr = max_rel(nll, expected, floor=1.0), rel_err(z, fx.get("infer/noise"))
        report("%s observe_many (%s), %d frames in one call: NLL max rel err vs fp64 oracle %.3e; z rel err vs infer/noise %.3e"
               % (name, precision, N, err, zerr))
        assert err < NLL_GATE and zerr < Z_GATE, (precision, err, zerr)


def _state_after_chunks(m, fx, data, noise, frames, inf, split, tag):
    """Generation after `split` teacher-forced frames, given as one chunk, as two, and as one generated frame + a chunk."""
    N, worst = noise.shape[0], {}
    plans = [("one call", 0, [split])]
    if split >= 2:
        plans.append(("two calls", 0, [split // 2, split - split // 2]))
        plans.append(("a step, then a chunk", 1, [split - 1]))
    for what, stepped, sizes in plans:
        with m.open_stream(_seed(data, fx.start)) as st:
            at = 0
            if stepped:
                st.step(_frame(data, fx.start), noise[0])
                at = 1
            for n in sizes:
                st.observe_many(_chunk(data, fx.start, at, n), _faces(frames, at, n))
                at += n
            assert at == split and st.steps == split
            out = _generate(st, data, noise, fx.start, split, N)
        worst[what] = (out - inf[:, split:]).abs().max().item()
        report("%s (%s): %d teacher-forced frames (%s), then generation: max abs err vs inference() %.3e"
               % (fx.name, tag, split, what, worst[what]))
    return worst


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "tiny_additive", "p1enc", "framenb"))
def test_state_after_a_chunk_carries_generation_as_inference_does(name, gpu_device):
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    N, Ks = noise.shape[0], m.spec.Ks
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        for split in sorted({1, 2, min(Ks + 1, N - 1), N - 1}):
            worst = _state_after_chunks(m, fx, data, noise, frames, inf, split, precision)
            assert all(v < FRAME_GATE for v in worst.values()), (precision, split, worst)


@pytest.mark.parametrize("name,n", (("tiny", 2), ("tiny", 9), ("mid", 10)))
def test_chunk_agrees_with_the_per_frame_calls_down_to_the_row_records(name, n, gpu_device):
    """n below and above the history (tiny: 4 frames) and against a long one (mid: 24): the windows a chunk leaves are copies of the
    same values - bit for bit - and h / c agree to the generated-frame gate."""
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    m.precision = "bf16x3"
    rows = list(range(fx.B))
    with m.open_stream(_seed(data, fx.start)) as one, m.open_stream(_seed(data, fx.start)) as many:
        got = [one.observe(_frame(data, fx.start + i), _face(frames, i), return_z=True) for i in range(n)]
        nll, z = many.observe_many(_chunk(data, fx.start, 0, n), _faces(frames, 0, n), return_z=True)
        a, b = one.save_rows(rows), many.save_rows(rows)
        sig = many.row_signature
    err = max_rel(nll, torch.stack([q for q, _ in got]), floor=1.0)
    zerr = rel_err(z, torch.stack([v for _, v in got]))
    nwin = sum(h * d for _, h, d in sig[5]) + (sig[6] + 1) * sig[0]
    serr = (a.data - b.data).abs().max().item()
    report("%s, %d frames, observe_many vs %d observe() calls: NLL max rel diff %.3e, z rel diff %.3e, row records max abs diff %.3e"
           % (name, n, n, err, zerr, serr))
    assert a.signature == b.signature
    assert err < NLL_GATE and zerr < Z_GATE and serr < FRAME_GATE
    assert torch.equal(a.data[:, :nwin], b.data[:, :nwin])
    if sig[4]:      # the frame counter, the record's last float
        assert torch.equal(a.data[:, -1], b.data[:, -1])


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_a_chunk_split_into_launches_of_three_frames_is_bit_identical(name, gpu_device, monkeypatch):
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            whole = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True)
        monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "3")
        with m.open_stream(_seed(data, fx.start)) as st:
            assert st._chunk_cap() == 3 and N > 3
            split = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True)
            assert st.steps == N
        monkeypatch.delenv("LFI_OBSERVE_CHUNK_FRAMES")
        assert torch.equal(whole[0], split[0]) and torch.equal(whole[1], split[1]), precision


@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1"))
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_chunks_on_the_per_frame_kernels(name, switch, gpu_device, monkeypatch):
    """The session's fallback (lfi_flow_score_seq_from with nframes = n on the chunk's sequences): the same Python path on the
    existing kernels, the gates of the first two tests at both precisions and every split of the second."""
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    _, expected = fixture_expected(fx)
    N, Ks = noise.shape[0], m.spec.Ks
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        assert _takes_the_chunk_chain(m, fx.B, N) == 1
        with monkeypatch.context() as mp:
            mp.setenv(*switch.split("="))
            assert _takes_the_chunk_chain(m, fx.B, N) == 0
            with m.open_stream(_seed(data, fx.start)) as st:
                nll, z = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True)
                assert "chunk_frame_work" in st._chunk_ws and "chunk_work" not in st._chunk_ws
            err, zerr = max_rel(nll, expected, floor=1.0), rel_err(z, fx.get("infer/noise"))
            report("%s observe_many (%s, %s): NLL max rel err vs fp64 oracle %.3e; z rel err %.3e" % (name, switch, precision, err, zerr))
            assert err < NLL_GATE and zerr < Z_GATE, precision
            for split in sorted({1, 2, min(Ks + 1, N - 1), N - 1}):
                worst = _state_after_chunks(m, fx, data, noise, frames, inf, split, "%s, %s" % (switch, precision))
                assert all(v < FRAME_GATE for v in worst.values()), (precision, split, worst)


def test_injected_masks_reach_the_frames_they_belong_to(gpu_device, monkeypatch):
    """Train mode with injected (N, B, hist) masks: frame steps + i of the masks goes to frame i of a chunk - after a per-frame call,
    across two chunks and across the launches of a split chunk - as the observe() loop gives frame n's row to step n."""
    fx = Fixture("p1enc")
    m = build(fx, gpu_device, train=True)
    data, noise, _ = _infer_case(fx, gpu_device)
    frames = fx.get("infer/out", torch.float32).to(gpu_device)
    N, B = noise.shape[0], noise.shape[1]
    g = torch.Generator().manual_seed(5)
    m.injected_masks = {e.name: ((torch.rand(N, B, e.hist, generator=g) < 0.6).float() / 0.6)
                        for e in m.spec.encoders if e.dropout > 0 and e.name != "p1_face"}
    assert m.injected_masks
    m.precision = "bf16x3"
    with m.open_stream(_seed(data, fx.start)) as st:
        want = torch.stack([st.observe(_frame(data, fx.start + n), _face(frames, n)) for n in range(N)])
    unmasked = m.injected_masks
    m.injected_masks = {k: torch.ones_like(v) for k, v in unmasked.items()}
    with m.open_stream(_seed(data, fx.start)) as st:
        plain = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N))
    m.injected_masks = unmasked
    assert max_rel(plain, want, floor=1.0) > 10 * NLL_GATE          # the masks matter: a wrong frame's row would show
    for cap in (None, "3"):
        if cap:
            monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", cap)
        with m.open_stream(_seed(data, fx.start)) as st:
            got = [st.observe(_frame(data, fx.start), _face(frames, 0)).unsqueeze(0),
                   st.observe_many(_chunk(data, fx.start, 1, 7), _faces(frames, 1, 7)),
                   st.observe_many(_chunk(data, fx.start, 8, N - 8), _faces(frames, 8, N - 8))]
            with pytest.raises(ValueError, match="holds %d frames" % N):
                st.observe_many(_chunk(data, fx.start, 0, 1), _faces(frames, 0, 1))      # beyond the masks: refused, nothing moved
            assert st.steps == N
        err = max_rel(torch.cat(got), want, floor=1.0)
        report("p1enc, injected dropout masks, observe / observe_many x 2 (frames per launch: %s) vs the observe() loop: NLL max rel "
               "diff %.3e" % (cap or "all", err))
        assert err < NLL_GATE


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_two_batch_tiles_at_final_widths(precision, gpu_device):
    """B = 20: two 16-row tiles, the second partial. A session's own generated frames, observed as chunks, score what it reported."""
    N, split = 8, 5
    m, data, noise, ref, ref_nll = _final_case(gpu_device, 20, N, precision)
    with m.open_stream(_seed(data, 24)) as st:
        nll = st.observe_many(_chunk(data, 24, 0, N), _faces(ref, 0, N))
    with m.open_stream(_seed(data, 24)) as st:
        head = st.observe_many(_chunk(data, 24, 0, split), _faces(ref, 0, split))
        out = _generate(st, data, noise, 24, split, N)
    err, herr = max_rel(nll, ref_nll, floor=1.0), max_rel(head, ref_nll[:split], floor=1.0)
    ferr = (out - ref[:, split:]).abs().max().item()
    report("final widths (%s), B = 20: observe_many over the session's own %d frames, NLL max rel diff vs what it reported %.3e "
           "(first %d: %.3e); generation afterwards max abs err %.3e" % (precision, N, err, split, herr, ferr))
    assert err < NLL_GATE and herr < NLL_GATE and ferr < FRAME_GATE


@pytest.mark.parametrize("name", ("tiny", "framenb"))
def test_chunks_mix_with_step_rows_and_reset_rows(name, gpu_device):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    _, expected = fixture_expected(fx)
    N, at, r = noise.shape[0], 3, 1
    m.precision = "bf16x3"
    # a chunk, one step_rows frame in which every row observes, a chunk
    with m.open_stream(_seed(data, fx.start)) as st:
        a = st.observe_many(_chunk(data, fx.start, 0, at), _faces(frames, 0, at))
        _, b = st.step_rows(_frame(data, fx.start + at), _face(frames, at), [True] * fx.B, noise[at])
        c = st.observe_many(_chunk(data, fx.start, at + 1, N - at - 1), _faces(frames, at + 1, N - at - 1))
        assert st.steps == N
    err = max_rel(torch.cat([a, b.unsqueeze(0), c]), expected, floor=1.0)
    report("%s: observe_many, step_rows, observe_many: NLL max rel err vs fp64 oracle %.3e" % (name, err))
    assert err < NLL_GATE
    # row r reseeded between two chunks lives its sequence again from the start: a fresh session's NLL (and, with the frame counter
    # among the features, its own count), while the other rows carry on
    with m.open_stream(_seed(data, fx.start)) as st:
        st.observe_many(_chunk(data, fx.start, 0, at), _faces(frames, 0, at))
        st.reset_rows([r], {k: v[r:r + 1].contiguous() for k, v in _seed(data, fx.start).items()})
        n2 = N - at
        fr, face = _chunk(data, fx.start, at, n2), _faces(frames, at, n2)
        for k, v in _chunk(data, fx.start, 0, n2).items():
            fr[k][r] = v[r]
        face[r] = frames[r, :n2]
        got = st.observe_many(fr, face)
    others = [b for b in range(fx.B) if b != r]
    err_r = max_rel(got[:, r], expected[:n2, r], floor=1.0)
    err_o = max_rel(got[:, others], expected[at:, others], floor=1.0)
    report("%s: NLL of a row reseeded between two chunks vs the oracle on its sequence %.3e; the other rows %.3e" % (name, err_r, err_o))
    assert err_r < NLL_GATE and err_o < NLL_GATE


def test_counters_refusals_and_a_stale_session(gpu_device):
    fx, m, data, noise, _, frames = _case("tiny", gpu_device)
    N = noise.shape[0]
    st = m.open_stream(_seed(data, fx.start))
    st.observe(_frame(data, fx.start), _face(frames, 0))
    st.observe(_frame(data, fx.start + 1), _face(frames, 1))
    assert (st.steps, st.replays) == (2, 1)
    st.observe_many(_chunk(data, fx.start, 2, 4), _faces(frames, 2, 4))
    assert (st.steps, st.replays) == (6, 1)
    graphs = dict(st._observe_graphs)
    st.observe(_frame(data, fx.start + 6), _face(frames, 6))            # the per-frame graph still stands
    assert (st.steps, st.replays) == (7, 2) and st._observe_graphs == graphs
    before = st.save_rows(list(range(fx.B))).data.clone()
    with pytest.raises(ValueError, match="faces"):
        st.observe_many(_chunk(data, fx.start, 7, 2), frames[:, 7:9, :3].contiguous())
    with pytest.raises(ValueError, match=r"n=2"):
        st.observe_many(_chunk(data, fx.start, 7, 3), _faces(frames, 7, 2))
    with pytest.raises(ValueError, match="faces"):
        st.observe_many(_chunk(data, fx.start, 7, 2), frames[:, 7:9])   # not contiguous
    with pytest.raises(TypeError, match="return_z"):
        st.observe_many(_chunk(data, fx.start, 7, 2), _faces(frames, 7, 2), return_z=1)
    assert st.steps == 7 and torch.equal(st.save_rows(list(range(fx.B))).data, before)
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.observe_many(_chunk(data, fx.start, 7, 2), _faces(frames, 7, 2))
    assert st.steps == 7
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.observe_many(_chunk(data, fx.start, 7, 2), _faces(frames, 7, 2))
    assert N > 9


def test_chunk_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    m, data, noise, ref, _ = _final_case(gpu_device, 8, 5)
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        on_default = st.observe_many(_chunk(data, 24, 0, 5), _faces(ref, 0, 5), return_z=True)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with m.open_stream(_seed(data, 24)) as st:
            on_side = st.observe_many(_chunk(data, 24, 0, 5), _faces(ref, 0, 5), return_z=True)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default[0], on_side[0]) and torch.equal(on_default[1], on_side[1])


def test_a_face_beyond_the_fp16_range_in_a_chunk_trips_the_guard(gpu_device):
    """As tests/test_gpu_stream_observe.py shows for observe(): the warning at the next call, then the range-free arithmetic (5); what
    the session reports afterwards is what a session opened at 5 reports, in the rows that never saw fp16 pieces out of range."""
    N = 10
    m, data, noise, ref, _ = _final_case(gpu_device, 8, N)
    bad = ref.clone()
    bad[0, 2, 5] = 1.0e5                           # row 0, inside the first chunk: observed with fp16 pieces, trips the guard
    bad[3, 6, 7] = -3.0e5                          # row 3, observed after the fallback
    eng = m._ensure_engine(gpu_device)
    eng.sample_frame_precision = 5
    try:
        with m.open_stream(_seed(data, 24)) as st:
            assert st.frame_precision == 5
            want = st.observe_many(_chunk(data, 24, 0, N), _faces(bad, 0, N))
    finally:
        eng.sample_frame_precision = None
    assert torch.isfinite(want).all()
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        got = [st.observe_many(_chunk(data, 24, 0, 4), _faces(bad, 0, 4))]
        torch.cuda.synchronize()                   # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            got.append(st.observe_many(_chunk(data, 24, 4, 3), _faces(bad, 4, 3)))
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got.append(st.observe_many(_chunk(data, 24, 7, N - 7), _faces(bad, 7, N - 7)))
    got = torch.cat(got)
    clean = [b for b in range(8) if b != 0]
    assert torch.isfinite(got[4:, clean]).all()
    err = max_rel(got[4:, clean], want[4:, clean], floor=1.0)
    report("final widths: NLL of chunks after the range guard's fallback (an out-of-range face among them) vs a session opened with "
           "six bf16 products: max rel diff %.3e" % err)
    assert err < NLL_GATE
    assert float(got[6, 3]) > 1e6                   # the out-of-range face is scored, not dropped
