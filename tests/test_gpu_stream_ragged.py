"""GPU: ragged chunks (SampleStream.observe_many with lengths -> lfi_stream_chunk_in_rows / lfi_flow_score_seq_chunk_rows /
lfi_stream_chunk_out_rows): every row's NLL and latents against the fp64 oracle up to its own length and exact zeros behind it, the
row records against dense chunks of each length bit for bit, generation afterwards against inference(), two batch tiles at final
widths, all lengths n / all lengths 0, split rounds, the per-frame fallback, padding that is never read, injected masks, the
housekeeping and the two window launches through the C ABI.

Gates, the project's own (tests/test_gpu_stream_observe.py): NLL max_rel(nll, expected, floor=1.0) < 1e-4; z rel_err < 1e-5; generated
frames and h / c 1e-5 absolute. Everything called "bit for bit" is torch.equal.

The golden clips are 22 frames (B = 4) and, `mid`, 10 frames (B = 8, 24-frame history): lengths below, at and above a 24-frame history
do not fit `mid`, which takes lengths inside its 10 frames, and run on the final-widths model with a 26-frame clip instead."""
import warnings

import pytest
import torch

from helpers import Fixture, max_rel, rel_err, report
from sample_nll_expected import fixture_expected
from test_gpu_parity import build
from test_gpu_stream import _frame, _seed
from test_gpu_stream_chunk import _case, _chunk, _faces, _takes_the_chunk_chain
from test_gpu_stream_observe import FRAME_GATE, NLL_GATE, Z_GATE, _face, _final_case, _infer_case

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "bf16x3")
_EXPECTED = {}


def _expected(fx):
    """The fp64 oracle's (z, nll) of the fixture's clip: computed once per fixture, shared, never written."""
    if fx.name not in _EXPECTED:
        _EXPECTED[fx.name] = fixture_expected(fx)
    return _EXPECTED[fx.name]


def _lengths(B, n):
    """B = 4: full, none, below the 4-frame history, one. B = 8 (mid): those, and the lengths next to them."""
    return [n, 0, 3, 1] if B == 4 else [n, 0, 3, 4, 5, 1, 2, n - 1]


def _rows(st):
    return st.save_rows(list(range(st.B))).data.clone()


def _nwin(sig):
    """Floats of a row record in front of h: the conditioning windows and the faces window."""
    return sum(h * d for _, h, d in sig[5]) + (sig[6] + 1) * sig[0]


def _check_outputs(tag, nll, z, lens, want_nll, want_z):
    """Row r up to its length under the gates, exact zeros behind it -> the worst errors."""
    worst = [0.0, 0.0]
    for r, L in enumerate(lens):
        assert torch.count_nonzero(nll[L:, r]) == 0 and torch.count_nonzero(z[L:, r]) == 0, (tag, r, L)
        if L:
            worst[0] = max(worst[0], max_rel(nll[:L, r], want_nll[:L, r], floor=1.0))
            worst[1] = max(worst[1], rel_err(z[:L, r], want_z[:L, r]))
    report("%s, lengths %s: NLL max rel err %.3e, z rel err %.3e, exact zeros behind each length" % (tag, lens, worst[0], worst[1]))
    assert worst[0] < NLL_GATE and worst[1] < Z_GATE, (tag, worst)
    return worst


# ---- 1. the oracle, per row
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "tiny_additive", "p1enc", "framenb", "mid"))
def test_every_row_is_scored_up_to_its_own_length_as_the_oracle_scores_it(name, gpu_device):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    _, expected = _expected(fx)
    N = noise.shape[0]
    lens = _lengths(fx.B, N)
    for precision in PRECISIONS:
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            nll, z = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True, lengths=lens)
            assert st.steps == N and st.replays == 0
            assert _takes_the_chunk_chain(m, fx.B, N) == 1 and st.hist1 >= 1
            assert "chunk_work" in st._chunk_ws and "chunk_frame_work" not in st._chunk_ws
        assert tuple(nll.shape) == (N, fx.B) and nll.dtype == torch.float32 and tuple(z.shape) == (N, fx.B, frames.shape[2])
        _check_outputs("%s ragged observe_many (%s)" % (name, precision), nll, z, lens, expected, fx.get("infer/noise"))


# ---- 2. the state, bit for bit
def _dense_records(m, seed, lead, chunk_of, lens):
    """{L: row records} of sessions that take the `lead` frames and then a dense chunk of L frames (nothing more for L = 0)."""
    out = {}
    for L in sorted(set(lens)):
        with m.open_stream(seed) as st:
            if lead:
                st.observe_many(*chunk_of(0, lead))
            if L:
                st.observe_many(*chunk_of(lead, L))
            out[L] = _rows(st)
    return out


def _records_match(tag, got, want, lens, sig=None, gate=None):
    """Row r of `got` against row r of the dense session of its length: bit for bit, or (gate: the fallback) windows and counter
    bit for bit and h / c under the gate."""
    worst = 0.0
    for r, L in enumerate(lens):
        if gate is None:
            assert torch.equal(got[r], want[L][r]), (tag, r, L, (got[r] - want[L][r]).abs().max().item())
            continue
        nwin = _nwin(sig)
        assert torch.equal(got[r, :nwin], want[L][r, :nwin]), (tag, r, L)
        if sig[4]:
            assert torch.equal(got[r, -1], want[L][r, -1]), (tag, r, L)
        worst = max(worst, (got[r] - want[L][r]).abs().max().item())
    if gate is not None:
        report("%s: row records vs dense chunks of each length, windows and counter bit for bit, h / c max abs diff %.3e" % (tag, worst))
        assert worst < gate, (tag, worst)


@pytest.mark.parametrize("name", ("tiny", "tiny_lstm", "framenb", "mid"))
def test_a_ragged_chunk_leaves_each_row_where_a_dense_chunk_of_its_length_leaves_it(name, gpu_device):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    N = noise.shape[0]
    seed = _seed(data, fx.start)

    def chunk_of(first, n):
        return _chunk(data, fx.start, first, n), _faces(frames, first, n)
    for precision in PRECISIONS:
        m.precision = precision
        for lead in (2, 0):         # a running session; one that has not stepped (length 0: a fresh session's record)
            n = N - lead
            lens = _lengths(fx.B, n)
            with m.open_stream(seed) as st:
                if lead:
                    st.observe_many(*chunk_of(0, lead))
                st.observe_many(*chunk_of(lead, n), lengths=lens)
                assert st.steps == N
                got = _rows(st)
            want = _dense_records(m, seed, lead, chunk_of, lens)
            _records_match("%s (%s), %d frames first" % (name, precision, lead), got, want, lens)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lengths_below_at_and_above_a_24_frame_history_at_final_widths(precision, gpu_device):
    """The lengths around the history that mid's 10-frame clip has no room for: 23, 24 and 25 frames into 24-frame windows."""
    N = 26
    lens = [N, 0, 23, 24, 25, 1, 2, N - 1]
    m, data, noise, ref, ref_nll = _final_case(gpu_device, 8, N, precision)
    seed = _seed(data, 24)

    def chunk_of(first, n):
        return _chunk(data, 24, first, n), _faces(ref, first, n)
    with m.open_stream(seed) as st:
        nll = st.observe_many(*chunk_of(0, N), lengths=lens)
        got = _rows(st)
    for r, L in enumerate(lens):
        assert torch.count_nonzero(nll[L:, r]) == 0
    err = max(max_rel(nll[:L, r], ref_nll[:L, r], floor=1.0) for r, L in enumerate(lens) if L)
    report("final widths (%s), B = 8, lengths %s: NLL max rel diff vs what the generating session reported %.3e" % (precision, lens, err))
    assert err < NLL_GATE
    _records_match("final widths (%s)" % precision, got, _dense_records(m, seed, 0, chunk_of, lens), lens)


# ---- 3. generation afterwards
@pytest.mark.parametrize("name", ("tiny", "p1enc"))
def test_generation_after_a_ragged_chunk_continues_each_row_as_inference_does(name, gpu_device):
    fx, m, data, noise, seq_len, frames = _case(name, gpu_device)
    lens, G = [5, 0, 3, 1], 6
    rows = torch.arange(fx.B, device=gpu_device)
    for precision in PRECISIONS:
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        with m.open_stream(_seed(data, fx.start)) as st:
            st.observe_many(_chunk(data, fx.start, 0, 5), _faces(frames, 0, 5), lengths=lens)
            out = []
            for j in range(G):      # row r is at its own frame lens[r] + j
                at = torch.tensor([L + j for L in lens], device=gpu_device)
                frame = {k: v[rows, fx.start + at].contiguous() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}
                out.append(st.step(frame, noise[at, rows].contiguous()))
        out = torch.stack(out, 1)
        want = torch.stack([inf[r, L:L + G] for r, L in enumerate(lens)])
        err = (out - want).abs().max().item()
        report("%s (%s): ragged chunk %s, then %d generated frames per row: max abs err vs inference() %.3e" % (name, precision, lens, G, err))
        assert err < FRAME_GATE, (precision, err)


# ---- 4. final widths, two tiles
@pytest.mark.parametrize("which", ("second tile empty", "first tile empty"))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_batch_tiles_at_final_widths_one_of_them_empty(precision, which, gpu_device):
    N = 8
    lens = [8, 5, 0, 1, 3, 8, 2, 0, 6, 4, 8, 1, 7, 0, 5, 8] + [0] * 4 if which == "second tile empty" else [0] * 16 + [8, 3, 0, 1]
    m, data, noise, ref, ref_nll = _final_case(gpu_device, 20, N, precision)
    with m.open_stream(_seed(data, 24)) as st:
        before = _rows(st)
        nll = st.observe_many(_chunk(data, 24, 0, N), _faces(ref, 0, N), lengths=lens)
        after = _rows(st)
    worst = 0.0
    for r, L in enumerate(lens):
        assert torch.count_nonzero(nll[L:, r]) == 0
        if L:
            worst = max(worst, max_rel(nll[:L, r], ref_nll[:L, r], floor=1.0))
            assert not torch.equal(after[r], before[r])
        else:
            assert torch.equal(after[r], before[r]), r
    report("final widths (%s), B = 20, %s: NLL of live entries max rel diff vs what the generating session reported %.3e; rows of "
           "length 0 untouched bit for bit" % (precision, which, worst))
    assert worst < NLL_GATE


# ---- 5. all lengths n, all lengths 0
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_all_lengths_n_is_the_dense_call_and_all_lengths_0_moves_nothing(name, gpu_device):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    N = noise.shape[0]
    for precision in PRECISIONS:
        m.precision = precision
        for lead in (0, 2):
            n = N - lead
            got = []
            for lengths in (None, [n] * fx.B):
                with m.open_stream(_seed(data, fx.start)) as st:
                    if lead:
                        st.observe_many(_chunk(data, fx.start, 0, lead), _faces(frames, 0, lead))
                    out = st.observe_many(_chunk(data, fx.start, lead, n), _faces(frames, lead, n), return_z=True, lengths=lengths)
                    got.append((out[0], out[1], _rows(st)))
            for a, b in zip(*got):
                assert torch.equal(a, b), (precision, lead)
        with m.open_stream(_seed(data, fx.start)) as st:
            st.observe_many(_chunk(data, fx.start, 0, 2), _faces(frames, 0, 2))
            before = _rows(st)
            nll, z = st.observe_many(_chunk(data, fx.start, 2, 5), _faces(frames, 2, 5), return_z=True, lengths=[0] * fx.B)
            assert st.steps == 7 and torch.equal(_rows(st), before)
            assert tuple(nll.shape) == (5, fx.B) and torch.count_nonzero(nll) == 0 and torch.count_nonzero(z) == 0


# ---- 6. split rounds
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_a_ragged_chunk_split_into_rounds_of_three_frames_is_bit_identical(name, gpu_device, monkeypatch):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    N = noise.shape[0]
    lens = [N, 0, 3, 4]             # (3: a length on a round boundary)
    for precision in PRECISIONS:
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            whole = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True, lengths=lens) + (_rows(st),)
        monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "3")
        with m.open_stream(_seed(data, fx.start)) as st:
            assert st._chunk_cap() == 3 and N > 3
            split = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N), return_z=True, lengths=lens) + (_rows(st),)
            assert st.steps == N
        monkeypatch.delenv("LFI_OBSERVE_CHUNK_FRAMES")
        for a, b in zip(whole, split):
            assert torch.equal(a, b), precision


# ---- 7. the fallback
@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1"))
@pytest.mark.parametrize("name", ("tiny", "tiny_lstm"))
def test_ragged_chunks_on_the_per_frame_kernels(name, switch, gpu_device, monkeypatch):
    fx, m, data, noise, _, frames = _case(name, gpu_device)
    _, expected = _expected(fx)
    N = noise.shape[0]
    seed = _seed(data, fx.start)

    def chunk_of(first, n):
        return _chunk(data, fx.start, first, n), _faces(frames, first, n)
    m._ensure_engine(gpu_device)
    for precision in PRECISIONS:
        m.precision = precision
        assert _takes_the_chunk_chain(m, fx.B, N) == 1
        with monkeypatch.context() as mp:
            mp.setenv(*switch.split("="))
            assert _takes_the_chunk_chain(m, fx.B, N) == 0
            lens = _lengths(fx.B, N)
            with m.open_stream(seed) as st:
                nll, z = st.observe_many(*chunk_of(0, N), return_z=True, lengths=lens)
                assert "chunk_frame_work" in st._chunk_ws and "chunk_work" not in st._chunk_ws
            _check_outputs("%s ragged observe_many (%s, %s)" % (name, switch, precision), nll, z, lens, expected, fx.get("infer/noise"))
            lens = _lengths(fx.B, N - 2)
            with m.open_stream(seed) as st:
                st.observe_many(*chunk_of(0, 2))
                st.observe_many(*chunk_of(2, N - 2), lengths=lens)
                got, sig = _rows(st), st.row_signature
            want = _dense_records(m, seed, 2, chunk_of, lens)
            _records_match("%s (%s, %s)" % (name, switch, precision), got, want, lens, sig, FRAME_GATE)


# ---- 8. padding is not read
def test_what_lies_behind_a_rows_length_is_never_read(gpu_device):
    N = 8
    lens = [N, 0, 3, 1, 5, 2, N, 4]
    m, data, noise, ref, _ = _final_case(gpu_device, 8, N)
    live = (torch.arange(N, device=gpu_device).unsqueeze(0) < torch.tensor(lens, device=gpu_device).unsqueeze(1)).unsqueeze(2)   # (B, N, 1)

    def run(pad, poke=None):
        """A ragged call with `pad` behind every length (poke: + that value inside a live frame), then a second call."""
        fr = {k: torch.where(live, v, torch.full_like(v, pad)) for k, v in _chunk(data, 24, 0, N).items()}
        faces = torch.where(live, _faces(ref, 0, N), torch.full_like(ref[:, :N], pad))
        if poke is not None:
            faces[4, 2, 7] = poke
        with m.open_stream(_seed(data, 24)) as st:
            assert st.frame_precision == 9
            nll, z = st.observe_many(fr, faces.contiguous(), return_z=True, lengths=lens)
            rows = _rows(st)
            torch.cuda.synchronize()        # (the guard's copy has landed: the next call reads it)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                st.observe_many(fr, faces.contiguous(), lengths=[0] * 8)
            return nll, z, rows, [w for w in caught if issubclass(w.category, RuntimeWarning)], st.frame_precision
    zero = run(0.0)
    assert not zero[3] and zero[4] == 9
    assert torch.isfinite(zero[0]).all() and torch.isfinite(zero[1]).all() and torch.isfinite(zero[2]).all()
    for pad in (float("nan"), 1.0e5):
        got = run(pad)
        assert all(torch.equal(a, b) for a, b in zip(zero[:3], got[:3])), pad
        assert not got[3] and got[4] == 9, pad
    poked = run(0.0, poke=1.0e5)            # the same value where it IS read trips the guard
    assert len(poked[3]) == 1 and "six bf16 products" in str(poked[3][0].message) and poked[4] == 5


# ---- 9. injected masks
def test_injected_masks_reach_the_frames_of_a_ragged_chunk(gpu_device):
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
    masks = m.injected_masks
    m.injected_masks = {k: torch.ones_like(v) for k, v in masks.items()}
    with m.open_stream(_seed(data, fx.start)) as st:
        plain = st.observe_many(_chunk(data, fx.start, 0, N), _faces(frames, 0, N))
    m.injected_masks = masks
    assert max_rel(plain, want, floor=1.0) > 10 * NLL_GATE          # the masks matter: a wrong frame's row would show
    first = 2
    lens = [N - first, 0, 3, 1]
    with m.open_stream(_seed(data, fx.start)) as st:
        st.observe_many(_chunk(data, fx.start, 0, first), _faces(frames, 0, first))
        got = st.observe_many(_chunk(data, fx.start, first, N - first), _faces(frames, first, N - first), lengths=lens)
        assert st.steps == N
    err = max(max_rel(got[:L, r], want[first:first + L, r], floor=1.0) for r, L in enumerate(lens) if L)
    report("p1enc, injected dropout masks, a ragged chunk %s from frame %d vs the observe() loop: NLL max rel diff %.3e" % (lens, first, err))
    assert err < NLL_GATE
    assert all(torch.count_nonzero(got[L:, r]) == 0 for r, L in enumerate(lens))


# ---- 10. housekeeping
def test_refusals_counters_and_the_per_frame_graph(gpu_device):
    fx, m, data, noise, _, frames = _case("tiny", gpu_device)
    with m.open_stream(_seed(data, fx.start)) as st:
        st.observe(_frame(data, fx.start), _face(frames, 0))
        st.observe(_frame(data, fx.start + 1), _face(frames, 1))
        assert (st.steps, st.replays) == (2, 1)
        before = _rows(st)
        fr, fa = _chunk(data, fx.start, 2, 4), _faces(frames, 2, 4)
        for bad in ([4, 0, 3], [4, 0, 3, 5], [4, 0, 3, -1], [True, False, True, True], [1.0, 2.0, 3.0, 4.0],
                    torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([[4, 0, 3, 1]]), torch.tensor([4, 0, 3, 1], device=gpu_device)):
            with pytest.raises((ValueError, TypeError), match="lengths"):
                st.observe_many(fr, fa, lengths=bad)
        assert (st.steps, st.replays) == (2, 1) and torch.equal(_rows(st), before)
        graphs = dict(st._observe_graphs)
        st.observe_many(fr, fa, lengths=torch.tensor([4, 0, 3, 1]))
        assert (st.steps, st.replays) == (6, 1)
        st.observe(_frame(data, fx.start + 6), _face(frames, 6))            # the per-frame graph still stands
        assert (st.steps, st.replays) == (7, 2) and st._observe_graphs == graphs


def test_ragged_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    lens = [5, 0, 3, 1, 4, 2, 5, 0]
    m, data, noise, ref, _ = _final_case(gpu_device, 8, 5)
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        on_default = st.observe_many(_chunk(data, 24, 0, 5), _faces(ref, 0, 5), return_z=True, lengths=lens) + (_rows(st),)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        with m.open_stream(_seed(data, 24)) as st:
            on_side = st.observe_many(_chunk(data, 24, 0, 5), _faces(ref, 0, 5), return_z=True, lengths=lens) + (_rows(st),)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(on_default, on_side))


# ---- 11. the window launches through the C ABI
def test_the_window_launches_against_a_torch_restatement(gpu_device):
    from lets_face_it_amd import _lib
    L, c = _lib.lib(), _lib.C
    B, n, start = 3, 5, 4
    lens = [0, 1, n]
    g = torch.Generator().manual_seed(11)
    shapes = ((3, 5, 0), (start + 1, 6, 1))          # (hist, dim, lead): a conditioning window; the faces window, hist - lead == start
    wins = [torch.randn(B, h, d, generator=g).to(gpu_device) for h, d, _ in shapes]
    srcs = [torch.randn(B, n, d, generator=g) for _, d, _ in shapes]
    for s in srcs:
        for b, v in enumerate(lens):
            s[b, v:] = float("nan")                  # never read
    srcs = [s.to(gpu_device) for s in srcs]
    seqs = [torch.full((B, start + n, d), 7.0, device=gpu_device) for _, d, _ in shapes]
    guard = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    frame_nb = torch.tensor([3.0, 5.0, 7.0], device=gpu_device)
    lengths = torch.tensor(lens, dtype=torch.int32, device=gpu_device)
    k = len(shapes)
    tab = lambda ts: (c.c_void_p * k)(*[t.data_ptr() for t in ts])
    ints = lambda i: (c.c_int * k)(*[s[i] for s in shapes])
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.lfi_stream_chunk_in_rows(B, n, start, k, tab(wins), tab(srcs), tab(seqs), ints(0), ints(1), ints(2), guard.data_ptr(),
                                          lengths.data_ptr(), stream), "lfi_stream_chunk_in_rows")
    amax = 0.0
    for (h, d, lead), win, src, seq in zip(shapes, wins, srcs, seqs):
        want = torch.full_like(seq, 7.0)
        want[:, start - (h - lead):start] = win[:, lead:]
        want[:, start:] = 0.0
        for b, v in enumerate(lens):
            want[b, start:start + v] = src[b, :v]
            if v:
                amax = max(amax, src[b, :v].abs().max().item())
        assert torch.equal(seq, want)
    assert guard.view(torch.float32).item() == amax
    want_wins = [w.clone() for w in wins]
    for (h, d, lead), want, seq in zip(shapes, want_wins, seqs):
        for b, v in enumerate(lens):
            if v:
                want[b] = seq[b, start + v - h:start + v]
    _lib.check(L.lfi_stream_chunk_out_rows(B, n, start, k, tab(wins), tab(seqs), ints(0), ints(1), ints(2), frame_nb.data_ptr(),
                                           lengths.data_ptr(), stream), "lfi_stream_chunk_out_rows")
    for win, want in zip(wins, want_wins):
        assert torch.equal(win, want)
    assert frame_nb.tolist() == [3.0, 5.0 + 2.0, 7.0 + 2.0 * n]
