"""GPU: keyed sampling noise per conversation in streaming sessions (SeqGlow.open_stream(row_seeds=...)) and in
inference(row_seeds=...). A keyed session is held to an unkeyed one that is GIVEN noise=GlowEngine.row_noise(...) for the same keys
and positions, bit for bit, in every kind of call; positions against the CPU position function; the row, the batch neighbours and
the form of the call do not matter; key and position travel with save_rows / load_rows; reset_rows; inference(); no host wait; an
unkeyed session is unchanged. Every comparison is torch.equal, but keyed inference() against a keyed session: the 1e-5 of
test_stream_matches_fixture_and_inference."""
import io

import pytest
import torch

from helpers import report
from lets_face_it_amd import stream as S
from lets_face_it_amd.engine import StreamRows
from test_gpu_parity import to_dev
from test_gpu_stream import _final_setup, _frame, _run, _seed
from test_gpu_stream_chunk import _chunk
from test_gpu_stream_rows import _conversations, _rows_of

pytestmark = pytest.mark.gpu

B, C_, FRAMES = 8, 50, 11        # C = 50: the last Philox call of a row is partial
KEYS = [2 ** 63 + 5, 1, 2 ** 64 - 1, 0, 12345678901234567, 7, 2 ** 32, 99]
OTHER = [2 ** 62 + r for r in range(8)]


@pytest.fixture(scope="module")
def setup(gpu_device):
    _, m, _, data, noise, seq_len = _final_setup(gpu_device, B, FRAMES)
    return m, to_dev(data, gpu_device), noise.to(gpu_device), seq_len, float(m.hparams.Infer["eps"])


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _graphs(st):
    """What a session shows of its captured graphs: which exist, what they were captured for, how many steps were replays."""
    return (st._graph is not None, st._graph_key, sorted(st._observe_graphs), sorted(st._rows_graphs), sorted(st._cand_graphs), st.replays,
            st.steps)


def _draws(eng, eps, pos, keys=KEYS, **layout):
    """The noise= tensor a keyed session with `keys`, every row at position pos (an int, or one per row), draws for a call."""
    pos = [pos] * len(keys) if isinstance(pos, int) else pos
    return eng.row_noise(eng.row_rng(keys, pos), eps=eps, **layout)


def test_plain_calls_reduce_to_explicit_noise(setup):
    m, data, _, _, eps = setup
    g = torch.Generator().manual_seed(11)
    face = torch.randn(B, 4, C_, generator=g).to(data["p1_face"].device)
    roles = torch.tensor([[True, False, False, True, True, False, True, False], [False, False, True, True, False, True, False, False]])
    with m.open_stream(_seed(data, 24), return_nll=True, row_seeds=KEYS) as K, m.open_stream(_seed(data, 24), return_nll=True) as U:
        eng, p = K.eng, 0
        assert K.rng.dtype == torch.int64 and tuple(K.rng.shape) == (B, 2) and U.rng is None
        state = K.rng.data_ptr()
        for n in range(2):                      # step: the second one captures and replays
            assert _same(K.step(_frame(data, 24 + p)), U.step(_frame(data, 24 + p), _draws(eng, eps, p))), ("step", n)
            p += 1
        for n in range(2):                      # step_rows, mixed roles; the draw is made whatever the mask says
            fr = _frame(data, 24 + p)
            assert _same(K.step_rows(fr, face[:, n].contiguous(), roles[n]),
                         U.step_rows(fr, face[:, n].contiguous(), roles[n], _draws(eng, eps, p))), ("step_rows", n)
            p += 1
        fr = _chunk(data, 24, p, 2)             # step_many
        assert _same(K.step_many(fr), U.step_many(fr, _draws(eng, eps, p, n=2))), "step_many"
        p += 2
        fr = _chunk(data, 24, p, 2)             # step_rows_many
        assert _same(K.step_rows_many(fr, face[:, 2:4].contiguous(), roles), U.step_rows_many(fr, face[:, 2:4].contiguous(), roles,
                                                                                              _draws(eng, eps, p, n=2))), "step_rows_many"
        p += 2
        assert _same(K.step(_frame(data, 24 + p)), U.step(_frame(data, 24 + p), _draws(eng, eps, p))), "step after the chunks"
        assert _graphs(K) == _graphs(U) and K.replays == 4 and K.steps == 9
        assert K.rng.data_ptr() == state        # allocated at the open, never reallocated
        assert torch.equal(K.row_rng(), torch.tensor([[S.key_to_word(k), 9] for k in KEYS]))


def test_candidate_calls_reduce_to_explicit_noise(setup):
    m, data, _, _, eps = setup
    choice = [2, 0, 1, 1, 0, 2, 2, 1]
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as K, m.open_stream(_seed(data, 24)) as U:
        eng, p = K.eng, 0
        assert _same(K.step(_frame(data, 24)), U.step(_frame(data, 24), _draws(eng, eps, 0)))
        p += 1
        for pick in (None, choice):             # step_candidates + commit: the device's choice, then a given one
            fr = _frame(data, 24 + p)
            assert _same(K.step_candidates(fr, 3), U.step_candidates(fr, 3, _draws(eng, eps, p, ncand=3))), ("step_candidates", pick)
            assert torch.equal(K.row_rng()[:, 1], torch.full((B,), p))                      # (candidates move nothing)
            assert _same(K.commit(pick), U.commit(pick)), ("commit", pick)
            p += 1
        fr = _chunk(data, 24, p, 2)             # rollouts: dropped, then committed with a given choice, then with the device's
        assert _same(K.rollout_candidates(fr, 3), U.rollout_candidates(fr, 3, _draws(eng, eps, p, n=2, ncand=3))), "rollouts"
        K.discard(), U.discard()
        assert torch.equal(K.row_rng()[:, 1], torch.full((B,), p))
        for pick in (choice, None):
            fr = _chunk(data, 24, p, 2)
            assert _same(K.rollout_candidates(fr, 3), U.rollout_candidates(fr, 3, _draws(eng, eps, p, n=2, ncand=3))), ("rollouts", pick)
            assert _same(K.commit(pick), U.commit(pick)), ("rollout commit", pick)
            p += 2
        assert _same(K.step(_frame(data, 24 + p)), U.step(_frame(data, 24 + p), _draws(eng, eps, p))), "step after the candidates"
        assert _graphs(K) == _graphs(U) and K.steps == 8
        assert torch.equal(K.row_rng()[:, 1], torch.full((B,), 8))


def test_candidate_zero_is_the_plain_call(setup):
    m, data, _, _, _ = setup
    with m.open_stream(_seed(data, 24), return_nll=True, row_seeds=KEYS) as P, m.open_stream(_seed(data, 24), row_seeds=KEYS) as Q:
        for n in range(2):
            frame, nll = P.step(_frame(data, 24 + n))
            Q.step_candidates(_frame(data, 24 + n), 3)
            got, got_nll, picked = Q.commit(choice=[0] * B)
            assert torch.equal(got, frame) and torch.equal(got_nll, nll) and not picked.any(), n
            assert torch.equal(P.noise, Q._cand[3].noise[:, 0])


def test_positions_follow_the_position_function(setup):
    m, data, noise, _, _ = setup
    dev = data["p1_face"].device
    g = torch.Generator().manual_seed(12)
    face = torch.randn(B, 3, C_, generator=g).to(dev)
    lens = [3, 0, 1, 2, 0, 3, 1, 1]
    mask = [[True, False] * 4, [False] * 8]
    fr1, fr2, fr3 = _frame(data, 24), _chunk(data, 24, 0, 2), _chunk(data, 24, 0, 3)
    script = []
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as st:
        def did(kind, n=1, lengths=None):
            script.append((kind, n, lengths))
        st.step(fr1), did("step")
        st.observe(fr1, face[:, 0].contiguous()), did("observe")
        st.step_rows(fr1, face[:, 1].contiguous(), mask[0]), did("step_rows")
        st.step_many(fr2), did("step_many", 2)
        st.observe_many(fr2, face[:, :2].contiguous()), did("observe_many", 2)
        st.observe_many(fr3, face, lengths=lens), did("observe_many", 3, lens)
        st.step_rows_many(fr2, face[:, :2].contiguous(), mask), did("step_rows_many", 2)
        st.step_candidates(fr1, 2), did("step_candidates")
        st.commit(), did("commit", 1)
        st.rollout_candidates(fr2, 2), did("rollout_candidates", 2)
        st.commit(), did("commit", 2)
        st.rollout_candidates(fr3, 3), did("rollout_candidates", 3)
        st.discard(), did("discard", 3)
        st.step(fr1, noise[0]), did("step")                                  # the caller's noise: the frame is taken all the same
        st.step_many(fr2, noise[:2].contiguous()), did("step_many", 2)
        st.step_candidates(fr1, 2, noise[:2].transpose(0, 1).contiguous()), did("step_candidates")
        st.commit([0] * B), did("commit", 1)
        got = st.row_rng()
    want = [0] * B
    for kind, n, lengths in script:
        move = S.row_position_advance(kind, n, lengths)
        want = [p + (move[r] if isinstance(move, list) else move) for r, p in enumerate(want)]
    assert {k for k, _, _ in script} == {"step", "observe", "step_rows", "step_many", "observe_many", "step_rows_many", "step_candidates",
                                         "rollout_candidates", "commit", "discard"}
    assert got[:, 1].tolist() == want and len(set(want)) > 1
    assert [S.word_to_key(w) for w in got[:, 0]] == KEYS


def test_the_row_and_the_neighbours_do_not_matter(setup):
    m, data, _, _, _ = setup
    d5 = _rows_of(data, [0, 1, 2, 3, 4])
    with m.open_stream(_seed(d5, 24), row_seeds=KEYS[:5]) as X, m.open_stream(_seed(d5, 24), row_seeds=[KEYS[3], KEYS[1]] + OTHER[:3]) as Y, \
            m.open_stream(_seed(data, 24), row_seeds=OTHER[:6] + [KEYS[1], KEYS[3]]) as Z:
        for n in range(2):
            X.step(_frame(d5, 24 + n)), Y.step(_frame(d5, 24 + n)), Z.step(_frame(data, 24 + n))
            assert torch.equal(X.noise[3], Y.noise[0]) and torch.equal(X.noise[1], Y.noise[1]), n
            assert torch.equal(X.noise[3], Z.noise[7]) and torch.equal(X.noise[1], Z.noise[6]), n          # another batch size too
            assert not torch.equal(X.noise[0], Y.noise[0])


def test_the_form_of_the_call_does_not_matter(setup):
    m, data, _, _, eps = setup
    n = 3
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as a, m.open_stream(_seed(data, 24), row_seeds=KEYS) as b, \
            m.open_stream(_seed(data, 24), row_seeds=KEYS) as c:
        singles = []
        for i in range(n):
            a.step(_frame(data, 24 + i))
            singles.append(a.noise.clone())
        singles = torch.stack(singles)
        b.step_many(_chunk(data, 24, 0, n))
        many = b._chunk_ws["chunk_noise_draw"][:n * B * C_].view(n, B, C_)
        c.rollout_candidates(_chunk(data, 24, 0, n), 2)
        rolled = c._chunk_ws["rollout_noise_draw"][:n * B * 2 * C_].view(n, B, 2, C_)
        assert torch.equal(singles, many) and torch.equal(singles, rolled[:, :, 0])
        assert torch.equal(singles, _draws(a.eng, eps, 0, n=n))
        assert not torch.equal(rolled[:, :, 0], rolled[:, :, 1])
        c.discard()


def _through_the_host(saved):
    f = io.BytesIO()
    torch.save(saved.cpu().state_dict(), f)
    f.seek(0)
    back = StreamRows.from_state_dict(torch.load(f))
    assert not back.rng.is_cuda and torch.equal(back.rng, saved.rng.cpu())
    return back.to(saved.data.device)


def test_rollback_repeats_the_frames_without_any_noise_given(setup):
    m, data, _, _, _ = setup
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as st:
        for n in range(2):
            st.step(_frame(data, 24 + n))
        saved = st.save_rows(range(B))
        assert tuple(saved.rng.shape) == (B, 2) and saved.rng.dtype == torch.int64 and saved.rng.is_cuda
        assert torch.equal(saved.rng.cpu(), torch.tensor([[S.key_to_word(k), 2] for k in KEYS]))
        assert saved.data.shape == (B, st.row_signature[-1]) and saved.signature == st.row_signature
        first = [st.step(_frame(data, 24 + n)) for n in range(2, 5)]
        st.load_rows(list(range(B)), _through_the_host(saved))
        again = [st.step(_frame(data, 24 + n)) for n in range(2, 5)]
    assert torch.equal(torch.stack(first), torch.stack(again))


def test_rows_move_to_other_rows_of_another_session_and_branch(setup):
    m, data, _, _, eps = setup
    new, _ = _conversations(data["p1_face"].device, B, 8)
    src, dst = [1, 6], [6, 3]

    def mixed(n, at, rows, entries):
        fr, mine = _frame(new, 24 + at), _frame(data, 24 + n)
        for k in fr:
            fr[k][rows] = mine[k][entries]
        return fr

    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as A, m.open_stream(_seed(new, 24), row_seeds=OTHER) as A2:
        for n in range(3):
            A.step(_frame(data, 24 + n))
        for n in range(2):
            A2.step(_frame(new, 24 + n))
        A2.load_rows(dst, A.save_rows(src))
        assert torch.equal(A2.row_rng()[dst], A.row_rng()[src])
        for n in range(3, 5):
            a, a2 = A.step(_frame(data, 24 + n)), A2.step(mixed(n, n - 1, dst, src))
            assert torch.equal(A2.noise[dst], A.noise[src]) and torch.equal(a2[dst], a[src]), n
        # a branch: row 1 of A into rows 0 and 4 of A2 - row 0 with the entry's key, row 4 with a key of its own
        saved = A.save_rows([1])
        A2.load_rows([0], saved, entries=[0])
        A2.load_rows([4], saved, entries=[0], row_seeds=[4242])
        rng = A2.row_rng()
        assert rng[0].tolist() == [S.key_to_word(KEYS[1]), 5] and rng[4].tolist() == [4242, 5]
        for n in range(5, 7):
            a, a2 = A.step(_frame(data, 24 + n)), A2.step(mixed(n, n - 1, [0, 4], [1, 1]))
            assert torch.equal(a2[0], a[1]), n                               # the sibling without a key of its own: identical
            assert not torch.equal(a2[4], a[1]), n                           # the branch: different from the next frame on
            assert torch.equal(A2.noise[4], _draws(A.eng, eps, n, keys=[4242])[0])


def test_rows_without_rng_need_a_key_and_start_at_position_zero(setup):
    m, data, _, _, eps = setup
    with m.open_stream(_seed(data, 24)) as U, m.open_stream(_seed(data, 24), row_seeds=KEYS) as K:
        U.step(_frame(data, 24)), K.step(_frame(data, 24)), K.step(_frame(data, 25))
        old = U.save_rows([3, 5])
        assert old.rng is None and "rng" not in old.state_dict()
        before = K.row_rng()
        with pytest.raises(ValueError, match="the rows carry no keyed-noise state"):
            K.load_rows([2, 0], old)
        assert torch.equal(K.row_rng(), before)
        K.load_rows([2, 0], old, row_seeds=[77, 2 ** 64 - 2])
        after = K.row_rng()
        assert after[2].tolist() == [77, 0] and after[0].tolist() == [-2, 0]
        assert torch.equal(after[[1, 3, 4, 5, 6, 7]], before[[1, 3, 4, 5, 6, 7]])
        K.step(_frame(data, 26))
        assert torch.equal(K.noise[[2, 0]], _draws(K.eng, eps, 0, keys=[77, 2 ** 64 - 2]))
        assert torch.equal(K.noise[1], _draws(K.eng, eps, 2, keys=[KEYS[1]])[0])
        # the other way round: an unkeyed session takes keyed rows and ignores their state
        U.load_rows([1], K.save_rows([4]))
        with pytest.raises(ValueError, match="opened without row_seeds"):
            U.load_rows([1], K.save_rows([4]), row_seeds=[1])


def test_reset_rows_replays_without_keys_and_not_with_new_ones(setup):
    m, data, _, _, eps = setup
    rows, keep = [2, 5], [0, 1, 3, 4, 6, 7]
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as st, m.open_stream(_seed(data, 24), row_seeds=KEYS) as twin:
        st.step(_frame(data, 24)), twin.step(_frame(data, 24))
        first = st.noise.clone()
        st.step(_frame(data, 25)), twin.step(_frame(data, 25))
        st.reset_rows(rows, _rows_of(_seed(data, 24), rows))
        rng = st.row_rng()
        assert torch.equal(rng[keep], twin.row_rng()[keep]) and rng[rows].tolist() == [[S.key_to_word(KEYS[r]), 0] for r in rows]
        a, b = st.step(_frame(data, 26)), twin.step(_frame(data, 26))
        assert torch.equal(a[keep], b[keep]) and torch.equal(st.noise[keep], twin.noise[keep])      # the others: undisturbed
        assert torch.equal(st.noise[rows], first[rows])                                             # None: the first draws again
        st.reset_rows(rows, _rows_of(_seed(data, 24), rows), row_seeds=[500, 501])
        assert st.row_rng()[rows].tolist() == [[500, 0], [501, 0]]
        st.step(_frame(data, 27)), twin.step(_frame(data, 27))
        assert not torch.equal(st.noise[2], first[2]) and not torch.equal(st.noise[5], first[5])
        assert torch.equal(st.noise[rows], _draws(st.eng, eps, 0, keys=[500, 501]))
        assert torch.equal(st.noise[keep], twin.noise[keep])
        # reset(): None keeps the keys at position 0, keys replace them
        st.reset(_seed(data, 24))
        assert st.row_rng().tolist() == [[S.key_to_word(k), 0] for k in KEYS[:2] + [500] + KEYS[3:5] + [501] + KEYS[6:]]
        st.reset(_seed(data, 24), row_seeds=OTHER)
        assert st.row_rng().tolist() == [[k, 0] for k in OTHER]
        st.step(_frame(data, 24))
        assert torch.equal(st.noise, _draws(st.eng, eps, 0, keys=OTHER))


def test_keyed_inference_draws_row_noise_and_matches_the_keyed_session(setup, monkeypatch):
    m, data, noise, seq_len, eps = setup
    n = FRAMES
    seen = {}
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as st:
        eng = st.eng
        out = torch.stack([st.step(_frame(data, 24 + i)) for i in range(n)], 1)
        sample = eng.sample

        def spy(seq_len, data, noise, *args, **kwargs):
            seen["noise"] = noise.clone()
            return sample(seq_len, data, noise, *args, **kwargs)
        monkeypatch.setattr(eng, "sample", spy)
        inf = m.inference(seq_len, data, row_seeds=KEYS)
        assert torch.equal(seen["noise"], _draws(eng, eps, 0, n=n))
        # a row's noise does not depend on its batch: rows 0 and 1 alone, the keys as bit patterns in a tensor
        m.inference(seq_len, _rows_of(data, [0, 1]), row_seeds=torch.tensor([S.key_to_word(KEYS[0]), KEYS[1]]))
        assert torch.equal(seen["noise"], _draws(eng, eps, 0, n=n)[:, [0, 1]])
        with pytest.raises(ValueError, match="noise and row_seeds are both given"):
            m.inference(seq_len, data, noise=noise, row_seeds=KEYS)
    err = (out - inf).abs().max().item()
    report("keyed inference() against a keyed session, %d frames: max abs difference %.3e" % (n, err))
    assert err < 1e-5, err


def test_keyed_steady_state_steps_do_not_synchronise(setup):
    m, data, _, _, _ = setup
    frames = [_frame(data, 24 + n) for n in range(6)]
    new = _rows_of(_seed(data, 24), [0, 1])
    with m.open_stream(_seed(data, 24), row_seeds=KEYS) as st:
        st.step(frames[0])
        st.step(frames[1])                      # (the capture synchronises once)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for n in range(2, 4):
                st.step(frames[n])
            saved = st.save_rows([1, 2])
            st.load_rows([4, 5], saved, row_seeds=[8, 9])
            st.reset_rows([6, 7], new, row_seeds=[10, 11])
            for n in range(4, 6):
                st.step(frames[n])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 5
        assert st.row_rng()[:, 1].tolist() == [6, 6, 6, 6, 6, 6, 2, 2]


def test_an_unkeyed_session_draws_from_the_process_generator_as_before(setup):
    m, data, _, _, eps = setup
    dev = data["p1_face"].device
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        with m.open_stream(_seed(data, 24)) as st:
            assert st.rng is None
            outs.append(torch.stack([st.step(_frame(data, 24 + n)) for n in range(3)], 1))
            assert st.save_rows([0]).rng is None
            with pytest.raises(ValueError, match="opened without row_seeds"):
                st.row_rng()
            with pytest.raises(ValueError, match="opened without row_seeds"):
                st.reset(_seed(data, 24), row_seeds=KEYS)
    torch.manual_seed(5)
    drawn = torch.stack([torch.empty(B, C_, device=dev).normal_(0.0, eps) for _ in range(3)])
    with m.open_stream(_seed(data, 24)) as st:
        given = _run(st, data, drawn, 24)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], given)
