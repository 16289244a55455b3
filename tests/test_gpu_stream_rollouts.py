"""GPU: N candidate rollouts of n frames per row of a streaming session (SampleStream.rollout_candidates -> lfi_stream_cand_seq_in and
lfi_flow_sample_cand_seq, the sampler over B * ncand virtual rows that read their parent row's static pre-activations in place;
commit -> lfi_stream_commit_cand_seq; discard; rollout_best_of): every candidate against the step_many() it stands for on a reference
session rolled back with save_rows / load_rows, commit against that reference's state, the commit kernel alone on crafted buffers,
discard, shared dropout masks, the pending rule, the range guard and no host wait.

Exactness. ncand = 1 is torch.equal with step_many() on every path (the same launches on the same shapes). At the final widths in
bf16x3 engine mode - the fused front end and the one-launch chain, in neither of which rows mix - every candidate and every committed
row record is torch.equal for any ncand. Everywhere else (the front-end GEMMs run over B * ncand rows and may tile differently) the
stream tests' own gates hold: frames and records 1e-5 absolute, NLL max_rel(nll, expected, floor=1.0) < 1e-4; what was bit-identical
anyway is reported."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, report
from lets_face_it_amd import _lib
from test_gpu_parity import build, to_dev
from test_gpu_stream import _final_setup, _frame, _seed
from test_gpu_stream_candidates import _case, _noise
from test_gpu_stream_chunk import _chunk

pytestmark = pytest.mark.gpu

NLL_GATE = 1e-4
FRAME_GATE = 1e-5
# (B, ncand): V = 15, one partial chain tile; V = 35, parents straddle chain tiles; V = 65, one row past the fused kernel's 64-row
# tile with a parent split across it; one parent over two chain tiles; one candidate per row (= step_many)
SHAPES = ((3, 5), (5, 7), (5, 13), (1, 17), (16, 1))


def _roll(S, R, data, start, first, n, ncand, z, before, seed, exact, label, worst):
    """Session S, `first` frames into its sequence and saved as `before` (None: fresh - the reference is reset instead), rolls ncand
    candidates of frames first .. first + n - 1 out; the reference R (return_nll), put back to the same state for every j, takes
    step_many(frames, z[:, :, j]). Then S commits a fixed choice and R, put back once more, takes the chosen draws: outputs, row
    records and the next generated frame must agree. worst: [frames, nll] - the largest differences seen where not exact."""
    B, Cc, dev = S.B, S.eng.spec.C, S.device
    every, rows = list(range(B)), torch.arange(B, device=dev)
    frames = _chunk(data, start, first, n)

    def rewind():
        if before is None:
            R.reset(seed)
        else:
            R.load_rows(every, before)

    def close(a, b, what, nll=False):
        if exact:
            assert torch.equal(a, b), (label, what)
        elif nll:
            worst[1] = max(worst[1], max_rel(a, b, floor=1.0))
        else:
            worst[0] = max(worst[0], (a - b).abs().max().item())

    was = None if before is None else S.save_rows(every).data.clone()
    steps = S.steps
    faces, nll = S.rollout_candidates(frames, ncand, z)
    assert tuple(faces.shape) == (B, ncand, n, Cc) and tuple(nll.shape) == (n, B, ncand) and nll.dtype == torch.float32
    assert S._pending.kind == "rollouts" and S._pending.ncand == ncand and S._pending.n == n and S.steps == steps
    assert torch.isfinite(faces).all() and torch.isfinite(nll).all()
    if ncand > 1:
        assert not torch.equal(faces[:, 0], faces[:, 1])
    same = True
    for j in range(ncand):
        rewind()
        out, q = R.step_many(frames, z[:, :, j].contiguous())
        close(faces[:, j], out, ("frames", j))
        close(nll[:, :, j], q, ("nll", j), nll=True)
        same = same and torch.equal(faces[:, j], out) and torch.equal(nll[:, :, j], q)
    choice = [(3 * r + first + 1) % ncand for r in range(B)]
    pick = torch.tensor(choice, device=dev)
    out, q, picked = S.commit(choice)
    assert S._pending is None and S.steps == steps + n and picked.tolist() == choice and picked.dtype == torch.int32
    assert tuple(out.shape) == (B, n, Cc) and tuple(q.shape) == (n, B)
    assert torch.equal(out, faces[rows, pick]) and torch.equal(q, nll[:, rows, pick])
    rewind()
    R.step_many(frames, z[:, rows, pick].contiguous())
    a, b = S.save_rows(every).data, R.save_rows(every).data
    close(a, b, "records")
    same = same and torch.equal(a, b)
    if was is not None:
        assert not torch.equal(a, was)
    # the frame generated next, from the committed state
    zz = z[0, :, 0].contiguous()
    fr = _frame(data, start + first + n)
    close(S.step(fr, zz), R.step(fr, zz)[0], "next frame")
    return same


def _rollouts_against_step_many(m, data, start, B, ncand, ns, warm, label, exact):
    """A session per n of `ns`: `warm` step()s (0: the rollout starts from a fresh session, first_frame = 0, zero state), then _roll.
    -> (worst frames / records difference, worst NLL relative difference, whether everything was bit-identical)."""
    dev = next(iter(data.values())).device
    Cc, every, seed = m.spec.C, list(range(B)), _seed(data, start)
    worst, same = [0.0, 0.0], True
    for n in ns:
        z = _noise(B, ncand, Cc, n, dev, seed=7 + n)
        with m.open_stream(seed) as S, m.open_stream(seed, return_nll=True) as R:
            for t in range(warm):
                S.step(_frame(data, start + t), z[0, :, 0].contiguous())
            before = S.save_rows(every) if warm else None
            same = _roll(S, R, data, start, warm, n, ncand, z, before, seed, exact, "%s, n = %d" % (label, n), worst) and same
    return worst[0], worst[1], same


@pytest.mark.parametrize("name", FIXTURES)
def test_each_rollout_is_the_step_many_it_stands_for(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    m._ensure_engine(gpu_device)
    B, ncand, n = 3, 5, 3
    data = _case(m, gpu_device, B, 2 + n + 1, fx.start)
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        f, q, same = _rollouts_against_step_many(m, data, fx.start, B, ncand, (n,), 2, name, exact=False)
        report("%s (%s) rollouts, (B, ncand, n) = (3, 5, 3) vs step_many(): frames / records max abs diff %.3e, NLL max rel diff %.3e%s"
               % (name, precision, f, q, "; bit-identical" if same else ""))
        assert f < FRAME_GATE and q < NLL_GATE, (name, precision, f, q)
        # one candidate per row: the launches and shapes of step_many, bit for bit
        _rollouts_against_step_many(m, data, fx.start, B, 1, (n,), 2, "%s (%s), ncand = 1" % (name, precision), exact=True)


@pytest.mark.parametrize("precision", ("bf16x3", "f32"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-n%d" % s)
def test_each_rollout_is_the_step_many_at_final_model_widths(shape, precision, gpu_device):
    """n = 1: the first frame only; 2: the first hand-over of window fragments from the chain to the next frame's front end;
    hist1 + 2: a window made wholly of generated frames."""
    B, ncand = shape
    _, m, _, data, _, _ = _final_setup(gpu_device, B, 2 + 16)
    m.precision = precision
    data = to_dev(data, gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        hist1 = st.hist1
    assert 1 <= hist1 <= 12
    exact = precision == "bf16x3" or ncand == 1
    f, q, same = _rollouts_against_step_many(m, data, 24, B, ncand, (1, 2, hist1 + 2), 2, "final widths %s (%s)" % (shape, precision), exact)
    if not exact:
        report("final widths %s (%s) rollouts vs step_many(): frames / records max abs diff %.3e, NLL max rel diff %.3e%s"
               % (shape, precision, f, q, "; bit-identical" if same else ""))
        assert f < FRAME_GATE and q < NLL_GATE, (shape, precision, f, q)


@pytest.mark.parametrize("precision", ("bf16x3", "f32"))
def test_rollouts_from_a_fresh_session(precision, gpu_device):
    """first_frame = 0: no state is broadcast, the first frame's cells start from zeros."""
    B, ncand = 5, 7
    _, m, _, data, _, _ = _final_setup(gpu_device, B, 6)
    m.precision = precision
    data = to_dev(data, gpu_device)
    exact = precision == "bf16x3"
    f, q, _ = _rollouts_against_step_many(m, data, 24, B, ncand, (1, 3), 0, "final widths, fresh (%s)" % precision, exact)
    assert f < FRAME_GATE and q < NLL_GATE, (precision, f, q)
    fx = Fixture("tiny_lstm")
    m = build(fx, gpu_device)
    m._ensure_engine(gpu_device)
    data = _case(m, gpu_device, 3, 4, fx.start)
    f, q, _ = _rollouts_against_step_many(m, data, fx.start, 3, 5, (3,), 0, "tiny_lstm, fresh", exact=False)
    assert f < FRAME_GATE and q < NLL_GATE, (f, q)


@pytest.mark.parametrize("switch", ("LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1", "LFI_SAMPLE_FUSED=0", "LFI_SAMPLE_XF_CHAIN=0",
                                    "LFI_SAMPLE_XFRAG=0", "LFI_SAMPLE_WFRAG16=0"))
def test_rollouts_under_every_switch(switch, gpu_device, monkeypatch):
    B, ncand = 5, 7
    _, m, _, data, _, _ = _final_setup(gpu_device, B, 6)
    m.precision = "bf16x3"
    data = to_dev(data, gpu_device)
    monkeypatch.setenv(*switch.split("="))
    f, q, same = _rollouts_against_step_many(m, data, 24, B, ncand, (2,), 2, "final widths (%s)" % switch, exact=False)
    report("final widths (%s) rollouts, (B, ncand, n) = (5, 7, 2) vs step_many(): frames / records max abs diff %.3e, NLL max rel "
           "diff %.3e%s" % (switch, f, q, "; bit-identical" if same else ""))
    assert f < FRAME_GATE and q < NLL_GATE, (switch, f, q)
    _rollouts_against_step_many(m, data, 24, B, 1, (2,), 2, "final widths (%s), ncand = 1" % switch, exact=True)


@pytest.mark.parametrize("name", ("tiny_lstm", "p1enc", "p1lstm", "p1mlp"))
def test_rollouts_of_an_lstm_flow_and_of_encoded_face_windows(name, gpu_device):
    """B, ncand = 5, 7 (V = 35: parents straddle chain tiles), n = 4, where the every-fixture test has one tile."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    m._ensure_engine(gpu_device)
    m.precision = "bf16x3"
    data = _case(m, gpu_device, 5, 2 + 4 + 1, fx.start)
    f, q, same = _rollouts_against_step_many(m, data, fx.start, 5, 7, (4,), 2, name, exact=False)
    report("%s rollouts, (B, ncand, n) = (5, 7, 4) vs step_many(): frames / records max abs diff %.3e, NLL max rel diff %.3e%s"
           % (name, f, q, "; bit-identical" if same else ""))
    assert f < FRAME_GATE and q < NLL_GATE, (name, f, q)


def _final_case(device, B, ncand, N, n, precision="bf16x3"):
    _, m, _, data, _, _ = _final_setup(device, B, N)
    m.precision = precision
    return m, to_dev(data, device), _noise(B, ncand, 50, n, device)


def _host_choice(nll):
    """The default choice from the returned nll (n, B, ncand): the sum over the frames in ascending order in fp32, then the least."""
    tot = nll[0].clone()
    for f in range(1, nll.shape[0]):
        tot = tot + nll[f]
    return tot.argmin(1).tolist()


@pytest.mark.parametrize("how", ("host", "device", "none"))
def test_commit_leaves_the_session_where_step_many_would(how, gpu_device):
    B, ncand, n, N = 5, 7, 3, 10
    m, data, z = _final_case(gpu_device, B, ncand, N, n)
    every, rows = list(range(B)), torch.arange(B, device=gpu_device)
    plain = _noise(B, 1, 50, N, gpu_device, seed=3)[:, :, 0].contiguous()
    with m.open_stream(_seed(data, 24)) as S, m.open_stream(_seed(data, 24), return_nll=True) as R:
        S.step(_frame(data, 24), plain[0])
        R.step(_frame(data, 24), plain[0])
        faces, nll = S.rollout_candidates(_chunk(data, 24, 1, n), ncand, z)
        want = [6, 0, 3, 3, 1]
        if how == "none":
            want = _host_choice(nll)
            out, q, picked = S.commit()
        else:
            out, q, picked = S.commit(want if how == "host" else torch.tensor(want, device=gpu_device))
        assert picked.tolist() == want and picked.dtype == torch.int32
        pick = torch.tensor(want, device=gpu_device)
        assert torch.equal(out, faces[rows, pick]) and torch.equal(q, nll[:, rows, pick])
        ref, ref_q = R.step_many(_chunk(data, 24, 1, n), z[:, rows, pick].contiguous())
        assert torch.equal(out, ref) and torch.equal(q, ref_q)
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data) and S.steps == R.steps == 1 + n
        for t in range(1 + n, N):
            assert torch.equal(S.step(_frame(data, 24 + t), plain[t]), R.step(_frame(data, 24 + t), plain[t])[0]), t
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data)
    # a device choice outside the candidates is clamped by the kernel, int64 as int32
    with m.open_stream(_seed(data, 24)) as S:
        S.rollout_candidates(_chunk(data, 24, 0, n), ncand, z)
        _, _, picked = S.commit(torch.tensor([-3, 0, 6, 7, 1 << 20], device=gpu_device, dtype=torch.int64))
        assert picked.tolist() == [0, 0, 6, 6, 6]


@pytest.mark.parametrize("lstm", (False, True))
def test_commit_kernel_alone_on_crafted_buffers(lstm, gpu_device):
    B, ncand, n, start, Ks, H, Cc, hist, G = 5, 3, 3, 4, 2, 7, 6, 5, 11   # hist > n: old frames stay in the window; G: guard floats
    L, V, T, dev = _lib.lib(), 5 * 3, 4 + 3, gpu_device
    g = torch.Generator().manual_seed(1)
    nan = float("nan")
    cand_seq = torch.randn(V, T, Cc, generator=g).to(dev)
    cand_h, cand_c = torch.randn(Ks, V, H, generator=g).to(dev), torch.randn(Ks, V, H, generator=g).to(dev)
    # sums, exact by construction. row 0: a tie of the first two (3 + 1 + 0.5 and 0.5 + 1 + 3); row 1: a NaN sum in front; row 2: all
    # NaN; row 3: the last wins; row 4: a NaN sum behind a tie of 0 and 1
    per_row = [[[3.0, 1.0, 0.5], [0.5, 1.0, 3.0], [2.0, 2.0, 1.0]],
               [[1.0, nan, 1.0], [2.0, 2.0, 1.0], [1.0, 2.0, 1.0]],
               [[nan, 1.0, 1.0], [1.0, nan, 1.0], [1.0, 1.0, nan]],
               [[4.0, 4.0, 1.0], [4.0, 2.0, 2.0], [-9.0, 1.0, 1.0]],
               [[0.25, 0.5, 0.25], [0.5, 0.25, 0.25], [0.0, nan, 0.0]]]
    cand_nll = torch.tensor(per_row).permute(2, 0, 1).contiguous().to(dev)      # (n, B, ncand)

    def guarded(*shape, dtype=torch.float32):
        k = 1
        for v in shape:
            k *= v
        buf = torch.full((k + 2 * G,), -77.0, device=dev).to(dtype)
        return buf, buf[G:G + k].view(*shape)

    def run(choice):
        bufs = {k: guarded(*shape) for k, shape in (("win", (B, hist, Cc)), ("h", (Ks, B, H)), ("c", (Ks, B, H)), ("out", (B, n, Cc)),
                                                    ("nll", (n, B)), ("nb", (B,)))}
        bufs["pick"] = guarded(B, dtype=torch.int32)
        guard = torch.zeros(1, dtype=torch.int32, device=dev)
        cs = bufs["c"][1] if lstm else None
        rc = L.lfi_stream_commit_cand_seq(B, ncand, n, start, Cc, Ks, H, None if choice is None else choice.data_ptr(),
                                          cand_seq.data_ptr(), cand_nll.data_ptr(), cand_h.data_ptr(), cand_c.data_ptr() if lstm else None,
                                          bufs["win"][1].data_ptr(), hist, bufs["h"][1].data_ptr(), None if cs is None else cs.data_ptr(),
                                          bufs["nb"][1].data_ptr(), bufs["out"][1].data_ptr(), bufs["nll"][1].data_ptr(),
                                          bufs["pick"][1].data_ptr(), guard.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.lfi_last_error()
        torch.cuda.synchronize()
        return bufs, guard

    for choice, want in ((None, [0, 2, 0, 2, 0]),
                         (torch.tensor([2, -1, 3, 1, 100], dtype=torch.int32, device=dev), [2, 0, 2, 1, 2])):
        bufs, guard = run(choice)
        rows, pick = torch.arange(B, device=dev), torch.tensor(want, device=dev)
        v = rows * ncand + pick
        assert bufs["pick"][1].tolist() == want
        assert torch.equal(bufs["out"][1], cand_seq[v, start:])
        got, exp = bufs["nll"][1], cand_nll[:, rows, pick]
        assert torch.equal(got.isnan(), exp.isnan()) and torch.equal(got[~exp.isnan()], exp[~exp.isnan()])
        assert torch.equal(bufs["win"][1], cand_seq[v, T - hist:])
        assert torch.equal(bufs["h"][1], cand_h[:, v])
        assert torch.equal(bufs["c"][1], cand_c[:, v]) if lstm else bool((bufs["c"][1] == -77.0).all())
        assert bool((bufs["nb"][1] == -77.0 + 2 * n).all())
        for name, (whole, _) in bufs.items():
            assert bool((whole[:G] == -77).all()) and bool((whole[-G:] == -77).all()), name
        # the guard word holds max |frame| of the committed frames, as bits
        assert guard.view(torch.float32).item() == cand_seq[v, start:].abs().max().item()
    # the entry point's refusals
    assert L.lfi_stream_commit_cand_seq(B, ncand, n, start, Cc, Ks, H, None, cand_seq.data_ptr(), cand_nll.data_ptr(), cand_h.data_ptr(),
                                        None, cand_seq.data_ptr(), start + n + 1, cand_h.data_ptr(), None, None, cand_seq.data_ptr(),
                                        cand_nll.data_ptr(), cand_nll.data_ptr(), None, None) == -1
    assert b"hist" in L.lfi_last_error()


def test_discard_leaves_the_session_bit_for_bit_as_it_was(gpu_device):
    B, ncand, n, N = 5, 7, 3, 6
    m, data, z = _final_case(gpu_device, B, ncand, N, n)
    every = list(range(B))
    plain = _noise(B, 1, 50, N, gpu_device, seed=3)[:, :, 0].contiguous()
    with m.open_stream(_seed(data, 24)) as S, m.open_stream(_seed(data, 24)) as R:
        with pytest.raises(RuntimeError, match="discard\\(\\) without pending rollouts"):
            S.discard()
        for st in (S, R):
            st.step(_frame(data, 24), plain[0])
            st.step(_frame(data, 25), plain[1])
        was = S.save_rows(every).data.clone()
        replays = S.replays
        # rolled out under OTHER conditioning than what follows: a hypothesis that is dropped
        S.rollout_candidates(_chunk(data, 24, 3, n), ncand, z)
        assert S.steps == 2
        S.discard()
        assert S._pending is None and S.steps == 2 and S.replays == replays
        assert torch.equal(S.save_rows(every).data, was) and torch.equal(was, R.save_rows(every).data)
        for t in range(2, N):
            assert torch.equal(S.step(_frame(data, 24 + t), plain[t]), R.step(_frame(data, 24 + t), plain[t])), t
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data)
        # one-frame candidates cannot be discarded: their windows have moved
        S.reset(_seed(data, 24))
        S.step_candidates(_frame(data, 24), 3)
        with pytest.raises(RuntimeError, match=r"commit\(\) one of them, or reset\(\)"):
            S.discard()
        assert S._pending == 3
        S.commit()


def test_rollouts_share_their_rows_dropout_masks_in_train_mode(gpu_device):
    """Train mode with injected per-frame masks: the static part runs once per row, so a row's candidates see the masks its
    step_many() would, frame by frame."""
    fx = Fixture("p1enc")
    m = build(fx, gpu_device, train=True)
    m._ensure_engine(gpu_device)
    B, n = 3, 3
    g = torch.Generator().manual_seed(5)
    m.injected_masks = {e.name: ((torch.rand(2 + n + 1, B, e.hist, generator=g) < 0.6).float() / 0.6)
                        for e in m.spec.encoders if e.dropout > 0 and e.name != "p1_face"}
    assert m.injected_masks
    data = _case(m, gpu_device, B, 2 + n + 1, fx.start)
    dev, Cc, every, seed = gpu_device, m.spec.C, list(range(B)), _seed(data, fx.start)
    z = _noise(B, 5, Cc, n, dev)
    worst = [0.0, 0.0]
    with m.open_stream(seed) as S, m.open_stream(seed, return_nll=True) as R:
        for t in range(2):
            for st in (S, R):                   # (R steps too: injected masks are indexed by `steps`)
                st.step(_frame(data, fx.start + t), z[0, :, 0].contiguous())
        before = S.save_rows(every)
        frames = _chunk(data, fx.start, 2, n)
        faces, nll = S.rollout_candidates(frames, 5, z)
        for j in range(5):
            R.load_rows(every, before)
            R.steps = 2
            out, q = R.step_many(frames, z[:, :, j].contiguous())
            worst[0] = max(worst[0], (out - faces[:, j]).abs().max().item())
            worst[1] = max(worst[1], max_rel(nll[:, :, j], q, floor=1.0))
        # the masks matter: without them the frames differ by more than the gate
        S.discard()
        m.injected_masks = {k: torch.ones_like(v) for k, v in m.injected_masks.items()}
    with m.open_stream(seed) as S:
        for t in range(2):
            S.step(_frame(data, fx.start + t), z[0, :, 0].contiguous())
        plain, _ = S.rollout_candidates(frames, 5, z)
    report("p1enc, train mode, injected masks: rollouts vs step_many(): frames max abs diff %.3e, NLL max rel diff %.3e" % tuple(worst))
    assert worst[0] < FRAME_GATE and worst[1] < NLL_GATE, worst
    assert (plain - faces).abs().max().item() > 10 * FRAME_GATE


def test_pending_rollouts_refuse_every_other_call_and_leave_the_session_as_it_was(gpu_device):
    B, ncand, n, N = 5, 7, 2, 6
    m, data, z = _final_case(gpu_device, B, ncand, N, n)
    every = list(range(B))
    plain = _noise(B, 1, 50, N, gpu_device, seed=3)[:, :, 0].contiguous()
    seed = _seed(data, 24)
    face = torch.zeros(B, 50, device=gpu_device)
    with m.open_stream(seed) as S, m.open_stream(seed) as R:
        for st in (S, R):
            st.step(_frame(data, 24), plain[0])
        saved = S.save_rows(every)
        was = saved.data.clone()
        S.rollout_candidates(_chunk(data, 24, 1, n), ncand, z)
        fr, frs = _frame(data, 26), _chunk(data, 24, 2, 1)
        calls = (lambda: S.step(fr, plain[2]), lambda: S.observe(fr, face), lambda: S.step_rows(fr, face, [True] * B),
                 lambda: S.step_candidates(fr, ncand), lambda: S.step_best_of(fr, ncand), lambda: S.step_many(frs, plain[2:3]),
                 lambda: S.observe_many(frs, face[:, None].contiguous()),
                 lambda: S.step_rows_many(frs, face[:, None].contiguous(), [[True] * B]),
                 lambda: S.rollout_candidates(frs, ncand), lambda: S.rollout_best_of(frs, ncand),
                 lambda: S.save_rows(every), lambda: S.load_rows(every, saved), lambda: S.reset_rows([0], {k: v[:1] for k, v in seed.items()}))
        for call in calls:
            with pytest.raises(RuntimeError, match=r"7 candidate rollouts of 2 frames per row are pending \(rollout_candidates\)"):
                call()
        assert S._pending.ncand == ncand and S.steps == 1
        S.discard()
        assert torch.equal(S.save_rows(every).data, was)
        # reset() drops pending rollouts and starts the sequence again
        S.rollout_candidates(_chunk(data, 24, 1, n), ncand, z)
        S.reset(seed)
        R.reset(seed)
        assert S._pending is None and S.steps == 0
        with pytest.raises(RuntimeError, match="without pending candidates"):
            S.commit()
        assert torch.equal(S.step(_frame(data, 24), plain[0]), R.step(_frame(data, 24), plain[0]))
        assert torch.equal(S.save_rows(every).data, R.save_rows(every).data)


def test_a_rollout_is_one_round(gpu_device, monkeypatch):
    B, ncand, n, N = 5, 7, 3, 6
    m, data, z = _final_case(gpu_device, B, ncand, N, n)
    every = list(range(B))
    with m.open_stream(_seed(data, 24)) as S:
        assert S._rollout_cap(1) == S._chunk_cap() and S._rollout_cap(256) < S._rollout_cap(2) <= S._chunk_cap()
        S.step(_frame(data, 24), z[0, :, 0].contiguous())
        was = S.save_rows(every).data.clone()
        monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "2")
        with pytest.raises(ValueError, match=r"more than the one round a rollout is \(at most 2 frames\)"):
            S.rollout_candidates(_chunk(data, 24, 1, n), ncand, z)
        assert S._pending is None and S.steps == 1 and torch.equal(S.save_rows(every).data, was)    # refused: nothing moved
        monkeypatch.setenv("LFI_OBSERVE_CHUNK_FRAMES", "3")
        _, nll = S.rollout_candidates(_chunk(data, 24, 1, n), ncand, z)
        out, q, picked = S.commit()
        assert S.steps == 1 + n and tuple(out.shape) == (B, n, 50) and picked.tolist() == _host_choice(nll)


def test_rollouts_are_refused_after_a_parameter_change_and_after_close(gpu_device):
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    B = data["p1_face"].shape[0]
    st = m.open_stream(_seed(data, fx.start))
    st.rollout_candidates(_chunk(data, fx.start, 0, 2), 3)
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.commit()
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.discard()
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.rollout_candidates(_chunk(data, fx.start, 0, 2), 3)
    st = m.open_stream(_seed(data, fx.start))
    out, q, picked = st.rollout_best_of(_chunk(data, fx.start, 0, 2), 3)     # the session's own draws
    assert tuple(out.shape) == (B, 2, fx.C) and torch.isfinite(out).all() and torch.isfinite(q).all() and int(picked.max()) < 3
    with pytest.raises(ValueError, match="ncand"):
        st.rollout_candidates(_chunk(data, fx.start, 2, 2), 0)
    with pytest.raises(ValueError, match="noise"):
        st.rollout_candidates(_chunk(data, fx.start, 2, 2), 3, torch.zeros(2, B, 2, fx.C, device=gpu_device))
    st.rollout_candidates(_chunk(data, fx.start, 2, 2), 3)
    with pytest.raises(ValueError, match="choice"):
        st.commit([0] * (B + 1))
    assert st.steps == 2 and st._pending.ncand == 3
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.commit()
    with pytest.raises(RuntimeError, match="closed"):
        st.discard()
    with pytest.raises(RuntimeError, match="closed"):
        st.rollout_candidates(_chunk(data, fx.start, 2, 2), 3)
    assert st._pending is None


def test_rollout_noise_beyond_the_fp16_range_trips_the_guard_as_step_manys_does(gpu_device):
    B, ncand, n, N = 5, 7, 2, 8
    m, data, z = _final_case(gpu_device, B, ncand, N, n)
    bad = z.clone()
    bad[1, 3, 5, 2] = 1.0e5                           # one candidate of one row, not the first: only the rollout's own fold sees it
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        st.rollout_best_of(_chunk(data, 24, 0, n), ncand, z)
        torch.cuda.synchronize()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            st.rollout_best_of(_chunk(data, 24, 2, n), ncand, z)
        assert st.frame_precision == 9
    with m.open_stream(_seed(data, 24)) as st:
        st.rollout_candidates(_chunk(data, 24, 0, n), ncand, bad)
        st.discard()
        torch.cuda.synchronize()                      # (the guard's copy has landed: the next call reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            st.rollout_candidates(_chunk(data, 24, 0, n), ncand, z)
        assert st.frame_precision == 5
        out, q, _ = st.commit()
        assert torch.isfinite(out).all() and torch.isfinite(q).all()
    # step_many() itself, the same warning for the same value
    with m.open_stream(_seed(data, 24)) as st:
        st.step_many(_chunk(data, 24, 0, n), bad[:, :, 5].contiguous())
        torch.cuda.synchronize()
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            st.step_many(_chunk(data, 24, 2, n), z[:, :, 0].contiguous())


def test_steady_state_rollouts_do_not_synchronise(gpu_device):
    B, ncand, n, N = 5, 7, 2, 12
    m, data, z = _final_case(gpu_device, B, ncand, N, n)
    chunks = [_chunk(data, 24, t, n) for t in range(0, N - n, n)]
    pick = torch.tensor([1, 0, 6, 2, 9], device=gpu_device)
    with m.open_stream(_seed(data, 24)) as st:
        st.rollout_best_of(chunks[0], ncand, z)                  # (the buffers' first use)
        st.rollout_candidates(chunks[1], ncand, z)
        st.discard()
        torch.cuda.set_sync_debug_mode("error")
        try:
            st.rollout_candidates(chunks[1], ncand, z)
            st.commit()                                          # the arg-min on the device
            st.rollout_candidates(chunks[2], ncand, z)
            st.discard()
            st.rollout_candidates(chunks[2], ncand, z)
            st.commit(pick)                                      # a device choice
            st.rollout_best_of(chunks[3], ncand)                 # noise drawn by the session
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 0 and st.steps == 4 * n and st._graph is None
