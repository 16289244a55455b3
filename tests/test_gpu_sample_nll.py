"""GPU: the per-frame likelihood the samplers report (SeqGlow.inference / open_stream with return_nll=True) against the fp64
oracle's teacher-forced pass over the generated frames (tests/sample_nll_expected.py), against the engine's own forward NLL, in
streaming sessions (graph replay, reseeded rows, branches, best-of-N), on every kernel path of the sampler and at full depth.

One gate everywhere, the project's per-frame NLL gate (tests/test_gpu_parity.py, BASELINE.json north_star):
max_rel(nll, expected, floor=1.0) < 1e-4."""
import pytest
import torch

from helpers import FIXTURES, Fixture, max_rel, report
from oracle import seqglow_oracle as oracle
from sample_nll_expected import fixture_expected, teacher_forced
from test_gpu_parity import build, final_model_hparams, perturbed_model, to_dev

pytestmark = pytest.mark.gpu

GATE = 1e-4


def _infer_case(fx, device):
    data = to_dev(fx.group("infer/data/"), device)
    noise = fx.get("infer/noise", torch.float32).to(device)
    return data, noise, int(fx.get("infer/seq_len"))


def _seed(data, start):
    return {k: v[:, :start].contiguous() for k, v in data.items() if v.dim() == 3}


def _frame(data, t):
    return {k: v[:, t].contiguous() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}


def _check_parity(fx, m, device, what, precisions=("f32", "bf16x3")):
    """Test 1 of the feature: nll against the oracle's NLL of the reference's frames, frames bit-identical to a run without it."""
    data, noise, seq_len = _infer_case(fx, device)
    _, expected = fixture_expected(fx)
    for precision in precisions:
        m.precision = precision
        plain = m.inference(seq_len, data, noise=noise)
        for rep in range(2):      # (the second call of a shape replays the captured graphs)
            out, nll = m.inference(seq_len, data, noise=noise, return_nll=True)
            assert nll.is_cuda and nll.dtype == torch.float32 and tuple(nll.shape) == (seq_len - fx.start, fx.B)
            err = max_rel(nll, expected, floor=1.0)
            report("%s%s (%s, call %d): sampler NLL max rel err vs fp64 oracle over the reference's frames %.3e"
                   % (fx.name, what, precision, rep, err))
            assert torch.equal(out, plain), (precision, rep)
            assert err < GATE, (precision, rep, err)
        assert torch.equal(m.inference(seq_len, data, noise=noise), plain)     # and back: the flag is part of the graph key


@pytest.mark.parametrize("name", FIXTURES)
def test_inference_nll_matches_oracle_and_leaves_frames_alone(name, gpu_device):
    fx = Fixture(name)
    _check_parity(fx, build(fx, gpu_device), gpu_device, "")


@pytest.mark.parametrize("name", FIXTURES)
def test_inference_nll_matches_the_engines_forward_nll(name, gpu_device):
    """Feeding the generated sequence back through SeqGlow.forward gives the same per-frame NLL (itself gated against the oracle)."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, seq_len = _infer_case(fx, gpu_device)
    out, nll = m.inference(seq_len, data, noise=noise, return_nll=True)
    batch = {k: v[:, :seq_len].contiguous() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}
    batch["p1_face"] = torch.cat([data["p1_face"][:, :fx.start], out], 1).contiguous()
    if fx.hp["Conditioning"]["use_frame_nb"]:
        batch["frame_nb"] = torch.full((fx.B, 1), 1.0 - 2 * fx.start, device=gpu_device)
    with torch.no_grad():
        _, _, losses = m(batch)
    err = max_rel(nll, torch.stack(losses), floor=1.0)
    report("%s: sampler NLL vs forward() over the generated sequence: max rel diff %.3e" % (name, err))
    assert err < GATE


@pytest.mark.parametrize("name", FIXTURES)
def test_stream_nll_matches_oracle_inference_and_a_session_without_it(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data, noise, seq_len = _infer_case(fx, gpu_device)
    _, expected = fixture_expected(fx)
    N = noise.shape[0]
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        with m.open_stream(_seed(data, fx.start)) as st:
            assert st.return_nll is False
            plain = torch.stack([st.step(_frame(data, fx.start + n), noise[n]) for n in range(N)], 1)
        with m.open_stream(_seed(data, fx.start), return_nll=True) as st:
            assert st.return_nll is True
            steps = [st.step(_frame(data, fx.start + n), noise[n]) for n in range(N)]
            assert st.replays > 0
            replays = st.replays
        out, nll = torch.stack([f for f, _ in steps], 1), torch.stack([q for _, q in steps])
        assert all(tuple(q.shape) == (fx.B,) and q.dtype == torch.float32 for _, q in steps)
        assert torch.equal(out, plain), precision
        err = max_rel(nll, expected, floor=1.0)
        err_replayed = max_rel(nll[N - replays:], expected[N - replays:], floor=1.0)
        inf, inf_nll = m.inference(seq_len, data, noise=noise, return_nll=True)
        same = torch.equal(out, inf)
        report("%s stream (%s): NLL max rel err vs fp64 oracle %.3e (replayed steps %.3e); frames bit-identical to inference(): %s; "
               "NLL vs inference()'s max rel diff %.3e" % (name, precision, err, err_replayed, same, max_rel(nll, inf_nll, floor=1.0)))
        assert err < GATE and err_replayed < GATE, (precision, err, err_replayed)
        if same:
            assert torch.equal(nll, inf_nll), precision


def test_stream_rows_report_their_own_nll(gpu_device):
    """reset_rows mid-session: the reseeded row's NLL is a fresh session's on that seed, the other rows' are an undisturbed session's
    bit for bit. A branch gives equal NLL under equal noise, and under different noise nll.argmin() is the oracle's choice."""
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data, noise, _ = _infer_case(fx, gpu_device)
    start, N, B = fx.start, noise.shape[0], fx.B
    with m.open_stream(_seed(data, start), return_nll=True) as st:
        undisturbed = torch.stack([st.step(_frame(data, start + n), noise[n])[1] for n in range(N)])
    r, s0 = 2, 5
    others = [b for b in range(B) if b != r]
    with m.open_stream(_seed(data, start), return_nll=True) as st:
        got = []
        for n in range(N):
            fr, nz = _frame(data, start + n), noise[n].clone()
            if n == s0:
                st.reset_rows([r], {k: v[r:r + 1].contiguous() for k, v in _seed(data, start).items()})
            if n >= s0:       # row r lives its sequence again from the start: its own frames and noise of step n - s0
                for k, v in _frame(data, start + n - s0).items():
                    fr[k][r] = v[r]
                nz[r] = noise[n - s0, r]
            got.append(st.step(fr, nz)[1])
        got = torch.stack(got)
    err = max_rel(got[s0:, r], undisturbed[:N - s0, r], floor=1.0)
    report("tiny stream: NLL of a row reseeded after %d steps vs a fresh session on its seed: max rel diff %.3e" % (s0, err))
    assert err < GATE
    assert torch.equal(got[:, others], undisturbed[:, others])
    assert torch.equal(got[:s0], undisturbed[:s0])

    # ---- branch: row 0 after s0 steps into rows 1 and 2, stepped with row 0's conditioning
    a, b = 1, 2
    with m.open_stream(_seed(data, start), return_nll=True) as st:
        hist = [st.step(_frame(data, start + n), noise[n])[0] for n in range(s0)]
        saved = st.save_rows([0])
        fr = {k: v.clone() for k, v in _frame(data, start + s0).items()}
        for v in fr.values():
            v[a], v[b] = v[0], v[0]
        st.load_rows([a, b], saved, entries=[0, 0])
        nz = noise[s0].clone()
        nz[a], nz[b] = nz[0], nz[0]
        x, q = st.step(fr, nz)
        assert torch.equal(x[a], x[b]) and torch.equal(x[a], x[0])
        assert torch.equal(q[a], q[b]) and torch.equal(q[a], q[0])
        # ---- best of two: the same branch again, now with different noise in the two rows
        st.load_rows([a, b], saved, entries=[0, 0])
        g = torch.Generator().manual_seed(17)
        nz[a], nz[b] = (torch.randn(2, fx.C, generator=g) * 0.8).to(gpu_device)
        x, q = st.step(fr, nz)
    # the oracle's NLL of both continuations: row 0's conditioning and generated history, then candidate a / candidate b
    past = torch.stack(hist, 1)[0:1].cpu()
    frames = torch.cat([past.expand(2, -1, -1), torch.stack([x[a], x[b]]).cpu().unsqueeze(1)], 1)
    data2 = {k: v[0:1].expand(2, *v.shape[1:]).cpu() for k, v in data.items() if v.dim() == 3}
    z, expected = teacher_forced(fx.hp, fx.state_dict(), data2, frames, start)
    got2 = torch.stack([q[a], q[b]]).cpu()
    err = max_rel(got2, expected[-1], floor=1.0)
    report("tiny stream best-of-2: NLL of the two candidates %s, oracle %s (max rel err %.3e); z recovered to %.2e"
           % (got2.tolist(), expected[-1].tolist(), err, float((z[-1] - torch.stack([nz[a], nz[b]]).cpu().double()).abs().max())))
    assert err < GATE
    assert int(got2.argmin()) == int(expected[-1].argmin())
    assert abs(float(expected[-1][0] - expected[-1][1])) > 1e-2      # (a choice the gate can tell apart)


@pytest.mark.parametrize("switch", ["LFI_SAMPLE_CHAIN=0", "LFI_FLOW_GENERIC=1", "LFI_NO_GRAPH=1"])
@pytest.mark.parametrize("name", ["tiny", "tiny_lstm"])
def test_inference_nll_on_every_sampler_path(name, switch, gpu_device, monkeypatch):
    """The per-step launches of the fast cell, the generic cell, and eager launches of the chain."""
    key, value = switch.split("=")
    monkeypatch.setenv(key, value)
    fx = Fixture(name)
    _check_parity(fx, build(fx, gpu_device), gpu_device, " [%s]" % switch)


@pytest.mark.parametrize("wfrag16", ["1", "0"])
def test_inference_nll_on_the_three_product_cells_at_final_widths(wfrag16, gpu_device, monkeypatch):
    """Final widths (whole 32-k blocks everywhere) in bf16x3: the reverse cell in three fp16 products, with the weights' fragment
    images lfi_flow_prep left (the default) and - LFI_SAMPLE_WFRAG16=0 - splitting the f32 fragments itself. K = 4, batch 20 (a
    partial second row tile), 6 generated frames; expected: the fp64 oracle's NLL of the frames the GPU generated."""
    monkeypatch.setenv("LFI_SAMPLE_WFRAG16", wfrag16)
    hp = final_model_hparams(50, 27, K=4)
    m, sd = perturbed_model(hp, gpu_device)
    m.eval()
    m.precision = "bf16x3"
    B, frames = 20, 6
    g = torch.Generator().manual_seed(7)
    data = {"p1_face": torch.randn(B, 24, 50, generator=g)}
    for name, d in (("p2_face", 50), ("p1_speech", 27), ("p2_speech", 27)):
        data[name] = torch.randn(B, 24 + frames, d, generator=g)
    noise = torch.randn(frames, B, 50, generator=g) * 0.8
    plain = m.inference(24 + frames, to_dev(data, gpu_device), noise=noise.to(gpu_device))
    for rep in range(2):
        out, nll = m.inference(24 + frames, to_dev(data, gpu_device), noise=noise.to(gpu_device), return_nll=True)
        assert torch.equal(out, plain)
        _, expected = teacher_forced(hp, sd, data, out.cpu(), 24)
        err = max_rel(nll, expected, floor=1.0)
        report("final widths, K=4, batch 20 x 6 frames (bf16x3, LFI_SAMPLE_WFRAG16=%s, call %d): sampler NLL max rel err vs the fp64 "
               "oracle's NLL of the GPU's frames %.3e" % (wfrag16, rep, err))
        assert err < GATE


def test_inference_nll_at_full_depth_against_oracle(gpu_device):
    """final_model widths, K = 16, batch 8, 56 generated frames (the case of tests/test_gpu_headline_parity.py's
    test_k16_sampling_against_oracle). Through 56 autoregressive frames the GPU's frames drift from the oracle's (2.6e-5 there), so the
    expected values are the fp64 oracle's teacher-forced NLL of the frames the GPU generated; the distance to the oracle's NLL of its
    own frames - how far that drift moves a likelihood - is reported without a gate."""
    hp = final_model_hparams(50, 27, K=16)
    m, sd = perturbed_model(hp, gpu_device)
    m.eval()
    B, seq_len = 8, 24 + 56
    g = torch.Generator().manual_seed(3)
    data = {"p1_face": torch.randn(B, 24, 50, generator=g)}
    for name, d in (("p2_face", 50), ("p1_speech", 27), ("p2_speech", 27)):
        data[name] = torch.randn(B, seq_len, d, generator=g)
    noise = torch.randn(seq_len - 24, B, 50, generator=g) * 0.8
    threads = torch.get_num_threads()
    torch.set_num_threads(min(8, threads))
    try:
        ref = oracle.seqglow_inference(hp, {k: v.double() for k, v in sd.items()}, seq_len,
                                       {k: v.double() for k, v in data.items()}, noise.double())
        _, own_nll = teacher_forced(hp, sd, data, ref, 24)
        for precision in ("f32", "bf16x3"):
            m.precision = precision
            plain = m.inference(seq_len, to_dev(data, gpu_device), noise=noise.to(gpu_device))
            out, nll = m.inference(seq_len, to_dev(data, gpu_device), noise=noise.to(gpu_device), return_nll=True)
            out2, nll2 = m.inference(seq_len, to_dev(data, gpu_device), noise=noise.to(gpu_device), return_nll=True)   # hipGraph replay
            z, expected = teacher_forced(hp, sd, data, out.cpu(), 24)
            err = max_rel(nll, expected, floor=1.0)
            drift = max_rel(nll, own_nll, floor=1.0)
            report("K=16 sampling NLL, batch 8 x 56 generated frames (%s): max rel err vs the fp64 oracle's NLL of the GPU's frames "
                   "%.3e (gate %.0e; oracle recovers z to %.2e); vs the oracle's NLL of its own frames %.3e (frames apart by %.2e, "
                   "no gate); NLL in [%.1f, %.1f] bits"
                   % (precision, err, GATE, float((z - noise.double()).abs().max()), drift,
                      float((out.cpu().double() - ref).abs().max()), float(expected.min()), float(expected.max())))
            assert torch.equal(out, plain) and torch.equal(out, out2) and torch.equal(nll, nll2), precision
            assert err < GATE, (precision, err)
    finally:
        torch.set_num_threads(threads)
