"""GPU: streaming frame-by-frame sampling (SeqGlow.open_stream -> engine.SampleStream) against SeqGlow.inference, the golden
fixtures and the fp64 oracle; graph replay against eager launches; isolation from other engine work between steps; the caller on
the legacy default stream; no host synchronisation in a steady-state step; frozen weights; the range guard; input validation."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, report
from oracle import seqglow_oracle as oracle
from test_gpu_parity import build, final_model_hparams, perturbed_model, to_dev

pytestmark = pytest.mark.gpu


def _seed(data, start):
    return {k: v[:, :start].contiguous() for k, v in data.items() if v.dim() == 3}


def _frame(data, t):
    return {k: v[:, t].contiguous() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}


def _run(st, data, noise, start, first=0, last=None):
    last = noise.shape[0] if last is None else last
    return torch.stack([st.step(_frame(data, start + n), noise[n]) for n in range(first, last)], 1)


def _stream(m, data, noise, start):
    with m.open_stream(_seed(data, start)) as st:
        return _run(st, data, noise, start)


def _final_setup(device, B, frames, K=4, seed=3):
    hp = final_model_hparams(50, 27, K=K)
    m, sd = perturbed_model(hp, device)
    m.eval()
    g = torch.Generator().manual_seed(seed)
    seq_len = 24 + frames
    data = {"p1_face": torch.randn(B, 24, 50, generator=g)}
    for name, d in (("p2_face", 50), ("p1_speech", 27), ("p2_speech", 27)):
        data[name] = torch.randn(B, seq_len, d, generator=g)
    noise = torch.randn(frames, B, 50, generator=g) * 0.8
    return hp, m, sd, data, noise, seq_len


@pytest.mark.parametrize("name", FIXTURES)
def test_stream_matches_fixture_and_inference(name, gpu_device):
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    noise = fx.get("infer/noise", torch.float32).to(gpu_device)
    seq_len = int(fx.get("infer/seq_len"))
    ref = fx.get("infer/out")
    for precision in ("f32", "bf16x3"):
        m.precision = precision
        out = _stream(m, data, noise, fx.start)
        assert tuple(out.shape) == tuple(ref.shape)
        err = (out.double().cpu() - ref).abs().max().item()
        inf = m.inference(seq_len, data, noise=noise)
        err_inf = (out - inf).abs().max().item()
        report("%s stream (%s): max abs err vs fp64 reference %.3e, vs inference() %.3e" % (name, precision, err, err_inf))
        assert err < 1e-5 and err_inf < 1e-5, (precision, err, err_inf)


def test_stream_with_injected_dropout_masks_matches_inference(gpu_device):
    """Train mode: a step takes its masks from _draw_masks(B, 1); injected (N, B, hist) masks give frame n's row to step n."""
    fx = Fixture("p1enc")
    m = build(fx, gpu_device, train=True)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    noise = fx.get("infer/noise", torch.float32).to(gpu_device)
    N, B = noise.shape[0], noise.shape[1]
    g = torch.Generator().manual_seed(5)
    m.injected_masks = {e.name: ((torch.rand(N, B, e.hist, generator=g) < 0.6).float() / 0.6)
                        for e in m.spec.encoders if e.dropout > 0 and e.name != "p1_face"}
    ref = m.inference(int(fx.get("infer/seq_len")), data, noise=noise)
    out = _stream(m, data, noise, fx.start)
    assert (out - ref).abs().max().item() < 1e-5


def test_stream_headline_size_against_oracle(gpu_device):
    """final_model widths at K = 16, B = 64, 56 streamed frames, bf16x3, against the fp64 oracle with the gate of
    tests/test_gpu_headline_parity.py's inference test: max(1e-5, 1.5 x the plain-fp32 oracle error)."""
    hp, m, sd, data, noise, seq_len = _final_setup(gpu_device, 64, 56, K=16)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    ref = oracle.seqglow_inference(hp, {k: v.double() for k, v in sd.items()}, seq_len,
                                   {k: v.double() for k, v in data.items()}, noise.double())
    ref32 = oracle.seqglow_inference(hp, sd, seq_len, data, noise)
    torch.set_num_threads(threads)
    own = float((ref32.double() - ref).abs().max())
    gate = max(1e-5, 1.5 * own)
    m.precision = "bf16x3"
    out = _stream(m, to_dev(data, gpu_device), noise.to(gpu_device), 24)
    err = float((out.cpu().double() - ref).abs().max())
    report("K=16 streaming, batch 64 x 56 frames (bf16x3): max abs err vs fp64 oracle %.2e; plain fp32 torch %.2e; gate %.2e"
           % (err, own, gate))
    assert err <= gate, (err, gate)


def test_stream_graph_replay_is_bit_identical_to_eager(gpu_device, monkeypatch):
    for precision in ("bf16x3", "f32"):
        _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 7)
        m.precision = precision
        data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
        with m.open_stream(_seed(data, 24)) as st:
            out = _run(st, data, noise, 24)
            assert st.steps == 7 and st.replays == 6     # step 1 eager, steps 2.. one replayed graph
        monkeypatch.setenv("LFI_NO_GRAPH", "1")
        with m.open_stream(_seed(data, 24)) as st:
            eager = _run(st, data, noise, 24)
            assert st.replays == 0
        monkeypatch.delenv("LFI_NO_GRAPH")
        assert torch.equal(out, eager), precision
        # reset() starts the sequence again and keeps the graph
        with m.open_stream(_seed(data, 24)) as st:
            a = _run(st, data, noise, 24, 0, 3)
            st.reset(_seed(data, 24))
            b = _run(st, data, noise, 24)
        assert torch.equal(torch.cat([a], 1), out[:, :3]) and torch.equal(b, out)


def test_stream_is_isolated_from_other_engine_work(gpu_device):
    _, m, _, data, noise, seq_len = _final_setup(gpu_device, 8, 6)
    m.precision = "bf16x3"
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    ref = _stream(m, data, noise, 24)
    fx = Fixture("tiny")
    other = build(fx, gpu_device, train=True)
    other.injected_masks = fx.masks(torch.float32)
    batch = to_dev(fx.batch(), gpu_device)
    sub = {k: v[:3].contiguous() for k, v in data.items()}
    with m.open_stream(_seed(data, 24)) as st:
        outs = []
        for n in range(noise.shape[0]):
            outs.append(st.step(_frame(data, 24 + n), noise[n]))
            m.inference(seq_len, sub, noise=noise[:, :3].contiguous())        # another batch size on the same engine
            _, loss, _ = other(batch)                                          # training forward + backward on another model
            loss.sum().backward()
    assert torch.equal(torch.stack(outs, 1), ref)
    # two sessions of different batch sizes on one model, stepped in turns
    d5, n5 = {k: v[:5].contiguous() for k, v in data.items()}, noise[:, :5].contiguous()
    ref5 = _stream(m, d5, n5, 24)
    with m.open_stream(_seed(data, 24)) as a, m.open_stream(_seed(d5, 24)) as b:
        oa, ob = [], []
        for n in range(noise.shape[0]):
            oa.append(a.step(_frame(data, 24 + n), noise[n]))
            ob.append(b.step(_frame(d5, 24 + n), n5[n]))
    assert torch.equal(torch.stack(oa, 1), ref) and torch.equal(torch.stack(ob, 1), ref5)


def test_stream_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 5)
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    on_default = _stream(m, data, noise, 24)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        on_side = _stream(m, data, noise, 24)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default, on_side)


def test_stream_steady_state_steps_do_not_synchronise(gpu_device):
    _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 8)
    m.precision = "bf16x3"
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    frames = [_frame(data, 24 + n) for n in range(8)]
    with m.open_stream(_seed(data, 24)) as st:
        st.step(frames[0], noise[0])
        st.step(frames[1], noise[1])          # (the capture synchronises once)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for n in range(2, 6):
                st.step(frames[n], noise[n])
            for n in range(6, 8):
                st.step(frames[n])            # noise drawn by the session
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 7


def test_stream_refuses_to_step_after_parameter_changes(gpu_device):
    fx = Fixture("tiny")
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    st = m.open_stream(_seed(data, fx.start))
    st.step(_frame(data, fx.start))
    m.engine.optimizer_step(1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step(_frame(data, fx.start + 1))
    st = m.open_stream(_seed(data, fx.start))
    st.step(_frame(data, fx.start))
    m.load_state_dict(fx.state_dict(torch.float32))
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.step(_frame(data, fx.start + 1))
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.step(_frame(data, fx.start + 1))


def test_stream_range_guard_falls_back_to_six_bf16_products(gpu_device):
    hp, m, _, data, noise, _ = _final_setup(gpu_device, 8, 8, seed=11)
    m.precision = "bf16x3"
    data = to_dev(data, gpu_device)
    noise = noise.to(gpu_device)
    bad = {k: v.clone() for k, v in data.items()}
    bad["p2_speech"][0, 24 + 2, 5] = 1.0e5          # beyond fp16's range, in a GRU-encoded modality
    eng = m._ensure_engine(gpu_device)
    eng.sample_frame_precision = 5
    try:
        ref = _stream(m, bad, noise, 24)           # six bf16 products from the open
    finally:
        eng.sample_frame_precision = None
    with m.open_stream(_seed(bad, 24)) as st:
        assert st.frame_precision == 9
        outs = [st.step(_frame(bad, 24 + n), noise[n]) for n in range(3)]
        torch.cuda.synchronize()                   # (the guard's copy has landed: the next step reads it)
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            outs.append(st.step(_frame(bad, 27), noise[3]))
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            outs += [st.step(_frame(bad, 24 + n), noise[n]) for n in range(4, 8)]
    out = torch.stack(outs, 1)
    assert torch.isfinite(out).all()
    scale = max(float(ref.abs().max()), 1.0)
    assert float((out[:, 3:] - ref[:, 3:]).abs().max()) <= 2e-5 * scale


def test_stream_validates_inputs_before_any_launch(gpu_device):
    fx = Fixture("framenb")
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    noise = fx.get("infer/noise", torch.float32).to(gpu_device)
    ref = _stream(m, data, noise, fx.start)
    seed = _seed(data, fx.start)
    with pytest.raises(ValueError, match="T>=4"):
        m.open_stream({k: v[:, :fx.start - 1].contiguous() for k, v in seed.items()})
    with pytest.raises(KeyError, match="p2_speech"):
        m.open_stream({k: v for k, v in seed.items() if k != "p2_speech"})
    with pytest.raises(ValueError, match="p2_face"):
        m.open_stream(dict(seed, p2_face=seed["p2_face"].double()))
    with m.open_stream(seed) as st:
        outs = []
        for n in range(noise.shape[0]):
            fr = _frame(data, fx.start + n)
            if n == 2:
                with pytest.raises(KeyError, match="p1_speech"):
                    st.step({k: v for k, v in fr.items() if k != "p1_speech"}, noise[n])
                with pytest.raises(ValueError, match="p2_face"):
                    st.step(dict(fr, p2_face=fr["p2_face"][:3].contiguous()), noise[n])
                with pytest.raises(ValueError, match="p2_face"):
                    st.step(dict(fr, p2_face=fr["p2_face"].cpu()), noise[n])
                with pytest.raises(ValueError, match="p2_speech"):
                    st.step(dict(fr, p2_speech=fr["p2_speech"].half()), noise[n])
                with pytest.raises(ValueError, match="noise"):
                    st.step(fr, noise[n][:, :3])
                assert st.steps == 2
            outs.append(st.step(fr, noise[n]))
    assert torch.equal(torch.stack(outs, 1), ref)
