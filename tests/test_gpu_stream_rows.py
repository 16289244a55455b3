"""GPU: reseeding single batch rows of a streaming sampling session (SampleStream.reset_rows -> lfi_stream_reset_rows) - the other
rows carry on bit for bit, a reseeded row is bit for bit a fresh session's row, every golden fixture against inference(), all rows
against reset(), no host synchronisation, the range guard, validation before any launch, and the caller's stream."""
import warnings

import pytest
import torch

from helpers import FIXTURES, Fixture, report
from test_gpu_parity import build, to_dev
from test_gpu_stream import _final_setup, _frame, _run, _seed, _stream

pytestmark = pytest.mark.gpu


def _conversations(device, n, frames, seed=17):
    """n new conversations at _final_setup's widths: 24 seed frames of p1_face, 24 + frames of the other modalities, their noise."""
    g = torch.Generator().manual_seed(seed)
    data = {"p1_face": torch.randn(n, 24, 50, generator=g)}
    for name, d in (("p2_face", 50), ("p1_speech", 27), ("p2_speech", 27)):
        data[name] = torch.randn(n, 24 + frames, d, generator=g)
    noise = torch.randn(frames, n, 50, generator=g) * 0.8
    return to_dev(data, device), noise.to(device)


def _rows_of(d, rows):
    return {k: v[rows].contiguous() for k, v in d.items()}


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_reset_rows_leaves_other_rows_alone_and_equals_a_fresh_start(precision, gpu_device):
    _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 10)
    m.precision = precision
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    rows, at = [2, 5], 4
    new, new_noise = _conversations(gpu_device, 2, 10 - at)

    def mixed(n):
        """Frame n of the session after the reseed: rows 2 and 5 get the new conversations' frame n - at and their noise."""
        fr, nf = _frame(data, 24 + n), _frame(new, 24 + n - at)
        for k in fr:
            fr[k][rows] = nf[k]
        nz = noise[n].clone()
        nz[rows] = new_noise[n - at]
        return fr, nz

    ref = _stream(m, data, noise, 24)
    with m.open_stream(_seed(data, 24)) as st:
        outs = [st.step(_frame(data, 24 + n), noise[n]) for n in range(at)]
        st.reset_rows(rows, _seed(new, 24))
        outs += [st.step(*mixed(n)) for n in range(at, 10)]
        assert st.steps == 10 and st.replays == 9
    out = torch.stack(outs, 1)
    keep = [b for b in range(8) if b not in rows]
    assert torch.equal(out[keep], ref[keep]), precision
    # a session opened with the new conversations in rows 2 and 5 from the start
    seed = _seed(data, 24)
    for k, v in _seed(new, 24).items():
        seed[k][rows] = v
    with m.open_stream(seed) as st:
        fresh = torch.stack([st.step(*mixed(n)) for n in range(at, 10)], 1)
    assert torch.equal(out[rows, at:], fresh[rows]), precision


@pytest.mark.parametrize("name", FIXTURES)
def test_reset_rows_matches_fixture_inference(name, gpu_device):
    """Open, step 2 frames, reseed a strict subset of rows with the fixture's own seed and step the fixture's frames again: the
    reseeded rows give inference() (the gate of test_stream_matches_fixture_and_inference), the others an undisturbed session's
    frames bit for bit. tiny_lstm resets the cell state, framenb the frame counter."""
    fx = Fixture(name)
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    noise = fx.get("infer/noise", torch.float32).to(gpu_device)
    seq_len = int(fx.get("infer/seq_len"))
    B = noise.shape[1]
    rows = list(range(B - 1, 0, -2))       # strict subset, listed out of order
    keep = [b for b in range(B) if b not in rows]
    seed = _seed(data, fx.start)
    for precision, row_arg in (("f32", rows), ("bf16x3", torch.tensor(rows))):
        m.precision = precision
        inf = m.inference(seq_len, data, noise=noise)
        with m.open_stream(seed) as st, m.open_stream(seed) as undisturbed:
            for n in range(2):
                st.step(_frame(data, fx.start + n), noise[n])
                undisturbed.step(_frame(data, fx.start + n), noise[n])
            st.reset_rows(row_arg, _rows_of(seed, rows))
            out = _run(st, data, noise, fx.start)
            other = _run(undisturbed, data, noise, fx.start)
        err = (out[rows] - inf[rows]).abs().max().item()
        report("%s stream, rows %s reseeded after 2 frames (%s): max abs err vs inference() %.3e" % (name, rows, precision, err))
        assert err < 1e-5, (precision, err)
        assert torch.equal(out[keep], other[keep]), precision


@pytest.mark.parametrize("precision", ("f32", "bf16x3"))
def test_reset_rows_of_every_row_equals_reset(precision, gpu_device):
    _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 6)
    m.precision = precision
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    new, new_noise = _conversations(gpu_device, 8, 4)
    nseed = _seed(new, 24)
    with m.open_stream(_seed(data, 24)) as st:
        _run(st, data, noise, 24, 0, 2)
        st.reset(nseed)
        want = torch.stack([st.step(_frame(new, 24 + n), new_noise[n]) for n in range(4)], 1)
    perm = [3, 0, 7, 1, 6, 2, 5, 4]             # entry j -> row perm[j]: row r gets conversation r again
    with m.open_stream(_seed(data, 24)) as st:
        _run(st, data, noise, 24, 0, 2)
        graph = st._graph
        st.reset_rows(perm, _rows_of(nseed, perm))
        got = torch.stack([st.step(_frame(new, 24 + n), new_noise[n]) for n in range(4)], 1)
        assert st._graph is graph and st.steps == 6 and st.replays == 5
    assert torch.equal(got, want), precision


def test_reset_rows_do_not_synchronise(gpu_device):
    """Reseeds between steady-state steps, one of them of more rows than one launch carries (256): no host synchronisation, and
    the split list still gives reset()'s frames."""
    B = 300
    _, m, _, data, noise, _ = _final_setup(gpu_device, B, 8)
    m.precision = "bf16x3"
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    new, _ = _conversations(gpu_device, B, 8)
    nseed = _seed(new, 24)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(2)).tolist()
    pseed = _rows_of(nseed, perm)
    few = _rows_of(nseed, [0, 1, 2])
    frames = [_frame(data, 24 + n) for n in range(8)]
    with m.open_stream(_seed(data, 24)) as st:
        st.step(frames[0], noise[0])
        st.step(frames[1], noise[1])          # (the capture synchronises once)
        torch.cuda.set_sync_debug_mode("error")
        try:
            st.reset_rows([17, 250, 299], few)
            st.step(frames[2], noise[2])
            st.reset_rows(torch.tensor([5, 9, 100]), few)
            st.step(frames[3])                # noise drawn by the session
            st.reset_rows(perm, pseed)
            got = [st.step(frames[n], noise[n]) for n in range(4, 8)]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert st.replays == 7
    with m.open_stream(_seed(data, 24)) as st:
        st.step(frames[0], noise[0])
        st.reset(nseed)
        want = [st.step(frames[n], noise[n]) for n in range(4, 8)]
    assert torch.equal(torch.stack(got, 1), torch.stack(want, 1))


def test_reset_rows_range_guard(gpu_device):
    _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 8, seed=11)
    m.precision = "bf16x3"
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    new, _ = _conversations(gpu_device, 2, 8)
    good = _seed(new, 24)
    bad = {k: v.clone() for k, v in good.items()}
    bad["p2_speech"][1, 23, 5] = 1.0e5           # beyond fp16's range, in the newest frame of a GRU-encoded window
    with m.open_stream(_seed(data, 24)) as st:
        assert st.frame_precision == 9
        st.step(_frame(data, 24), noise[0])
        st.step(_frame(data, 25), noise[1])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            st.reset_rows([1, 6], good)
            st.step(_frame(data, 26), noise[2])
            torch.cuda.synchronize()
            st.step(_frame(data, 27), noise[3])  # (reads the guard behind the reseed: within range)
        assert st.frame_precision == 9
        st.reset_rows([6, 1], bad)
        st.step(_frame(data, 28), noise[4])      # its advance copies the guard, which now holds 1e5
        torch.cuda.synchronize()
        with pytest.warns(RuntimeWarning, match="six bf16 products"):
            outs = [st.step(_frame(data, 29), noise[5])]
        assert st.frame_precision == 5
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            outs += [st.step(_frame(data, 24 + n), noise[n]) for n in (6, 7)]
    assert torch.isfinite(torch.stack(outs, 1)).all()


def test_reset_rows_validates_before_any_launch(gpu_device):
    fx = Fixture("framenb")
    m = build(fx, gpu_device)
    data = to_dev(fx.group("infer/data/"), gpu_device)
    noise = fx.get("infer/noise", torch.float32).to(gpu_device)
    ref = _stream(m, data, noise, fx.start)
    seed = _seed(data, fx.start)
    sub = _rows_of(seed, [1, 3])
    bad_calls = (
        ([1, 1], sub, ValueError, "more than once"),
        ([1, 4], sub, ValueError, "outside"),
        ([-1, 2], sub, ValueError, "outside"),
        ([], sub, ValueError, "empty"),
        ([0.5, 1], sub, ValueError, "rows"),
        (torch.tensor([1, 3], device=gpu_device), sub, ValueError, "rows"),
        (torch.tensor([1.0, 3.0]), sub, ValueError, "rows"),
        ([1], sub, ValueError, "p1_face"),                                          # len(rows) != the seed's batch
        ([1, 3], {k: v for k, v in sub.items() if k != "p2_speech"}, KeyError, "p2_speech"),
        ([1, 3], {k: v for k, v in sub.items() if k != "p1_face"}, KeyError, "p1_face"),
        ([1, 3], dict(sub, p2_face=sub["p2_face"].cpu()), ValueError, "p2_face"),
        ([1, 3], dict(sub, p1_speech=sub["p1_speech"].double()), ValueError, "p1_speech"),
        ([1, 3], dict(sub, p2_face=sub["p2_face"].transpose(0, 1).contiguous().transpose(0, 1)), ValueError, "p2_face"),
        ([1, 3], dict(sub, p2_speech=sub["p2_speech"][:, :fx.start - 1].contiguous()), ValueError, "T>=4"),
        ([1, 3], dict(sub, p1_face=sub["p1_face"][..., :-1].contiguous()), ValueError, "p1_face"),
    )
    with m.open_stream(seed) as st:
        outs = [st.step(_frame(data, fx.start + n), noise[n]) for n in range(2)]
        for rows, s, exc, text in bad_calls:
            with pytest.raises(exc, match=text):
                st.reset_rows(rows, s)
        assert st.steps == 2
        outs += [st.step(_frame(data, fx.start + n), noise[n]) for n in range(2, noise.shape[0])]
    assert torch.equal(torch.stack(outs, 1), ref)
    # a session whose weights changed, and a closed one
    st = m.open_stream(seed)
    st.step(_frame(data, fx.start))
    m.load_state_dict(fx.state_dict(torch.float32))
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.reset_rows([1, 3], sub)
    st.close()
    st = m.open_stream(seed)
    st.close()
    with pytest.raises(RuntimeError, match="closed"):
        st.reset_rows([1, 3], sub)


def test_reset_rows_caller_on_legacy_default_stream_and_on_its_own(gpu_device):
    _, m, _, data, noise, _ = _final_setup(gpu_device, 8, 6)
    data, noise = to_dev(data, gpu_device), noise.to(gpu_device)
    new, _ = _conversations(gpu_device, 3, 6)

    def run():
        with m.open_stream(_seed(data, 24)) as st:
            outs = []
            for n in range(6):
                if n == 2:
                    st.reset_rows([0, 4, 7], _seed(new, 24))      # (the seed is dropped at once)
                if n == 4:
                    st.reset_rows(torch.tensor([4]), _rows_of(_seed(new, 24), [1]))
                outs.append(st.step(_frame(data, 24 + n), noise[n]))
            return torch.stack(outs, 1)

    assert torch.cuda.current_stream(gpu_device) == torch.cuda.default_stream(gpu_device)
    on_default = run()
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        on_side = run()
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    assert torch.equal(on_default, on_side)
