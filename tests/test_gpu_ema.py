"""GPU: the running average of the weights (Polyak / EMA), from the kernel behind lfi_ema_update through the engine, the eager and
the captured training step, SeqGlow.ema_weights(), checkpoints and Trainer.validate. Reference: tests/ema_expected.py (fp64, the
coefficient rounded as the entry point rounds it); bound per element 5 * 2^-24 * max(|p|, |ema|), derived there."""
import copy
import math
import warnings
from argparse import Namespace

import pytest
import torch

from ema_expected import worst_ratio
from helpers import Fixture, report
from test_gpu_optimizers import CASES

pytestmark = pytest.mark.gpu

GUARD = 64            # floats of guard band on either side of each buffer (a multiple of 4: keeps the 16-byte alignment)
SENTINEL = 12345.0
PLACEMENTS = [(0, 0), (1, 0), (0, 3), (1, 3)]     # float offsets of (ema, p) from a 16-byte boundary


def _call(ema_ptr, p_ptr, n, decay):
    from lets_face_it_amd import _lib
    return _lib.lib().lfi_ema_update(ema_ptr, p_ptr, n, decay, torch.cuda.current_stream().cuda_stream)


def _spread(n, gen, device):
    """randn scaled across 1e-4 ... 1e2, element by element."""
    scale = 10.0 ** (torch.rand(n, generator=gen) * 6.0 - 4.0)
    return (torch.randn(n, generator=gen) * scale).to(device)


@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
@pytest.mark.parametrize("n", [0, 1, 3, 1027, 2 ** 20 + 5])
def test_kernel_through_the_c_abi(n, decay, gpu_device):
    gen = torch.Generator().manual_seed(1000 + n % 997)
    span = (n + 3) // 4 * 4 + 4      # room for the buffer at any offset 0..3
    for eoff, poff in PLACEMENTS:
        whole = torch.full((3 * GUARD + 2 * span,), SENTINEL, device=gpu_device)
        e0, p0 = GUARD + eoff, 2 * GUARD + span + poff
        ema_ptr, p_ptr = whole.data_ptr() + 4 * e0, whole.data_ptr() + 4 * p0      # (an empty slice reports no address)
        assert (ema_ptr % 16, p_ptr % 16) == (4 * eoff, 4 * poff)
        whole[e0:e0 + n] = _spread(n, gen, gpu_device)
        whole[p0:p0 + n] = _spread(n, gen, gpu_device)
        before = whole.clone()
        assert _call(ema_ptr, p_ptr, n, decay) == 0
        torch.cuda.synchronize()
        ratio = worst_ratio(whole[e0:e0 + n], before[e0:e0 + n], before[p0:p0 + n], decay)
        outside = torch.ones_like(whole, dtype=torch.bool)
        outside[e0:e0 + n] = False
        touched = int((whole[outside] != before[outside]).sum())
        report("lfi_ema_update n=%d decay=%g ema+%d p+%d floats: worst |err| / bound %.3f (bound 5 * 2^-24 * max(|p|, |ema|)); "
               "floats outside the average that changed: %d" % (n, decay, eoff, poff, ratio, touched))
        assert touched == 0, "guard bands or the parameters were written"
        assert ratio <= 1.0, ratio
        if n >= 1027:
            assert not torch.equal(whole[e0:e0 + n], before[e0:e0 + n]), "nothing was updated"


def test_kernel_refuses_bad_arguments_and_launches_nothing(gpu_device):
    from lets_face_it_amd import _lib
    L = _lib.lib()
    buf = torch.randn(256, device=gpu_device)
    before = buf.clone()
    ema, p = buf[:64], buf[128:192]
    bad = {
        "null ema": (None, p.data_ptr(), 64, 0.9),
        "null p": (ema.data_ptr(), None, 64, 0.9),
        "decay 1": (ema.data_ptr(), p.data_ptr(), 64, 1.0),
        "decay -0.5": (ema.data_ptr(), p.data_ptr(), 64, -0.5),
        "decay NaN": (ema.data_ptr(), p.data_ptr(), 64, float("nan")),
        "same range": (ema.data_ptr(), ema.data_ptr(), 64, 0.9),
        "p inside ema": (ema.data_ptr(), ema.data_ptr() + 4 * 63, 64, 0.9),
        "ema inside p": (p.data_ptr() + 4, p.data_ptr(), 64, 0.9),
        "n < 0": (ema.data_ptr(), p.data_ptr(), -1, 0.9),
    }
    for what, args in bad.items():
        rc = _call(*args)
        msg = L.lfi_last_error()
        assert rc != 0, what
        assert msg and b"lfi_ema_update" in msg, (what, msg)
    torch.cuda.synchronize()
    assert torch.equal(buf, before), "a refused call wrote"
    # adjacent ranges do not overlap; n == 0 succeeds with any pointers
    assert _call(ema.data_ptr(), ema.data_ptr() + 4 * 64, 64, 0.9) == 0
    assert _call(None, None, 0, 0.9) == 0
    torch.cuda.synchronize()


def _module(fx_name, gpu_device, name="adam", kwargs=None, ema_decay=None, validation=None):
    """The module of test_gpu_optimizers (fixture weights, injected masks, exact-f32 GEMMs), with Optim.ema_decay."""
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    fx = Fixture(fx_name)
    hp = Namespace(**copy.deepcopy(fx.hp))
    hp.Train["use_negative_nll_loss"] = False
    hp.gradient_clip_val = 5.0
    hp.Optim["name"] = name
    hp.Optim["args"][name] = dict(kwargs if kwargs is not None else {"betas": [0.9, 0.9999], "eps": 1e-8})
    if ema_decay is not None:
        hp.Optim["ema_decay"] = ema_decay
    if validation:
        hp.Validation.update(validation)
    hp.engine_precision = "f32"
    lm = LetsFaceItGlow(hp)
    lm.seq_glow.load_state_dict(fx.state_dict(torch.float32))
    lm.to(gpu_device)
    lm.seq_glow.glow.set_actnorm_init(True)
    lm.train()
    lm.seq_glow.injected_masks = {k: v.to(gpu_device) for k, v in fx.masks(torch.float32).items()} if fx.masks() else None
    return lm, {k: v.to(gpu_device) for k, v in fx.batch(torch.float32).items()}, fx


ONE_OF_EACH = [next(c for c in CASES if c[0] == name) for name in ("sgd", "rmsprop", "adam")]


@pytest.mark.parametrize("fx_name", ["tiny", "mid"])
@pytest.mark.parametrize("name,kwargs", ONE_OF_EACH, ids=[c[0] for c in ONE_OF_EACH])
def test_one_update_per_step_for_every_optimiser(fx_name, name, kwargs, gpu_device):
    lm, batch, _ = _module(fx_name, gpu_device, name, kwargs, ema_decay=0.99)
    eng = lm.seq_glow._ensure_engine(gpu_device)
    assert eng.ema is None and eng.ema_updates == 0
    prev, worst = None, 0.0
    for step in range(4):
        lm.fused_training_step(batch, 3e-3)
        assert eng.ema is not None and eng.ema.data_ptr() != eng.params.data_ptr() and eng.ema.numel() == eng.n_params
        if step == 0:
            assert torch.equal(eng.ema, eng.params), "the first average is a copy"
        else:
            assert not torch.equal(eng.params, prev_params), "the optimiser did not move the parameters"
            worst = max(worst, worst_ratio(eng.ema, prev, eng.params, 0.99))
        prev, prev_params = eng.ema.clone(), eng.params.clone()
    report("ema after fused %s steps on %s: worst |err| / bound over 3 updates %.3f" % (name, fx_name, worst))
    assert worst <= 1.0, worst
    assert eng.ema_updates == 4


def test_averaging_does_not_disturb_training(gpu_device):
    states = []
    for decay in (None, 0.99):
        lm, batch, _ = _module("tiny", gpu_device, ema_decay=decay)
        for _ in range(4):
            lm.fused_training_step(batch, 3e-3)
        eng = lm.seq_glow.engine
        assert (eng.ema is None) == (decay is None) and eng.ema_updates == (0 if decay is None else 4)
        states.append((eng.params.clone(), eng.grads.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
    for a, b, what in zip(states[0], states[1], ("params", "grads", "adam_m", "adam_v")):
        assert torch.equal(a, b), what


def test_captured_step_averages_like_the_eager_step(gpu_device):
    """step_graph on: steps 1 and 2 eager (the second makes the first lerp), from step 3 one replayed graph that holds the update
    behind Adam; against a module that launches everything eagerly, fed the same batches and the same dropout key."""
    fx = Fixture("tiny")
    gen = torch.Generator().manual_seed(5)
    base = fx.batch(torch.float32)
    batches = [{k: (v + 0.05 * i * torch.randn(v.shape, generator=gen)).to(gpu_device) for k, v in base.items()} for i in range(2)]
    runs, later, restarted = {}, {}, {}
    for graph in (False, True):
        torch.manual_seed(7)
        lm, _, _ = _module("tiny", gpu_device, ema_decay=0.99)
        lm.seq_glow.injected_masks = None      # (a captured step draws its own masks, keyed on the seed and the call counter)
        lm.step_graph = graph
        for i in range(6):
            lm.fused_training_step(batches[i % 2], 1e-3 * (1 + i % 2))
        eng = lm.seq_glow.engine
        graphs = [v for v in getattr(lm, "_step_graphs", {}).values() if isinstance(v, dict)]
        assert len(graphs) == (1 if graph else 0), "expected one captured step graph"
        assert not getattr(lm, "_step_graphs", {}).get("broken")
        runs[graph] = (eng.ema.clone(), eng.params.clone(), eng.ema_updates, eng.step_count)
        # training inside ema_weights() is refused before anything moves - also when the step would be a replay, which passes none of
        # the engine's own checks
        moments, version = (eng.adam_m.clone(), eng.adam_v.clone()), eng.param_version
        with lm.seq_glow.ema_weights():
            assert torch.equal(eng.params, runs[graph][0]) and torch.equal(eng.ema, runs[graph][1])
            for i in range(2):
                with pytest.raises(RuntimeError, match="averaged weights are swapped in"):
                    lm.fused_training_step(batches[i % 2], 1e-3)
            assert torch.equal(eng.params, runs[graph][0]) and torch.equal(eng.ema, runs[graph][1]), "a refused step wrote"
        assert torch.equal(eng.ema, runs[graph][0]) and torch.equal(eng.params, runs[graph][1])
        assert torch.equal(eng.adam_m, moments[0]) and torch.equal(eng.adam_v, moments[1])
        assert (eng.ema_updates, eng.step_count, lm.global_step, eng.param_version) == (6, 6, 6, version + 2)
        # a state load replaces the buffers a captured step holds by address: the graph must not go on writing the old average
        old = eng.ema
        eng.load_optimizer_state(eng.optimizer_state())
        assert eng.ema is not old and torch.equal(eng.ema, old)
        for i in range(6, 8):
            lm.fused_training_step(batches[i % 2], 1e-3 * (1 + i % 2))
        assert torch.equal(old, runs[graph][0]), "a step after the state load wrote the replaced buffer"
        assert len([v for v in getattr(lm, "_step_graphs", {}).values() if isinstance(v, dict)]) == (1 if graph else 0)
        later[graph] = (eng.ema.clone(), eng.params.clone(), eng.ema_updates)
        # a state without an average (an older checkpoint): the step that makes the first copy runs eagerly in both modes, counted
        state = eng.optimizer_state()
        state["ema"] = None
        eng.load_optimizer_state(state)
        assert eng.ema is None and eng.ema_updates == 0
        lm.fused_training_step(batches[0], 1e-3)
        assert torch.equal(eng.ema, eng.params) and eng.ema_updates == 1
        lm.fused_training_step(batches[1], 2e-3)
        lm.fused_training_step(batches[0], 1e-3)
        assert len([v for v in getattr(lm, "_step_graphs", {}).values() if isinstance(v, dict)]) == (1 if graph else 0)
        restarted[graph] = (eng.ema.clone(), eng.params.clone(), eng.ema_updates, eng.step_count)
    a, b = runs[False], runs[True]
    assert a[2] == b[2] == 6 and a[3] == b[3] == 6
    assert torch.equal(a[1], b[1]), "parameters differ between eager and replayed steps"
    assert torch.equal(a[0], b[0]), "the average differs between eager and replayed steps"
    assert not torch.equal(a[0], a[1])
    assert later[False][2] == later[True][2] == 8
    assert torch.equal(later[False][0], later[True][0]) and torch.equal(later[False][1], later[True][1])
    assert not torch.equal(later[True][0], b[0])
    assert restarted[False][2:] == restarted[True][2:] == (3, 11)
    assert torch.equal(restarted[False][0], restarted[True][0]) and torch.equal(restarted[False][1], restarted[True][1])
    assert not torch.equal(restarted[True][0], restarted[True][1])
    report("ema under hipGraph-replayed steps vs eager launches, 6 steps (4 replayed): average and parameters bit-identical")


def _nll(sg, batch):
    with torch.no_grad():
        return torch.stack(sg(batch)[2])


def test_ema_weights_context(gpu_device):
    from lets_face_it_amd.glow.models import SeqGlow
    lm, batch, fx = _module("tiny", gpu_device, ema_decay=0.9)
    sg = lm.seq_glow
    with pytest.raises(RuntimeError, match="no averaged weights"):
        with sg.ema_weights():
            pass
    for _ in range(3):
        lm.fused_training_step(batch, 3e-3)
    eng = sg.engine
    lm.eval()
    raw = {k: v.detach().clone() for k, v in sg.state_dict().items()}
    esd = sg.ema_state_dict()
    assert list(esd) == list(raw)
    changed = [k for k in raw if not torch.equal(raw[k], esd[k])]
    same = [k for k in raw if k not in changed]
    assert changed and all(k.endswith((".p", ".sign_s")) or not raw[k].is_floating_point() for k in same), same
    # reading the average out by name goes through the layout
    name = next(n for n in eng.layout if n.startswith("flow.w_hh"))
    assert torch.equal(eng.view(name, eng.ema).reshape(-1), eng.ema[eng.layout[name][0]:eng.layout[name][0] + eng.view(name).numel()])

    data = {k: v.to(gpu_device) for k, v in fx.group("infer/data/", torch.float32).items()}
    seed = {k: v[:, :fx.start].contiguous() for k, v in data.items() if v.dim() == 3}
    frame = {k: v[:, fx.start].contiguous() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}
    noise = torch.zeros(seed["p1_face"].shape[0], fx.C, device=gpu_device)
    masks, sg.injected_masks = sg.injected_masks, None      # (the fixture's masks are shaped for its training batch, not for a session)
    outer = sg.open_stream(seed)
    outer.step(frame, noise)

    version = eng.param_version
    with sg.ema_weights() as inside:
        assert inside is sg and eng.param_version == version + 1
        for k, v in sg.state_dict().items():
            assert torch.equal(v, esd[k]), k
        sg.injected_masks = masks
        nll_in = _nll(sg, batch)
        fresh = SeqGlow(Namespace(**copy.deepcopy(vars(lm.hparams))))
        fresh.load_state_dict(esd)
        fresh.to(gpu_device)
        fresh.glow.set_actnorm_init(True)
        fresh.eval()
        fresh.precision = sg.precision
        fresh.injected_masks = masks
        nll_fresh = _nll(fresh, batch)
        rel = float(((nll_in - nll_fresh).abs() / nll_fresh.abs().clamp(min=1.0)).max())
        report("forward inside ema_weights() vs a fresh module loaded from ema_state_dict(): per-frame NLL max rel diff %.3e "
               "(gate 1e-4), bit-equal: %s" % (rel, torch.equal(nll_in, nll_fresh)))
        assert rel <= 1e-4
        lm.train()
        with pytest.raises(RuntimeError, match="averaged weights are swapped in"):
            lm.fused_training_step(batch, 3e-3)
        with pytest.raises(RuntimeError, match="averaged weights are swapped in"):
            eng.ema_update(0.9)
        for step in (lambda: eng.optimizer_step(1e-3, 0.9, 0.999, 1e-8), lambda: eng.optimizer_step_sgd(1e-3),
                     lambda: eng.optimizer_step_rmsprop(1e-3), lambda: eng.backward(1.0)):
            with pytest.raises(RuntimeError, match="averaged weights are swapped in"):
                step()
        lm.eval()
        with pytest.raises(RuntimeError, match="already inside"):
            with sg.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside ema_weights"):      # refused before any tensor moves
            lm.to("cpu")
        assert all(v.is_cuda and torch.equal(v, esd[k]) for k, v in sg.state_dict().items())
        sg.injected_masks = None
        with pytest.raises(RuntimeError, match="parameters changed"):
            outer.step(frame, noise)
        inner = sg.open_stream(seed)
        inner.step(frame, noise)
    assert eng.param_version == version + 2 and not eng._ema_swapped
    for k, v in sg.state_dict().items():
        assert torch.equal(v, raw[k]), k
    with pytest.raises(RuntimeError, match="parameters changed"):
        inner.step(frame, noise)
    sg.injected_masks = masks
    nll_raw = _nll(sg, batch)
    assert not torch.equal(nll_raw, nll_in)
    # an exception inside still swaps back
    with pytest.raises(KeyError):
        with sg.ema_weights():
            raise KeyError("x")
    assert not eng._ema_swapped and all(torch.equal(v, raw[k]) for k, v in sg.state_dict().items())
    assert eng.ema_updates == 3
    inner.close()
    outer.close()


def test_rebind_keeps_the_average(gpu_device):
    lm, batch, _ = _module("tiny", gpu_device, ema_decay=0.9)
    for _ in range(2):
        lm.fused_training_step(batch, 3e-3)
    old = lm.seq_glow.engine
    ema, params = old.ema.clone(), old.params.clone()
    lm.to("cpu")
    lm.to(gpu_device)
    eng = lm.seq_glow._ensure_engine(gpu_device)
    assert eng is not old
    assert torch.equal(eng.ema, ema) and torch.equal(eng.params, params) and eng.ema_updates == 2
    lm.fused_training_step(batch, 3e-3)
    assert eng.ema_updates == 3 and worst_ratio(eng.ema, ema, eng.params, 0.9) <= 1.0


def test_checkpoint_round_trip(gpu_device, tmp_path):
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    from lets_face_it_amd.trainer import Trainer
    lm, batch, fx = _module("tiny", gpu_device, ema_decay=0.9)
    for _ in range(3):
        lm.fused_training_step(batch, 3e-3)
    path = str(tmp_path / "ema.ckpt")
    Trainer(lm.hparams, device=gpu_device, checkpoint_dir="").save_checkpoint(lm, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ckpt["ema_state_dict"]) == set(ckpt["state_dict"]) and all(not v.is_cuda for v in ckpt["ema_state_dict"].values())
    assert ckpt["optimizer_state"]["ema_updates"] == 3 and ckpt["optimizer_state"]["ema"].numel() == lm.seq_glow.engine.n_params
    assert "ema_swapped" not in ckpt["optimizer_state"] and "_ema_swapped" not in ckpt["optimizer_state"]

    lm2 = LetsFaceItGlow(Namespace(**copy.deepcopy(vars(lm.hparams))))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        Trainer(lm2.hparams, device=gpu_device, checkpoint_dir="").resume(lm2, path)
    assert not [w for w in caught if "averaged" in str(w.message)], "a checkpoint that holds the average resumes without that warning"
    lm2.train()
    lm2.seq_glow.injected_masks = lm.seq_glow.injected_masks
    e1, e2 = lm.seq_glow.engine, lm2.seq_glow.engine
    assert torch.equal(e1.ema, e2.ema) and e2.ema_updates == 3
    for _ in range(2):
        lm.fused_training_step(batch, 3e-3)
        lm2.fused_training_step(batch, 3e-3)
    assert e1.ema_updates == e2.ema_updates == 5
    assert torch.equal(e1.params, e2.params) and torch.equal(e1.ema, e2.ema)
    assert not torch.equal(e1.ema, e1.params)

    served = LetsFaceItGlow.load_from_checkpoint(path, weights="ema")
    assert served.state_dict().keys() == ckpt["ema_state_dict"].keys()
    for k, v in served.state_dict().items():
        assert torch.equal(v.cpu(), ckpt["ema_state_dict"][k]), k
    plain = LetsFaceItGlow.load_from_checkpoint(path)
    assert all(torch.equal(v.cpu(), ckpt["state_dict"][k]) for k, v in plain.state_dict().items())
    assert any(not torch.equal(served.state_dict()[k], plain.state_dict()[k]) for k in ckpt["state_dict"])
    with pytest.raises(ValueError, match="weights"):
        LetsFaceItGlow.load_from_checkpoint(path, weights="average")

    # a checkpoint written with averaging off
    off, batch_off, _ = _module("tiny", gpu_device)
    for _ in range(2):
        off.fused_training_step(batch_off, 3e-3)
    path_off = str(tmp_path / "plain.ckpt")
    Trainer(off.hparams, device=gpu_device, checkpoint_dir="").save_checkpoint(off, path_off)
    assert "ema_state_dict" not in torch.load(path_off, map_location="cpu", weights_only=False)
    with pytest.raises(KeyError, match="plain.ckpt"):
        LetsFaceItGlow.load_from_checkpoint(path_off, weights="ema")
    lm3 = LetsFaceItGlow(Namespace(**copy.deepcopy(vars(lm.hparams))))
    with pytest.warns(UserWarning, match="no averaged weights") as caught:
        Trainer(lm3.hparams, device=gpu_device, checkpoint_dir="").resume(lm3, path_off)
    assert len([w for w in caught if "no averaged weights" in str(w.message)]) == 1
    lm3.train()
    lm3.seq_glow.injected_masks = lm.seq_glow.injected_masks
    e3 = lm3.seq_glow.engine
    assert e3.ema is None and e3.ema_updates == 0
    lm3.fused_training_step(batch, 3e-3)
    assert torch.equal(e3.ema, e3.params) and e3.ema_updates == 1


class _OneBatch:
    def __init__(self, batch):
        self.batch = {k: v.cpu() for k, v in batch.items()}

    def val_dataloader(self):
        return [self.batch]


def test_validation_uses_the_average(gpu_device):
    from lets_face_it_amd.trainer import Trainer
    results = {}
    for use_ema in (True, False):
        lm, batch, _ = _module("tiny", gpu_device, ema_decay=0.5, validation=None if use_ema else {"use_ema": False})
        assert "use_ema" not in lm.hparams.Validation or not use_ema      # the default is on
        for _ in range(3):
            lm.fused_training_step(batch, 3e-3)
        sg = lm.seq_glow
        lm.eval()
        with torch.no_grad():
            raw = float(lm.validation_step(batch, 0).double())
            with sg.ema_weights():
                avg = float(lm.validation_step(batch, 0).double())
        before = sg.engine.params.clone()
        val = Trainer(lm.hparams, device=gpu_device, checkpoint_dir="").validate(lm, _OneBatch(batch))
        assert torch.equal(sg.engine.params, before) and lm.training
        results[use_ema] = (val, raw, avg)
    (val_on, raw, avg), (val_off, raw2, avg2) = results[True], results[False]
    report("Trainer.validate with ema_decay 0.5 after 3 steps: val_loss %.6f on the average (by hand %.6f), %.6f with use_ema off "
           "(raw weights by hand %.6f)" % (val_on, avg, val_off, raw2))
    assert (raw, avg) == (raw2, avg2)
    assert val_on == avg and val_off == raw
    # three steps of lr 3e-3 against an average that still holds half of the start: far beyond fp32 rounding of an NLL of this size
    assert abs(avg - raw) > 1e3 * 2.0 ** -24 * max(1.0, abs(raw)), (avg, raw)
    assert math.isfinite(avg) and math.isfinite(raw)
