"""CPU: the non-finite step guard's reference (tests/guard_expected.py) against hand-computed cases and against planted defects, the
validation of its hparams, and the Trainer's reading of the record with a recording stand-in for the model (no kernels run)."""
import copy
from argparse import Namespace

import pytest
import torch

from guard_expected import DEFECTS, GuardedRun, mismatches, run
from helpers import Fixture
from lets_face_it_amd.mimicry_data_module import WindowLoader
from lets_face_it_amd.trainer import Trainer

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ the reference by hand
def test_sgd_with_momentum_by_hand():
    """step 1 skipped (NaN): nothing exists afterwards; step 2 is the FIRST step (buf = g); step 3 uses the buffer."""
    r = GuardedRun("sgd", {"momentum": 0.5, "dampening": 0.25}, 0.1, [1.0, 2.0], ema_decay=0.75)
    assert not r.step([NAN, 1.0])
    out = r.result()
    assert out["p"].tolist() == [1.0, 2.0] and out["state"]["adam_m"] is None and out["ema"] is None
    assert (out["skipped"], out["consecutive"], out["applied"]) == (1, 1, 0)
    assert r.step([1.0, -2.0])
    out = r.result()
    assert torch.allclose(out["p"], torch.tensor([0.9, 2.2])) and out["state"]["adam_m"].tolist() == [1.0, -2.0]
    assert torch.equal(out["ema"], out["p"])      # the first average is a copy
    assert r.step([2.0, 2.0])
    out = r.result()
    buf = torch.tensor([0.5 * 1.0 + 0.75 * 2.0, 0.5 * -2.0 + 0.75 * 2.0])
    assert torch.allclose(out["state"]["adam_m"], buf)
    assert torch.allclose(out["p"], torch.tensor([0.9, 2.2]) - 0.1 * buf)
    assert torch.allclose(out["ema"], torch.tensor([0.9, 2.2]) + 0.25 * (out["p"] - torch.tensor([0.9, 2.2])))
    assert (out["skipped"], out["consecutive"], out["applied"]) == (1, 0, 2)


def test_adam_by_hand():
    """A taken step, then a skipped one (+Inf): t stays 1, so the third gradient is corrected with t = 2."""
    r = GuardedRun("adam", {"betas": [0.5, 0.75], "eps": 0.0}, 0.1, [1.0], clip=0.0)
    assert r.step([2.0])      # m = 1, v = 1; m / (1 - 0.5) = 2, sqrt(v / 0.25) = 2: p -= 0.1
    assert abs(float(r.p.detach()) - 0.9) < 1e-7
    assert not r.step([INF])
    assert abs(float(r.p.detach()) - 0.9) < 1e-7 and r.state()["t"] == 1 and r.last_norm == INF and r.max_norm == 2.0
    assert r.step([2.0])      # m = 1.5, v = 1.75; t = 2: m / 0.75 = 2, sqrt(1.75 / 0.4375) = 2: p -= 0.1 again
    assert abs(float(r.p.detach()) - 0.8) < 1e-6 and r.state()["t"] == 2
    assert (r.skipped, r.consecutive, r.applied) == (1, 0, 2)


def test_clip_and_gmul_by_hand():
    """norm = sqrt(sumsq) * |gmul|, the clip coefficient clip / (norm + 1e-6) when < 1, both folded into one multiplier."""
    r = GuardedRun("sgd", {}, 1.0, [0.0, 0.0], clip=2.5, gmul=0.5)
    assert r.step([6.0, 8.0])      # norm 5: coefficient 0.5 * 0.5
    assert torch.allclose(r.p.detach(), torch.tensor([-1.5, -2.0]), atol=1e-6) and abs(r.last_norm - 5.0) < 1e-12
    r = GuardedRun("sgd", {}, 1.0, [0.0, 0.0], clip=20.0, gmul=0.5)
    assert r.step([6.0, 8.0])      # not clipped
    assert torch.allclose(r.p.detach(), torch.tensor([-3.0, -4.0]))


def test_huge_finite_gradients_are_taken():
    g = torch.full((1000,), 3e38)
    g[::2] = -3e38
    out = run("sgd", {}, 1e-40, torch.zeros(1000), [g], clip=1.0)
    assert out["applied"] == 1 and out["skipped"] == 0 and 9e39 < out["last_norm"] < 1e40
    assert torch.isfinite(out["p"]).all()


# ------------------------------------------------------------------ planted defects
def _sequence(n=64, steps=6, poisoned=(0, 2, 3), kind=NAN, seed=0):
    gen = torch.Generator().manual_seed(seed)
    grads = [torch.randn(n, generator=gen) for _ in range(steps)]
    for k in poisoned:
        grads[k][(7 * k + 3) % n] = kind
    return torch.randn(n, generator=gen), grads


CASE_OF = {
    "t_on_skip": ("adam", {"betas": [0.9, 0.99], "eps": 1e-8}, NAN),
    "momentum_on_skip": ("sgd", {"momentum": 0.8, "dampening": 0.1}, NAN),
    "ema_on_skip": ("adam", {"betas": [0.9, 0.99], "eps": 1e-8}, NAN),
    "inf_is_finite": ("rmsprop", {"eps": 1e-8}, INF),
    "big_is_nonfinite": ("sgd", {}, None),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_are_caught(defect):
    name, kwargs, kind = CASE_OF[defect]
    if kind is None:      # no poison at all: every gradient is +-3e38
        p0 = torch.zeros(64)
        grads = [torch.full((64,), 3e38) * (1 if k % 2 else -1) for k in range(3)]
        lr = 1e-40
    else:
        # "ema_on_skip" poisons steps 2 and 3 only: the average exists by then, and lerping it on a skip moves it
        p0, grads = _sequence(kind=kind, poisoned=(2, 3) if defect == "ema_on_skip" else (0, 2, 3))
        lr = 3e-2
    good = run(name, kwargs, lr, p0, grads, clip=5.0, ema_decay=0.5)
    again = run(name, kwargs, lr, p0, grads, clip=5.0, ema_decay=0.5)
    assert mismatches(again, good) == []
    bad = run(name, kwargs, lr, p0, grads, clip=5.0, ema_decay=0.5, defect=defect)
    assert mismatches(bad, good), "the comparison the GPU tests make does not see %s" % defect


def test_a_skipped_first_step_with_the_average_defect_is_caught_too():
    p0, grads = _sequence(poisoned=(0,))
    good = run("sgd", {}, 3e-2, p0, grads[:1], ema_decay=0.5)
    bad = run("sgd", {}, 3e-2, p0, grads[:1], ema_decay=0.5, defect="ema_on_skip")
    assert good["ema"] is None and "ema exists on one side only" in mismatches(bad, good)


# ------------------------------------------------------------------ hparams
def _hparams(optim=None, **top):
    hp = Namespace(**copy.deepcopy(Fixture("tiny").hp))
    hp.Optim.update(optim or {})
    for k, v in top.items():
        setattr(hp, k, v)
    return hp


def test_guard_is_off_unless_asked_for():
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    assert "skip_nonfinite" not in Fixture("tiny").hp["Optim"]
    assert LetsFaceItGlow(_hparams()).skip_nonfinite is False
    for off in (None, False):
        assert LetsFaceItGlow(_hparams({"skip_nonfinite": off})).skip_nonfinite is False
    assert LetsFaceItGlow(_hparams(terminate_on_nan=False, track_grad_norm=-1)).skip_nonfinite is False
    assert LetsFaceItGlow(_hparams({"skip_nonfinite": True})).skip_nonfinite is True
    assert LetsFaceItGlow(_hparams(terminate_on_nan=True)).skip_nonfinite is True      # implies it
    assert LetsFaceItGlow(_hparams(track_grad_norm=2)).skip_nonfinite is True          # the norm comes from the guard's record


@pytest.mark.parametrize("value", [1, 0, "yes", 1.0, [True]])
def test_bad_skip_nonfinite_raises_at_construction(value):
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    with pytest.raises(ValueError, match="skip_nonfinite"):
        LetsFaceItGlow(_hparams({"skip_nonfinite": value}))


@pytest.mark.parametrize("value", [0, -1, 2.5, "10", True])
def test_bad_max_consecutive_skips_raises_at_construction(value):
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow, max_consecutive_skips_of
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        LetsFaceItGlow(_hparams({"max_consecutive_skips": value}))
    assert max_consecutive_skips_of(_hparams()) == 10 and max_consecutive_skips_of(_hparams({"max_consecutive_skips": 3})) == 3


@pytest.mark.parametrize("value", [0, 1, "inf", 2.5])
def test_other_grad_norms_are_not_implemented(value):
    from lets_face_it_amd.glow.lets_face_it_glow import track_grad_norm_of
    with pytest.raises(NotImplementedError, match="track_grad_norm"):
        track_grad_norm_of(Namespace(track_grad_norm=value))
    with pytest.raises(NotImplementedError, match="track_grad_norm"):
        Trainer(_trainer_hparams(track_grad_norm=value), device="cpu", checkpoint_dir="").fit(_Recorder(()), _Data())


def test_the_graph_key_tells_guarded_steps_apart():
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    eng = Namespace(precision="f32", backward_products="auto", pass_skip={})
    batch = {"p1_face": torch.zeros(2, 3, 4)}
    keys = {LetsFaceItGlow(_hparams({"skip_nonfinite": on}))._graph_key(batch, False, eng) for on in (False, True)}
    assert len(keys) == 2


def test_mismatched_nll_keeps_its_value_when_the_new_one_is_not_finite():
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    for on in (True, False):
        lm = LetsFaceItGlow(_hparams({"skip_nonfinite": on}))
        lm._store_mismatched(torch.tensor(3.5))
        assert float(lm.last_missmatched_nll) == 3.5
        for bad in (NAN, INF, -INF):
            lm._store_mismatched(torch.tensor(bad))
            got = float(lm.last_missmatched_nll)
            assert got == 3.5 if on else (got != got or got == bad), (on, bad, got)
            if not on:
                lm._store_mismatched(torch.tensor(3.5))
        lm._store_mismatched(torch.tensor(-1.25))
        assert float(lm.last_missmatched_nll) == -1.25 and lm._last_mm() == -1.25


# ------------------------------------------------------------------ the Trainer's reading of the record
class _Windows:
    def __len__(self):
        return 40

    def batch(self, index):
        idx = torch.as_tensor(index, dtype=torch.int64)
        return {"p1_face": idx.float().reshape(-1, 1, 1).repeat(1, 30, 1)}


class _Data:
    def train_dataloader(self):
        return WindowLoader(_Windows(), 8, shuffle=False)      # 5 batches per epoch


class _Engine:
    """What the Trainer touches of GlowEngine: the record (read through guard_state) and the optimiser state around checkpoints."""

    def __init__(self):
        self.guard = object()
        self.ema = None
        self.counts = {"skipped": 0, "consecutive": 0, "applied": 0, "last_norm": 0.0, "max_norm": 0.0}
        self.reads = 0

    def take(self, poisoned):
        c = self.counts
        if poisoned:
            c.update(skipped=c["skipped"] + 1, consecutive=c["consecutive"] + 1, last_norm=NAN)
        else:
            c.update(applied=c["applied"] + 1, consecutive=0, last_norm=1.5, max_norm=1.5)

    def guard_state(self):
        self.reads += 1
        return dict(self.counts)

    def optimizer_state(self):
        return {"optimizer": None, "guard": {k: self.counts[k] for k in ("skipped", "consecutive", "applied", "max_norm")}}

    def load_optimizer_state(self, state):
        self.counts.update(state.get("guard") or {"skipped": 0, "consecutive": 0, "applied": 0, "max_norm": 0.0})


class _Recorder(torch.nn.Module):
    """Stands in for LetsFaceItGlow; step numbers (1-based) in `poisoned` are skipped by its engine, and change no weight."""

    def __init__(self, poisoned):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))
        self.poisoned, self.steps = set(poisoned), 0
        eng = self.eng = _Engine()
        glow = Namespace(actnorm_inited=lambda: True, set_actnorm_init=lambda flag: None)
        self.seq_glow = Namespace(spec=Namespace(start=24), engine=eng, glow=glow, allreduce_hook=None,
                                  _ensure_engine=lambda device: eng)
        self.hparams = Namespace(Optim={"name": "adam"})

    def fused_training_step(self, batch, lr, world, allreduce):
        self.steps += 1
        bad = self.steps in self.poisoned
        self.eng.take(bad)
        if not bad:
            with torch.no_grad():
                self.w += 1
        return torch.zeros(())


def _trainer_hparams(optim=None, **top):
    return Namespace(**{"lr": 1e-3, "Optim": {"Schedule": {"name": None}, **(optim or {})}, "max_epochs": 2, "max_steps": None,
                        "checkpoint_callback": True, **top})


@pytest.fixture
def no_device_wait(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)      # the log point's wait: nothing runs on a device here


def test_terminate_on_nan_stops_at_the_first_observed_skip_with_a_clean_checkpoint(tmp_path, no_device_wait):
    m = _Recorder(poisoned={3})
    tr = Trainer(_trainer_hparams(terminate_on_nan=True), device="cpu", log_every=2, checkpoint_dir=str(tmp_path))
    with pytest.raises(ValueError, match=r"between step 3 and step 4 .*terminate_on_nan") as err:
        tr.fit(m, _Data())
    assert "1 optimiser step(s)" in str(err.value)
    assert m.steps == 4, "the skip of step 3 is seen at the log point of step 4"
    ckpt = torch.load(str(tmp_path / "last.ckpt"), map_location="cpu", weights_only=False)      # written before the raise
    assert ckpt["global_step"] == 4 and float(ckpt["state_dict"]["w"][0]) == 3.0
    assert ckpt["optimizer_state"]["guard"] == {"skipped": 1, "consecutive": 0, "applied": 3, "max_norm": 1.5}


def test_without_terminate_a_lone_skip_is_survived_and_the_limit_stops_the_run(tmp_path, no_device_wait):
    m = _Recorder(poisoned={3})
    Trainer(_trainer_hparams({"skip_nonfinite": True}), device="cpu", log_every=2, checkpoint_dir="").fit(m, _Data())
    assert m.steps == 10 and float(m.w.detach()[0]) == 9.0

    m = _Recorder(poisoned=set(range(2, 40)))
    tr = Trainer(_trainer_hparams({"skip_nonfinite": True, "max_consecutive_skips": 3}), device="cpu", log_every=1,
                 checkpoint_dir=str(tmp_path))
    with pytest.raises(ValueError, match=r"3 steps in a row skipped \(Optim.max_consecutive_skips = 3\)"):
        tr.fit(m, _Data())
    assert m.steps == 4 and float(m.w.detach()[0]) == 1.0
    assert torch.load(str(tmp_path / "last.ckpt"), map_location="cpu", weights_only=False)["global_step"] == 4

    # the default limit is 10, and the read points before validation / the checkpoint see it without any log line
    m = _Recorder(poisoned=set(range(1, 40)))
    with pytest.raises(ValueError, match=r"Optim.max_consecutive_skips = 10"):
        Trainer(_trainer_hparams({"skip_nonfinite": True}), device="cpu", log_every=10 ** 9, checkpoint_dir="").fit(m, _Data())
    assert m.steps == 10, "two epochs of five steps: the second epoch's end is the first read that sees ten in a row"


def test_counters_travel_through_checkpoint_and_resume(tmp_path, no_device_wait):
    m = _Recorder(poisoned={2, 3})
    tr = Trainer(_trainer_hparams({"skip_nonfinite": True}, max_steps=4), device="cpu", log_every=10 ** 9, checkpoint_dir=str(tmp_path))
    tr.fit(m, _Data())
    m2 = _Recorder(poisoned=())
    tr2 = Trainer(_trainer_hparams(terminate_on_nan=True), device="cpu", log_every=1, checkpoint_dir="")
    tr2.resume(m2, str(tmp_path / "last.ckpt"))
    assert m2.eng.counts["skipped"] == 2 and m2.eng.counts["applied"] == 2 and tr2._guard_seen == 2
    tr2.fit(m2, _Data())      # the two skips of the earlier run are known: they do not terminate this one
    assert m2.steps == 6


def test_track_grad_norm_puts_the_norm_and_the_skips_on_the_log_line(capsys, no_device_wait):
    m = _Recorder(poisoned={1})
    Trainer(_trainer_hparams(track_grad_norm=2, max_steps=2), device="cpu", log_every=1, checkpoint_dir="").fit(m, _Data())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch 0 step")]
    assert len(lines) == 2
    assert "grad_norm nan skipped 1" in lines[0] and "grad_norm 1.5000e+00 skipped 1" in lines[1]
    m = _Recorder(poisoned=())
    Trainer(_trainer_hparams({"skip_nonfinite": True}, max_steps=1), device="cpu", log_every=1, checkpoint_dir="").fit(m, _Data())
    assert "grad_norm" not in capsys.readouterr().out
