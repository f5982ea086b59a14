"""Optimizer options on the device, host side (no GPU): the fp64 statement of the guarded step (probav_amd/optim_numpy.py) against the oracle's
plain optimizers, a hand-written clip_by_global_norm and torch's AveragedModel; the CLI flags; the checkpoint fields; and the three new torch
ops traced on fake tensors.  The device is held to optim_numpy in tests/test_gpu_optim_guard.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import nadam_numpy
from probav_amd import optim_numpy as on
from probav_amd.modelsTF import WDSRModel
from probav_amd.trainClass import HipAdam, HipNadam, HipSGD, ModelTrainer, make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec = importlib.util.spec_from_file_location("cli_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name, ref", [("nadam", nadam_numpy.Nadam), ("adam", nadam_numpy.Adam), ("sgd", nadam_numpy.SGD)])
def test_options_off_is_the_oracles_optimizer(name, ref):
    """Every option off: norm, scale = 1, no skip, no EMA -- the rule by coefficients equals the oracle's Nadam / Adam / SGD over 5 steps to 1e-15."""
    rng = np.random.default_rng(3)
    theta = rng.normal(0, 0.1, 4096)
    a, b = on.GuardedOptimizer(name, 5e-4), ref(lr=5e-4)
    ta, tb = theta.copy(), theta.copy()
    for _ in range(5):
        g = rng.normal(0, 1e-2, theta.shape)
        ta, tb = a.step(ta, g), b.step(tb, g)
        assert a.control["scale"] == 1.0 and not a.control["skip"] and a.ema is None
        assert np.abs(ta - tb).max() <= 1e-15
    assert a.skipped_total == 0 and a.t == 5


def test_clip_is_clip_by_global_norm():
    rng = np.random.default_rng(4)
    tensors = [rng.normal(0, s, n) for s, n in ((1.0, 100), (3.0, 37), (0.01, 512))]            # a list of gradient tensors, as tf takes them
    flat = np.concatenate(tensors)
    norm = np.sqrt(sum(float(np.sum(t * t)) for t in tensors))                                    # tf.linalg.global_norm
    for clip in (0.5 * norm, 2.0 * norm, norm):
        want = [t * clip / max(norm, clip) for t in tensors]                                      # tf.clip_by_global_norm
        c = on.guard_control(flat, global_clipnorm=clip)
        assert abs(c["norm"] - norm) <= 1e-12 * norm and not c["skip"]
        np.testing.assert_allclose(flat * c["scale"], np.concatenate(want), rtol=1e-14, atol=0)
    assert on.guard_control(flat)["scale"] == 1.0 and on.clip_scale(norm, 2.0 * norm) == 1.0
    # a non-finite element: the total is non-finite, the guard (if on) skips, clipping without the guard poisons as tf does
    for bad in (np.inf, -np.inf, np.nan):
        g = flat.copy()
        g[17] = bad
        assert on.guard_control(g, skip_nonfinite=True)["skip"] and not on.guard_control(g)["skip"]
        assert np.isnan(on.guard_control(g, global_clipnorm=1.0)["scale"])
    # the largest finite fp32 everywhere does not overflow the fp64 total: no false skip
    big = np.full(535267, np.finfo(np.float32).max, np.float32)
    assert not on.guard_control(big, skip_nonfinite=True)["skip"]


def test_guarded_step_skip_and_schedule():
    """A skipped step leaves theta, m, v, ema; the host's step count (and with it Nadam's schedule) advances all the same."""
    rng = np.random.default_rng(5)
    theta = rng.normal(0, 0.1, 256)
    o = on.GuardedOptimizer("nadam", 5e-4, global_clipnorm=0.05, skip_nonfinite=True, use_ema=True, ema_momentum=0.9)
    t1 = o.step(theta, rng.normal(0, 1e-2, 256))
    assert o.control["scale"] < 1.0
    np.testing.assert_array_equal(o.ema, 0.9 * theta + (1 - 0.9) * t1)                           # ema_0 = theta_0
    keep = (t1.copy(), o.m.copy(), o.v.copy(), o.ema.copy(), o.momentum_cache)
    bad = rng.normal(0, 1e-2, 256)
    bad[3] = np.inf
    t2 = o.step(t1, bad)
    assert o.skipped_total == 1 and o.t == 2 and o.momentum_cache != keep[4]
    for got, want in zip((t2, o.m, o.v, o.ema), keep):
        np.testing.assert_array_equal(got, want)


def test_ema_is_torchs_averaged_model():
    swa = pytest.importorskip("torch.optim.swa_utils")
    if not hasattr(swa, "get_ema_multi_avg_fn"):
        pytest.skip("this torch has no get_ema_multi_avg_fn")
    lin = torch.nn.Linear(7, 5).double()
    avg = swa.AveragedModel(lin, multi_avg_fn=swa.get_ema_multi_avg_fn(0.97))
    flat = lambda mod: np.concatenate([p.detach().numpy().reshape(-1) for p in mod.parameters()])
    avg.update_parameters(lin)                                                                    # its first call copies: ema_0 = theta_0
    ema = flat(lin).copy()
    rng = np.random.default_rng(6)
    for _ in range(5):
        with torch.no_grad():
            for p in lin.parameters():
                p.add_(torch.as_tensor(rng.normal(0, 0.1, tuple(p.shape))))
        avg.update_parameters(lin)
        ema = on.ema_update(ema, flat(lin), 0.97)
        np.testing.assert_allclose(ema, flat(avg.module), rtol=1e-14, atol=1e-16)


def test_cli_flags_parse():
    train, test, evaluate = _cli("train"), _cli("test"), _cli("evaluate")
    o = train.parser([])
    assert o.global_clipnorm is None and o.skip_nonfinite is False and o.ema_momentum is None and o.validate_on == "raw"
    o = train.parser(["--global-clipnorm", "2.5", "--skip-nonfinite", "--ema-momentum", "0.995", "--validate-on", "ema"])
    assert (o.global_clipnorm, o.skip_nonfinite, o.ema_momentum, o.validate_on) == (2.5, True, 0.995, "ema")
    for bad in (["--validate-on", "ema"], ["--global-clipnorm", "0"], ["--ema-momentum", "1.5"]):
        with pytest.raises(SystemExit):
            train.parser(bad)
    assert test.parser([]).weights == "raw" and test.parser(["--weights", "ema"]).weights == "ema"
    with pytest.raises(SystemExit):
        test.parser(["--weights", "best"])
    cfg = os.path.join(ROOT, "cfg", "p16t9c85r12.cfg")
    assert evaluate.parser(["--cfg", cfg, "--model"]).weights == "raw"
    assert evaluate.parser(["--cfg", cfg, "--model", "--weights", "ema"]).weights == "ema"
    with pytest.raises(SystemExit):
        evaluate.parser(["--cfg", cfg, "--toCompare", ROOT, "--weights", "ema"])


def test_weights_ema_is_refused_on_a_checkpoint_without_one(tmp_path):
    model = WDSRModel("t", "NIR", 0.0, 1.0, 6, 3, 32, 12, 8, 0.8, 9, 16, seed=0)
    tr = ModelTrainer(model, None, None, None, str(tmp_path / "ck"), str(tmp_path / "lg"))
    tr.save()
    ModelTrainer(model, None, None, None, str(tmp_path / "ck"), str(tmp_path / "lg"), weights="raw")
    with pytest.raises(ValueError, match="holds no EMA weights"):
        ModelTrainer(model, None, None, None, str(tmp_path / "ck"), str(tmp_path / "lg"), weights="ema")
    with pytest.raises(ValueError, match="use_ema"):
        ModelTrainer(model, None, None, make_optimizer("nadam", model, 1e-3), str(tmp_path / "c2"), str(tmp_path / "l2"), validate_on="ema")


def test_make_optimizer_keywords_and_defaults():
    model = WDSRModel("t", "NIR", 0.0, 1.0, 6, 3, 32, 12, 8, 0.8, 9, 16, seed=0)
    for name, cls in (("nadam", HipNadam), ("adam", HipAdam), ("sgd", HipSGD)):
        plain = make_optimizer(name, model, 1e-3)
        assert isinstance(plain, cls) and plain.guard is None and plain.guard_stats() is None and "guard" not in plain.state_dict()
        opt = make_optimizer(name, model, 1e-3, global_clipnorm=1.5, skip_nonfinite=True, use_ema=True, ema_momentum=0.9)
        assert isinstance(opt, cls) and opt.guard == {"global_clipnorm": 1.5, "skip_nonfinite": True, "use_ema": True, "ema_momentum": 0.9}
    with pytest.raises(ValueError):
        make_optimizer("nadam", model, 1e-3, global_clipnorm=-1.0)
    with pytest.raises(ValueError):
        make_optimizer("nadam", model, 1e-3, use_ema=True, ema_momentum=1.5)
    with pytest.raises(ValueError, match="ONE flat gradient"):
        HipNadam([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))], global_clipnorm=1.0)


def test_state_dict_round_trips_the_new_fields(tmp_path):
    p = torch.nn.Parameter(torch.arange(8, dtype=torch.float32))
    opt = HipNadam([p], lr=1e-3, global_clipnorm=2.0, skip_nonfinite=True, use_ema=True, ema_momentum=0.95)
    opt.state[p] = {"step": 7, "momentum_cache": 0.123, "m": torch.full_like(p, 0.5), "v": torch.full_like(p, 0.25), "ema": p.detach() * 0.9}
    opt._skipped_restored = 3
    sd = opt.state_dict()
    assert sd["guard"] == {"options": opt.guard, "skipped_total": 3}
    torch.save(sd, tmp_path / "o.pt")
    q = torch.nn.Parameter(torch.zeros(8))
    new = HipNadam([q], lr=1e-3, global_clipnorm=2.0, skip_nonfinite=True, use_ema=True, ema_momentum=0.95)
    new.load_state_dict(torch.load(tmp_path / "o.pt"))
    st = new.state[q]
    assert st["step"] == 7 and st["momentum_cache"] == 0.123 and new._skipped_restored == 3
    assert torch.equal(st["ema"], p.detach() * 0.9) and torch.equal(new.ema_buffer(), st["ema"]) and torch.equal(st["m"], torch.full_like(p, 0.5))
    assert new.state_dict()["guard"] == sd["guard"]
    # an optimizer without the options reads the same checkpoint as a plain one
    plain = HipNadam([torch.nn.Parameter(torch.zeros(8))], lr=1e-3)
    plain.load_state_dict(torch.load(tmp_path / "o.pt"))
    assert "ema" not in next(iter(plain.state.values())) and "guard" not in plain.state_dict()


class _Stop(Exception):
    pass


def test_guarded_ops_trace_on_fake_tensors(built_lib):
    """The three new ops are opaque, well-typed nodes with fake-tensor rules: the guarded optimizer step traces with fullgraph=True on CPU tensors
    (nothing executes: the kernels exist for gfx950 only), as the training step does in tests/test_ops_trace_cpu.py."""
    pytest.importorskip("torch._dynamo")
    import probav_amd.ops  # noqa: F401
    seen = {}

    def backend(gm, example_inputs):
        seen["g"] = gm.print_readable(print_output=False)

        def run(*args):
            raise _Stop()
        return run

    def step(theta, g, m, v, wc, ema, ctl, scratch, plain):
        torch.ops.probav.grad_guard(g, ctl, scratch, 1.5, True)
        torch.ops.probav.optimizer_wn_step_guarded(theta, g, m, v, wc, ema, ctl, 1234, 5e-4, 0.9, 0.999, 1e-7, 1.0, 0.5, 2.0, 0.99)
        torch.ops.probav.nadam_step_guarded(plain, g, m, v, None, ctl, 5e-4, 0.9, 0.999, 1e-7, 1.0, 0.5, 2.0, 0.99)
        return theta + 0

    n = 535267
    z = lambda: torch.zeros(n)
    args = (z(), z(), z(), z(), torch.zeros(4096), z(), torch.zeros(4, dtype=torch.int32), torch.zeros(128, dtype=torch.float64), z())
    torch._dynamo.reset()
    with pytest.raises(_Stop):
        torch.compile(step, backend=backend, fullgraph=True)(*args)
    torch._dynamo.reset()
    for name in ("probav.grad_guard", "probav.optimizer_wn_step_guarded", "probav.nadam_step_guarded"):
        assert name in seen["g"], seen["g"]
    for name, mutated in (("grad_guard", 2), ("nadam_step_guarded", 4), ("optimizer_wn_step_guarded", 5)):
        schema = str(getattr(torch.ops.probav, name).default._schema)
        assert schema.count("!") == mutated and schema.endswith("-> ()"), schema
