"""Optimizer options on the device ('Optimizer options on the device'): the gradient's global norm and control block
(probav_grad_guard), the guarded update launches, the EMA, and their way up through make_optimizer, ModelTrainer and the CLIs -- held to the
fp64 numpy statement in probav_amd/optim_numpy.py.  Bars: the norm is fp64 in a fixed order (error <= n 2^-53 ~ 6e-11) and is stored as fp32:
1e-6 relative; parameters and EMA: the existing optimizer bar, 2e-6 max|theta| (tests/test_gpu_ops.py, tests/test_gpu_parity.py); fused against
element-wise launch: 1e-6 max|theta|, as their plain siblings are held; everything that is 'the same computation' is compared bit for bit."""
import copy
import glob
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from probav_amd import optim_numpy as on
from probav_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _model(dev, seed=61):
    from probav_amd.modelsTF import WDSRConv3D
    m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
    m.load_variables(synth.synth_params(seed=seed, perturb=True))
    return m.to(dev)


def _losses():
    from probav_amd.loss import Losses
    return Losses(targetShape=(48, 48, 1))


def _batch(dev, n, seed):
    return tuple(torch.as_tensor(a).to(dev) for a in synth.synth_batch(n, seed=seed))


def _gradient(m, lo, batch):
    x, hr, mask = batch
    m.flat.grad = None
    lo.shiftCompensatedL1Loss(hr, mask, m(x, training=True)).backward()
    return m.flat.grad.detach().clone()


def _guard(g, clipnorm=0.0, skip=False, ctl=None):
    from probav_amd import ops
    if ctl is None:
        ctl = torch.zeros(ops.GUARD_CTL_WORDS, dtype=torch.int32, device=g.device)
    scratch = torch.empty(ops.guard_scratch_doubles(g.numel()), dtype=torch.float64, device=g.device)
    torch.ops.probav.grad_guard(g, ctl, scratch, clipnorm, skip)
    return ctl, scratch


def _ctl(ctl):
    c, f = ctl.cpu(), ctl.cpu().view(torch.float32)
    return {"scale": float(f[0]), "skip": int(c[1]), "skipped_total": int(c[2]), "norm": float(f[3])}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- 1. norm ---------------------------------------------------------------------------------------------------------------------------------
def test_norm_and_scale_against_fp64_numpy(dev):
    m, lo = _model(dev), _losses()
    grads = [_gradient(m, lo, _batch(dev, 2, 71))]
    assert grads[0].numel() == 535267
    gen = torch.Generator(device="cpu").manual_seed(11)
    for s in (1e-3, 1e-1, 1.0, 1e2):
        grads.append((torch.randn(535267, generator=gen) * s).to(dev))
    for g in grads:
        want = float(np.sqrt(np.sum(g.cpu().double().numpy() ** 2)))
        for clip in (0.0, 0.5 * want, 2.0 * want):
            ctl, scratch = _guard(g, clip)
            c = _ctl(ctl)
            print("norm %.9g want %.9g  scale %.9g  clip %.4g" % (c["norm"], want, c["scale"], clip))
            assert abs(c["norm"] - want) <= 1e-6 * want
            want_scale = 1.0 if clip <= 0 else clip / max(want, clip)
            assert abs(c["scale"] - want_scale) <= 1e-6 * want_scale
            assert c["skip"] == 0 and c["skipped_total"] == 0
            if clip <= 0 or clip > want:
                assert c["scale"] == 1.0                                     # exactly: an un-biting clip must not touch the gradient
            # the same gradient gives the same bits: a second call; a copy at another address after an unrelated allocation; a zero appended
            ctl2, scratch2 = _guard(g, clip)
            assert _same(ctl, ctl2) and torch.equal(scratch.view(torch.int64), scratch2.view(torch.int64))
            junk = torch.empty(1234567, device=dev)
            ctl3, _ = _guard(g.clone(), clip)
            ctl4, _ = _guard(torch.cat([g, torch.zeros(1, device=dev)]), clip)
            assert _same(ctl, ctl3) and _same(ctl, ctl4)
            del junk
    # the largest finite fp32 everywhere: no overflow of the fp64 total, no false skip
    big = torch.full((535267,), torch.finfo(torch.float32).max, device=dev)
    assert _ctl(_guard(big, 0.0, True)[0])["skip"] == 0


# ---- 2. disabled means identical -----------------------------------------------------------------------------------------------------------------
def test_guarded_launches_with_everything_off_leave_the_plain_bits(dev):
    a, b, c, lo = _model(dev), _model(dev), _model(dev), _losses()
    eng = lambda m: int(m._handle().value)
    st = {k: {"m": torch.zeros_like(m.flat.detach()), "v": torch.zeros_like(m.flat.detach())} for k, m in (("a", a), ("b", b), ("c", c))}
    for m in (a, b, c):
        m.weight_cache_buffer().zero_()                                      # (the cache has alignment gaps no kernel writes)
    cache = 1.0
    for t in range(1, 4):
        g = _gradient(a, lo, _batch(dev, 2, 80 + t))
        b1, b2, eps, c_g, c_m, c_v, cache = on.coefficients("nadam", t, cache)
        with torch.no_grad():
            torch.ops.probav.optimizer_wn_step(a.flat, g, st["a"]["m"], st["a"]["v"], a.weight_cache_buffer(), eng(a), 5e-4, b1, b2, eps, c_g, c_m, c_v)
            ctl, _ = _guard(g, 0.0, False)                                   # clipping off, guard off: scale = 1, skip = 0
            assert _ctl(ctl)["scale"] == 1.0 and _ctl(ctl)["skip"] == 0
            torch.ops.probav.optimizer_wn_step_guarded(b.flat, g, st["b"]["m"], st["b"]["v"], b.weight_cache_buffer(), None, ctl, eng(b),
                                                       5e-4, b1, b2, eps, c_g, c_m, c_v, 0.99)
            torch.ops.probav.optimizer_wn_step_guarded(c.flat, g, st["c"]["m"], st["c"]["v"], c.weight_cache_buffer(), None, None, eng(c),
                                                       5e-4, b1, b2, eps, c_g, c_m, c_v, 0.99)
        a.mark_weight_cache()
        for k, m in (("b", b), ("c", c)):
            assert _same(m.flat, a.flat) and _same(st[k]["m"], st["a"]["m"]) and _same(st[k]["v"], st["a"]["v"]), (k, t)
            assert _same(m.weight_cache_buffer(), a.weight_cache_buffer()), (k, t)
    # the element-wise pair
    gen = torch.Generator(device="cpu").manual_seed(12)
    n = 100003
    t0 = (torch.randn(n, generator=gen) * 0.1).to(dev)
    t1 = t0.clone()
    m0, v0, m1, v1 = (torch.zeros(n, device=dev) for _ in range(4))
    cache = 1.0
    for t in range(1, 4):
        g = (torch.randn(n, generator=gen) * 1e-2).to(dev)
        b1, b2, eps, c_g, c_m, c_v, cache = on.coefficients("nadam", t, cache)
        torch.ops.probav.nadam_step(t0, g, m0, v0, 5e-4, b1, b2, eps, c_g, c_m, c_v)
        ctl, _ = _guard(g, 0.0, False)
        torch.ops.probav.nadam_step_guarded(t1, g, m1, v1, None, ctl if t % 2 else None, 5e-4, b1, b2, eps, c_g, c_m, c_v, 0.99)
        assert _same(t0, t1) and _same(m0, m1) and _same(v0, v1), t


# ---- 3. clip -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nadam", "sgd"])
@pytest.mark.parametrize("factor", [0.5, 100.0])
def test_clip_against_the_numpy_statement(dev, name, factor):
    """5 steps with global_clipnorm = factor x the first step's norm: 0.5 bites at every step (asserted), 100 never does.  The first moment m is
    linear in the clipped gradient and is held too: per step one rounding of g * scale, the fp32 (1 - beta_1) (2.4e-7 off 0.1) and three fp32
    operations of 2^-24 each -- below 2e-6 of max|m| over 5 steps."""
    from probav_amd.trainClass import HipNadam, HipSGD, make_optimizer
    m, lo = _model(dev), _losses()
    batches = [_batch(dev, 2, 90)] * 5                                       # one batch: the norm stays near the first step's, so "bites" is a fact of every step
    g0 = _gradient(m, lo, batches[0])
    norm0 = float(np.sqrt(np.sum(g0.cpu().double().numpy() ** 2)))
    clip = factor * norm0
    lr = 5e-4 if name == "nadam" else 1e-3 / norm0                          # (SGD: an un-clipped step moves theta by 1e-3 in L2, whatever the loss's scale)
    opt = make_optimizer(name, m, lr, global_clipnorm=clip)
    plain = torch.nn.Parameter(m.flat.detach().clone())
    popt = (HipNadam if name == "nadam" else HipSGD)([plain], lr=lr, global_clipnorm=clip)        # the element-wise guarded launch
    ref = on.GuardedOptimizer(name, lr, global_clipnorm=clip)
    theta = m.flat.detach().cpu().double().numpy()
    for k in range(5):
        g = _gradient(m, lo, batches[k])
        opt.step()
        plain.grad = g
        popt.step()
        theta = ref.step(theta, g.cpu().double().numpy())
        stats = {key: float(v) for key, v in opt.guard_stats().items()}
        assert abs(stats["norm"] - ref.control["norm"]) <= 1e-6 * ref.control["norm"]
        assert (stats["scale"] < 1.0) == (factor < 1.0) and abs(stats["scale"] - ref.control["scale"]) <= 1e-6 * ref.control["scale"]
        got = m.flat.detach().cpu().double().numpy()
        top = np.abs(theta).max()
        e_ref, e_pair = np.abs(got - theta).max(), float((m.flat.detach() - plain.detach()).abs().max())
        mm = opt.state[m.flat]["m"].cpu().double().numpy()
        e_m = np.abs(mm - ref.m).max() / np.abs(ref.m).max()
        print("%s x%g step %d: scale %.6g  err vs numpy %.3e  fused vs element-wise %.3e  (max|theta| %.3g)  m rel err %.3e"
              % (name, factor, k, stats["scale"], e_ref, e_pair, top, e_m))
        assert e_ref < 2e-6 * top and e_pair < 1e-6 * top
        assert e_m < 2e-6
    assert m.weight_cache() is not None


# ---- 4. skip -----------------------------------------------------------------------------------------------------------------------------------
def _advance_schedule(opt, steps):
    """What the host does to a HipNadam's schedule in `steps` steps, without a launch (beta_1 at its fp32 value, as HipNadam.step takes it)."""
    from probav_amd.trainClass import _as_fp32
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state[p]
            for _ in range(steps):
                st["step"] += 1
                st["momentum_cache"] *= _as_fp32(group["beta_1"]) * (1.0 - 0.5 * 0.96 ** (st["step"] * group["schedule_decay"]))


def test_nonfinite_gradient_costs_one_step_not_the_run(dev):
    from probav_amd.trainClass import make_optimizer
    m, lo = _model(dev), _losses()
    m.weight_cache_buffer().zero_()
    opts = dict(global_clipnorm=1e3, skip_nonfinite=True, use_ema=True, ema_momentum=0.9)
    opt = make_optimizer("nadam", m, 5e-4, **opts)
    for k in range(2):
        _gradient(m, lo, _batch(dev, 2, 100 + k))
        opt.step()
    st = opt.state[m.flat]
    # the twin: the same run without the two bad gradients, its host schedule moved on by the two steps the device dropped
    twin = _model(dev)
    with torch.no_grad():
        twin.flat.copy_(m.flat)
    topt = make_optimizer("nadam", twin, 5e-4, **opts)
    topt.state[twin.flat] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
    keep = {k: st[k].clone() for k in ("m", "v", "ema")}
    keep["flat"], keep["wc"] = m.flat.detach().clone(), m.weight_cache_buffer().clone()
    g = _gradient(m, lo, _batch(dev, 2, 102))
    assert int(opt.guard_stats()["skipped_total"]) == 0
    for n_bad, bad in enumerate((float("inf"), float("nan")), 1):
        gb = g.clone()
        gb[123457] = bad                                                     # data in a buffer, not a fault
        m.flat.grad = gb
        opt.step()
        c = _ctl(opt._ctl)
        assert c["skip"] == 1 and c["skipped_total"] == n_bad and not np.isfinite(c["norm"])
        assert _same(m.flat, keep["flat"]) and all(_same(st[k], keep[k]) for k in ("m", "v", "ema"))
        assert m.weight_cache() is not None and _same(m.weight_cache_buffer(), keep["wc"])
    assert st["step"] == 4                                                  # the host's count went on over the two dropped steps: documented
    # the next clean step is the twin's step at the same host step count
    _advance_schedule(topt, 2)
    m.flat.grad, twin.flat.grad = g.clone(), g.clone()
    opt.step()
    topt.step()
    assert _ctl(opt._ctl)["skip"] == 0 and _ctl(opt._ctl)["skipped_total"] == 2
    assert _same(m.flat, twin.flat) and all(_same(st[k], topt.state[twin.flat][k]) for k in ("m", "v", "ema"))
    assert not _same(m.flat, keep["flat"]) and bool(torch.isfinite(m.flat).all())
    # without the guard the same gradient poisons the parameters: the guard is what saved them
    for kw in (dict(global_clipnorm=1e3), dict(use_ema=True)):
        v = _model(dev)
        vopt = make_optimizer("nadam", v, 5e-4, **kw)
        gb = g.clone()
        gb[123457] = float("inf")
        v.flat.grad = gb
        vopt.step()
        assert not bool(torch.isfinite(v.flat).all()), kw


# ---- 5. EMA ------------------------------------------------------------------------------------------------------------------------------------
def test_ema_against_numpy_and_the_weights_from_scope(dev):
    """EMA after step 0 = mom theta_0 + (1 - mom) theta_1: two fp32 products and a sum on the device (2^-24 each, a fused multiply-add saves one)
    and the fp32 (1 - mom), 1e-6 off 0.01 on a term of 1 % -- below 2.5e-7 max|theta| against the fp64 evaluation of the same fp32 inputs."""
    from probav_amd.trainClass import make_optimizer
    m, lo = _model(dev), _losses()
    mom = 0.99
    opt = make_optimizer("nadam", m, 5e-4, use_ema=True, ema_momentum=mom)
    assert opt.guard_stats() is None                                         # EMA only: no control block, one launch as the plain step
    ref = on.GuardedOptimizer("nadam", 5e-4, use_ema=True, ema_momentum=mom)
    theta0 = m.flat.detach().cpu().double().numpy()
    theta = theta0
    for k in range(5):
        g = _gradient(m, lo, _batch(dev, 2, 110 + k))
        opt.step()
        theta = ref.step(theta, g.cpu().double().numpy())
        ema = opt.ema_buffer().cpu().double().numpy()
        top = np.abs(theta).max()
        print("step %d: EMA err %.3e  theta err %.3e  (max|theta| %.3g)" % (k, np.abs(ema - ref.ema).max(), np.abs(m.flat.detach().cpu().double().numpy() - theta).max(), top))
        assert np.abs(ema - ref.ema).max() < 2e-6 * top
        assert np.abs(m.flat.detach().cpu().double().numpy() - theta).max() < 2e-6 * top
        if k == 0:
            theta1 = m.flat.detach().cpu().double().numpy()
            assert np.abs(ema - (mom * theta0 + (1 - mom) * theta1)).max() < 2.5e-7 * top
    # forward from the EMA weights through the scope == a model loaded with the EMA buffer, bit for bit; the raw side is untouched
    x = _batch(dev, 3, 120)[0]
    ema = opt.ema_buffer()
    assert m.weight_cache() is not None
    raw_flat, raw_wc = m.flat.detach().clone(), m.weight_cache_buffer().clone()
    with torch.no_grad():
        y_raw = m(x)
        with m.weights_from(ema):
            y_scope = m(x)
            with pytest.raises(RuntimeError, match="forward passes only"):
                with torch.enable_grad():
                    m(x, training=True)
        y_raw2 = m(x)
    other = _model(dev, seed=7)
    with torch.no_grad():
        other.flat.copy_(ema)
        y_loaded = other(x)
    assert _same(y_scope, y_loaded) and not _same(y_scope, y_raw) and _same(y_raw, y_raw2)
    assert _same(m.flat, raw_flat) and m.weight_cache() is not None and _same(m.weight_cache_buffer(), raw_wc)
    with pytest.raises(ValueError):
        with m.weights_from(ema[:-1]):
            pass


# ---- 6. trainer ---------------------------------------------------------------------------------------------------------------------------------
class _InfOnce:
    """The trainer's loss, multiplied by inf at ONE training call: the gradient of that batch is inf / NaN throughout."""

    def __init__(self, loss, at):
        self.loss, self.at, self.calls = loss, at, 0

    def __call__(self, hr, mask, pred):
        out = self.loss(hr, mask, pred)
        if pred.requires_grad:
            self.calls += 1
            if self.calls == self.at:
                out = out * float("inf")
        return out


def _trainer(dev, d, loss=None, validate_on="raw"):
    from probav_amd.trainClass import ModelTrainer, make_optimizer
    m, lo = _model(dev, seed=41), _losses()
    opt = make_optimizer("nadam", m, 5e-4, global_clipnorm=50.0, skip_nonfinite=True, use_ema=True, ema_momentum=0.9)
    tr = ModelTrainer(m, loss or lo.shiftCompensatedL1Loss, lo.shiftCompensatedcPSNR, opt, os.path.join(d, "ck"), os.path.join(d, "lg"), evalStep=6,
                      validate_on=validate_on)
    tr.tune_side_stream = False
    return tr, m, opt, lo


def _state_digest(m, opt):
    h = hashlib.sha256()
    st = opt.state[m.flat]
    for t in (m.flat, st["m"], st["v"], st["ema"], opt._ctl):
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_trainer_with_all_three_options(dev, tmp_path):
    d = str(tmp_path)
    x, hr, mask = synth.synth_batch(24, seed=130)
    tr, m, opt, lo = _trainer(dev, d, loss=_InfOnce(_losses().shiftCompensatedL1Loss, at=4), validate_on="ema")
    tr.fitTrainData(x, [hr, mask], 2, 1, [x[:4], hr[:4], mask[:4]], valSteps=2, saveBestOnly=False)
    assert tr.step == 12 and bool(torch.isfinite(m.flat).all()) and bool(torch.isfinite(opt.ema_buffer()).all())
    events = [json.loads(l) for l in open(os.path.join(d, "lg", "events.jsonl"))]
    skipped = [e["value"] for e in events if e["tag"] == "Skipped steps"]
    norms = [e["value"] for e in events if e["tag"] == "Grad norm"]
    assert skipped == [0.0] * 3 + [1.0] * 9, skipped
    assert len(norms) == 12 and not np.isfinite(norms[3]) and all(np.isfinite(v) and v > 0 for i, v in enumerate(norms) if i != 3)
    assert open(os.path.join(d, "ck", "checkpoint.pt-index")).read().split() == ["ckpt-1.pt", "ckpt-2.pt"]
    state = torch.load(os.path.join(d, "ck", "ckpt-2.pt"), map_location="cpu")
    assert set(state["ema"]) == set(state["model"]) and state["optimizer"]["guard"]["skipped_total"] == 1
    flat_ema = torch.cat([torch.cat([state["ema"][L.name][k].reshape(-1) for k in ("g", "v", "bias")]) for L in m.layers])
    assert torch.equal(flat_ema, opt.ema_buffer().cpu()) and not torch.equal(flat_ema, m.flat.detach().cpu())
    # validate_on="ema": the reported metric is the EMA weights' (a direct evaluation), not the raw weights'
    vb = _batch(dev, 4, 131)
    tr.testPSNR.reset_states()
    tr.testStep(*vb)
    with torch.no_grad():
        with m.weights_from(opt.ema_buffer()):
            direct = float(lo.shiftCompensatedcPSNR(vb[1], vb[2], m(vb[0])).double().mean())
        raw = float(lo.shiftCompensatedcPSNR(vb[1], vb[2], m(vb[0])).double().mean())
    assert tr.testPSNR.result() == direct and direct != raw
    # a second trainer restored from the checkpoint continues bit for bit against the uninterrupted one
    tr2, m2, opt2, _ = _trainer(dev, d)
    assert tr2.step == 12 and _same(m2.flat, m.flat) and opt2._skipped_restored == 1
    for k in range(3):
        b = _batch(dev, 2, 140 + k)
        tr.trainStep(*b)
        tr2.trainStep(*b)
        assert _state_digest(m, opt) == _state_digest(m2, opt2), k
    assert _ctl(opt2._ctl)["skipped_total"] == 1
    # test.py's restore path: the EMA entry into a model
    from probav_amd.trainClass import ModelTrainer
    m3 = _model(dev, seed=5)
    ModelTrainer(m3, None, None, None, os.path.join(d, "ck"), os.path.join(d, "lg3"), weights="ema")
    assert torch.equal(m3.flat.detach().cpu(), flat_ema)


# ---- 7. data parallel at world size 1 -----------------------------------------------------------------------------------------------------------
DP = r"""
import hashlib, os, sys
sys.path.insert(0, %r)
import torch
import torch.distributed as dist
from probav_amd import synth
from probav_amd.loss import Losses
from probav_amd.modelsTF import WDSRConv3D
from probav_amd.trainClass import ModelTrainer, dp_state, make_optimizer
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
forced = os.environ.get("PROBAV_FORCE_DP") == "1"
if forced:
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
assert dp_state() == (forced, 1)
model = WDSRConv3D("dp", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True)
model.load_variables(synth.synth_params(seed=41, perturb=True))
model = model.to(dev)
lo = Losses(targetShape=(48, 48, 1))
opt = make_optimizer("nadam", model, 5e-4, global_clipnorm=0.5, skip_nonfinite=True, use_ema=True, ema_momentum=0.9)
tr = ModelTrainer(model, lo.shiftCompensatedL1Loss, lo.shiftCompensatedcPSNR, opt, sys.argv[1] + "/ck", sys.argv[1] + "/lg", multiGPU=True)
assert tr._dp() == forced
calls = []
if forced:
    real = dist.all_reduce
    def counting(t, *a, **k):
        calls.append(int(t.numel()))
        return real(t, *a, **k)
    dist.all_reduce = counting
h = hashlib.sha256()
for k in range(3):
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(6, seed=50 + k))
    tr.trainStep(x, hr, mask)
    torch.cuda.synchronize()
    st = opt.state[model.flat]
    for t in (model.flat, st["m"], st["v"], st["ema"], opt._ctl):
        h.update(t.detach().cpu().numpy().tobytes())
if forced:
    assert calls == [model.flat.numel() + 2] * 3, calls       # still ONE collective per step: the norm is taken on the reduced gradient
    dist.barrier()
    dist.destroy_process_group()
print("SCALE %%.9g" %% float(opt.guard_stats()["scale"]))
print("DIGEST", h.hexdigest())
""" % ROOT


def test_guarded_step_under_rccl_is_the_plain_guarded_step(dev, tmp_path):
    from tests.test_gpu_dp import _env, _free_port

    def run(tmp, **extra):
        os.makedirs(tmp, exist_ok=True)
        out = subprocess.run([sys.executable, "-c", DP, tmp], env=_env(MASTER_PORT=str(_free_port()), **extra), capture_output=True, text=True,
                             timeout=900, cwd=ROOT)
        assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
        lines = out.stdout.splitlines()
        return [l for l in lines if l.startswith("DIGEST")][0], float([l for l in lines if l.startswith("SCALE")][0].split()[1])
    plain, s0 = run(str(tmp_path / "plain"))
    forced, s1 = run(str(tmp_path / "dp"), PROBAV_FORCE_DP="1")
    assert plain == forced and s0 == s1 and 0.0 < s0 < 1.0                   # (the clip bit: the decision is part of what must agree)


# ---- 8. ops ------------------------------------------------------------------------------------------------------------------------------------
def test_opcheck_and_compile_of_the_guarded_ops(dev):
    m, lo = _model(dev), _losses()
    g = _gradient(m, lo, _batch(dev, 2, 150))
    from probav_amd import ops
    n = g.numel()
    ctl = torch.zeros(ops.GUARD_CTL_WORDS, dtype=torch.int32, device=dev)
    scratch = torch.zeros(ops.guard_scratch_doubles(n), dtype=torch.float64, device=dev)
    torch.library.opcheck(torch.ops.probav.grad_guard.default, (g, ctl, scratch, 0.5, True))
    torch.ops.probav.grad_guard(g, ctl, scratch, 0.5, True)
    z = lambda: torch.zeros(n, device=dev)
    theta, ema = m.flat.detach().clone(), m.flat.detach().clone()
    co = (5e-4, 0.9, 0.999, 1e-7, 1.0, 0.5, 2.0, 0.99)
    torch.library.opcheck(torch.ops.probav.nadam_step_guarded.default, (theta, g, z(), z(), ema, ctl) + co)
    torch.library.opcheck(torch.ops.probav.nadam_step_guarded.default, (theta, g, z(), z(), None, None) + co)
    wc = torch.zeros_like(m.weight_cache_buffer())
    eng = int(m._handle().value)
    torch.library.opcheck(torch.ops.probav.optimizer_wn_step_guarded.default, (theta, g, z(), z(), wc, ema, ctl, eng) + co)

    def step(theta, g, mm, vv, wc, ema, ctl, scratch):
        torch.ops.probav.grad_guard(g, ctl, scratch, 0.5, True)
        torch.ops.probav.optimizer_wn_step_guarded(theta, g, mm, vv, wc, ema, ctl, eng, *co)
        return theta * 1.0

    def fresh():
        return (m.flat.detach().clone(), g, z(), z(), torch.zeros_like(wc), m.flat.detach().clone(), torch.zeros_like(ctl), torch.zeros_like(scratch))
    a = fresh()
    want = step(*a)
    try:
        import importlib
        importlib.import_module("torch._dynamo")
        cstep = torch.compile(step, backend="aot_eager", fullgraph=True)
    except (ImportError, ModuleNotFoundError) as exc:
        pytest.skip("torch.compile (dynamo) is not part of this torch build: %r" % (exc,))
    b = fresh()
    got = cstep(*b)
    assert _same(got, want) and not _same(want, m.flat)
    for u, v in zip(a, b):                                                  # every mutated argument, bit for bit
        assert _same(u, v) if u.dtype == torch.float32 else torch.equal(u, v)


# ---- 9. CLI ------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_with_the_flags_then_test_py_weights_ema(dev, tmp_path):
    from tests.test_gpu_cli import CFG, _run
    from probav_amd.pngio import imread_uint16
    d = str(tmp_path)
    aug, res = os.path.join(d, "pre", "augmentedPatchesDir"), os.path.join(d, "pre", "resolverDir")
    os.makedirs(aug), os.makedirs(res)
    n, nval = 1000, 6                                                       # the trainer evaluates (and saves) every 1000 steps of an epoch
    x, hr, mask = synth.synth_batch(16, seed=5)
    rep = lambda a, k: np.concatenate([a] * (k // len(a) + 1))[:k]
    for tag, k in (("TRAIN", n), ("TRAINVAL", nval)):
        np.ma.masked_array(rep(x, k), mask=np.zeros(rep(x, k).shape, bool)).dump(os.path.join(aug, "%spatchesLR_NIR.npy" % tag))
        np.ma.masked_array(rep(hr, k), mask=~rep(mask, k).astype(bool)).dump(os.path.join(aug, "%spatchesHR_NIR.npy" % tag))
    sets = 2
    test_patches = synth.synth_batch(sets * 64, seed=6)[0].reshape(sets, 64, 22, 22, 9, 1)
    np.ma.masked_array(test_patches.transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((sets, 64, 9, 1, 22, 22), bool)).dump(
        os.path.join(res, "TESTpatchesLR_NIR.npy"))
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d))
    out = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR", "--global-clipnorm", "1000", "--skip-nonfinite", "--ema-momentum", "0.99",
                "--validate-on", "ema"], cwd=d)
    assert "Grad norm:" in out.stderr and "Skipped steps: 0" in out.stderr and "[ SAVE ] Saving checkpoint..." in out.stderr
    ck = os.path.join(d, "modelInfo", "ckpt_mini", "NIR")
    assert "ema" in torch.load(os.path.join(ck, "ckpt-1.pt"), map_location="cpu")
    images = {}
    for w in ("raw", "ema"):
        for p in glob.glob(os.path.join(d, "testout_mini", "*.png")):
            os.remove(p)
        _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR", "--weights", w], cwd=d)
        pngs = sorted(glob.glob(os.path.join(d, "testout_mini", "*.png")))
        assert [os.path.basename(p) for p in pngs] == ["imgset1306.png", "imgset1307.png"]
        images[w] = [imread_uint16(p) for p in pngs]
    assert all(not np.array_equal(a, b) for a, b in zip(images["raw"], images["ema"]))
