"""The five update kernels of csrc/kernels_small.hip -- nadam_kernel, nadam_guard_kernel, wn_forward_kernel<true>, wn_forward_guard_kernel (and
the reparameterisation they end in) -- held PER ELEMENT and PER STEP to the fp64 one-step statement of tests/optim_cases.py, from the device's
own previous state, with the counted bounds stated there (16 u A + 1/2 ulp on theta, 3 u M on m, 4 u v' on v, 3 u on the EMA): every rule's
coefficient set, every gradient class, fresh and late steps, vector sizes around the workgroup, the words behind the vectors, the skip, the
host's schedule at a late step, and gradients whose square leaves fp32.  tests/test_optim_cases_host.py proves the bounds attainable on the
host.  Every test prints its worst ratios (units of u) before it asserts."""
import numpy as np
import pytest
import torch

from oracle import wdsr_numpy as on
from probav_amd import synth
from tests import optim_cases as oc
from tests.cfg_grid import arch_of

pytestmark = pytest.mark.gpu

PAD = 256
NAN_BITS = 0x7FC0BEEF                                  # a quiet NaN with a payload nothing computes
SIZES = (1, 255, 256, 257, 100003)
EMA_MOM = 0.99


def _L():
    from probav_amd import _lib
    return _lib


def _padded(dev, values):
    """values (fp32 numpy, n) as the first n floats of an allocation PAD floats longer, the rest NaN_BITS."""
    n = values.size
    t = torch.full((n + PAD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    t[:n] = torch.as_tensor(values).to(dev)
    return t


def _tail_intact(t, n):
    tail = t[n:].view(torch.int32)
    return tail.numel() == PAD and bool((tail == NAN_BITS).all())


def _host(*ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def _ctl_block(dev, g, clipnorm, skip_nonfinite, ctl=None):
    from probav_amd import ops
    L = _L()
    if ctl is None:
        ctl = torch.zeros(ops.GUARD_CTL_WORDS, dtype=torch.int32, device=dev)
    scratch = torch.empty(ops.guard_scratch_doubles(g.numel()), dtype=torch.float64, device=dev)
    L.check(L.lib().probav_grad_guard(L.ptr(g), g.numel(), clipnorm, 1 if skip_nonfinite else 0, L.ptr(scratch), scratch.numel() * 8, L.ptr(ctl),
                                      L.current_stream()), "probav_grad_guard")
    c = ctl.cpu()
    return ctl, {"scale": float(c.view(torch.float32)[0]), "skip": int(c[1]), "skipped_total": int(c[2])}


def _launch(kernel, bufs, g, n, coef, ctl):
    """One step through the C ABI on the first n floats of bufs = (theta, m, v, ema or None)."""
    L = _L()
    theta, m, v, ema = bufs
    b1, b2, eps, c_g, c_m, c_v = coef
    if kernel == "plain":
        L.check(L.lib().probav_nadam_step(L.ptr(theta), L.ptr(g), L.ptr(m), L.ptr(v), n, oc.LR, b1, b2, eps, c_g, c_m, c_v, L.current_stream()),
                "probav_nadam_step")
    else:
        L.check(L.lib().probav_nadam_step_guarded(L.ptr(theta), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), n, oc.LR, b1, b2, eps, c_g, c_m, c_v, EMA_MOM,
                                                  L.ptr(ctl), L.current_stream()), "probav_nadam_step_guarded")


WORST = {}


def _note(kernel, r):
    w = WORST.setdefault(kernel, {})
    for k, x in r.items():
        w[k] = max(w.get(k, 0.0), x)


def _report(kernel):
    print("worst ratios so far, %s (units of u; bounds %g / %g / %g / %g): %s"
          % (kernel, oc.K_THETA, oc.K_M, oc.K_V, oc.K_EMA, {k: round(x, 3) for k, x in WORST.get(kernel, {}).items()}))


# ---- 1. the element-wise kernels through the C ABI ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("rule", oc.RULES)
@pytest.mark.parametrize("kernel", ["plain", "guard", "guard-ema"])
def test_elementwise_kernels_follow_the_statement(dev, kernel, rule, cls):
    """Three steps from t in {1, 2, 1000, 250 001} at n in {1, 255, 256, 257, 100 003}.  The guarded kernel runs under a control block that
    probav_grad_guard wrote with a clip of 0.37 of the gradient's norm (scale < 1: asserted, except for the zero gradient, whose norm cannot be
    clipped; not a power of two, so that g * scale rounds), with and without an EMA."""
    for n in SIZES:
        for t0 in oc.STEPS:
            seed = 1000 * t0 % 7919 + n
            theta0 = oc.theta0(seed, n)
            m0, v0 = oc.slots0(seed, n, t0)
            bufs = [_padded(dev, theta0), _padded(dev, m0), _padded(dev, v0), _padded(dev, theta0) if kernel == "guard-ema" else None]
            for k in range(3):
                coef = oc.coefficients(rule, t0 + k)
                b1, b2, eps, c_g, c_m, c_v = coef
                theta, m, v = _host(*(b[:n] for b in bufs[:3]))
                ema = _host(bufs[3][:n])[0] if bufs[3] is not None else None
                g = oc.gradient(cls, seed + 7 * k, m, b1, c_g, c_m)
                gd = torch.as_tensor(g).to(dev)
                ctl, scale = None, 1.0
                if kernel != "plain":
                    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
                    ctl, c = _ctl_block(dev, gd, 0.37 * norm if norm > 0 else 1.0, True)
                    scale = c["scale"]
                    assert c["skip"] == 0 and (scale < 1.0 if cls != "zero" else scale == 1.0), c
                ref = oc.one_step(theta, g, m, v, oc.LR, b1, b2, eps, c_g, c_m, c_v, scale, ema, EMA_MOM)
                _launch(kernel, bufs, gd, n, coef, ctl)
                got = _host(*(b[:n] for b in bufs[:3]))
                got_ema = _host(bufs[3][:n])[0] if bufs[3] is not None else None
                r = oc.ratios(ref, got[0], got[1], got[2], got_ema, ema, EMA_MOM)
                _note("nadam_kernel" if kernel == "plain" else "nadam_guard_kernel", r)
                if not oc.within(r):
                    _report("nadam_kernel" if kernel == "plain" else "nadam_guard_kernel")
                assert oc.within(r), (kernel, rule, cls, n, t0 + k, r)
                if cls == "zero" and t0 == 1:                     # nothing moves and nothing is invented from a zero gradient on zero slots
                    assert _bits_equal(got[0], theta0) and not got[1].any() and not got[2].any()
            for b in bufs:
                assert b is None or _tail_intact(b, n), (kernel, rule, cls, n, t0)
    _report("nadam_kernel" if kernel == "plain" else "nadam_guard_kernel")


@pytest.mark.parametrize("rule", oc.RULES)
def test_skip_leaves_every_buffer_bit_for_bit(dev, rule):
    for n in SIZES:
        seed = 77 + n
        theta0 = oc.theta0(seed, n)
        m0, v0 = oc.slots0(seed, n, 2)
        ema0 = (theta0 * np.float32(0.9)).astype(np.float32)
        bufs = [_padded(dev, a) for a in (theta0, m0, v0, ema0)]
        coef = oc.coefficients(rule, 2)
        g = oc.gradient("normal", seed, m0, coef[0], coef[3], coef[4])
        bad = g.copy()
        bad[n // 2] = np.inf                                              # data in a buffer: the control block's reason to skip
        ctl, c0 = _ctl_block(dev, torch.as_tensor(g).to(dev), 0.0, True)
        assert c0["skip"] == 0 and c0["skipped_total"] == 0
        ctl, c1 = _ctl_block(dev, torch.as_tensor(bad).to(dev), 0.0, True, ctl)
        assert c1["skip"] == 1 and c1["skipped_total"] == 1
        _launch("guard", bufs, torch.as_tensor(g).to(dev), n, coef, ctl)   # a clean gradient under a block that says skip: the block decides
        for b, want in zip(bufs, (theta0, m0, v0, ema0)):
            assert _bits_equal(_host(b[:n])[0], want) and _tail_intact(b, n), (rule, n)
        ctl, c2 = _ctl_block(dev, torch.as_tensor(bad).to(dev), 0.0, True, ctl)
        assert c2["skip"] == 1 and c2["skipped_total"] == 2


# ---- 2. the fused kernels through make_optimizer on the shipped network ------------------------------------------------------------------------------
def _network(dev, row=None, seed=61):
    from probav_amd.modelsTF import WDSRConv3D
    if row is None:
        m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
        m.load_variables(synth.synth_params(seed=seed, perturb=True))
    else:
        F, R, E, decay, D = row
        m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, F, (3, 3, 3), R, E, decay, 9, 16, True, seed=0)
        assert int(m.numFilters * m.decayRate) == D
        m.load_variables(synth.synth_params(seed=seed, perturb=True, **arch_of(row)))
    return m.to(dev)


def _weff_columns_match(m, flat_host, label):
    """The weight cache's first block (the effective weights the next forward pass starts from) against the fp64 weight normalisation of the
    UPDATED parameters, column by column: <= 2e-6 of each column's own largest |w| (the project's forward bar, per column instead of per layer)."""
    nw = _L().lib().probav_weff_count(m._handle())
    assert m.weight_cache() is not None
    weff = m.weight_cache_buffer()[:nw].cpu().double().numpy()
    off, worst = 0, 0.0
    for Lh in m.layers:
        v = flat_host[Lh.v_off:Lh.b_off].astype(np.float64).reshape(-1, Lh.cout)
        w = on.weight_norm(v, flat_host[Lh.g_off:Lh.v_off])
        got = weff[off:off + w.size].reshape(w.shape)
        top = np.abs(w).max(axis=0)
        err = np.abs(got - w).max(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(top > 0, err / top, 0.0))))
        assert (err <= 2e-6 * top).all(), (label, Lh.name, int(np.argmax(err - 2e-6 * top)))
        off += w.size
    return worst


def _fused_steps(dev, m, rule, guarded, classes, steps=3):
    from probav_amd.trainClass import make_optimizer
    kernel = "wn_forward_guard_kernel" if guarded else "wn_forward_kernel<true>"
    n = m.flat.numel()
    start = m.flat.detach().clone()
    for cls in classes:
        with torch.no_grad():
            m.flat.copy_(start)
        opt = make_optimizer(rule, m, oc.LR, **(dict(global_clipnorm=1.0, skip_nonfinite=True, use_ema=True, ema_momentum=EMA_MOM) if guarded else {}))
        m_prev, v_prev = np.zeros(n, np.float32), np.zeros(n, np.float32)
        ema_prev = _host(m.flat)[0] if guarded else None
        for k in range(steps):
            b1, b2, eps, c_g, c_m, c_v = oc.coefficients(rule, 1 + k)
            theta = _host(m.flat)[0]
            g = oc.gradient(cls, 31 + 7 * k, m_prev, b1, c_g, c_m)
            m.flat.grad = torch.as_tensor(g).to(dev)
            scale = 1.0
            if guarded:                                            # this step's clip: 0.37 of the gradient's norm, so that it bites (the zero gradient has none)
                norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
                opt.guard["global_clipnorm"] = 0.37 * norm if norm > 0 else 1.0
            opt.step()
            if guarded:
                st = opt.guard_stats()
                scale = float(st["scale"])
                assert int(st["skipped_total"]) == 0 and (scale < 1.0 if cls != "zero" else scale == 1.0), (cls, scale)
            ref = oc.one_step(theta, g, m_prev, v_prev, oc.LR, b1, b2, eps, c_g, c_m, c_v, scale, ema_prev, EMA_MOM)
            st = opt.state[m.flat]
            got_theta, got_m, got_v = _host(m.flat, st["m"], st["v"])
            got_ema = _host(st["ema"])[0] if guarded else None
            r = oc.ratios(ref, got_theta, got_m, got_v, got_ema, ema_prev, EMA_MOM)
            _note(kernel, r)
            if not oc.within(r):
                _report(kernel)
            assert oc.within(r), (kernel, rule, cls, 1 + k, r)
            m_prev, v_prev, ema_prev = got_m, got_v, got_ema
        e = _weff_columns_match(m, got_theta, (kernel, rule, cls))
        print("%s %s %s: worst column error of weff %.3g of the column's max" % (kernel, rule, cls, e))
    _report(kernel)


@pytest.fixture(scope="module")
def shipped(dev):
    m = _network(dev)
    assert m.flat.numel() == 535267
    return m


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("rule", oc.RULES)
def test_fused_kernels_follow_the_statement(dev, shipped, rule, guarded):
    """Every parameter of the shipped network (gains and biases on lanes 0 and 1, the filter columns in the wave's loop), every gradient class
    planted as model.flat.grad, three steps each, then the effective weights the step left in the weight cache, per output column."""
    _fused_steps(dev, shipped, rule, guarded, oc.CLASSES)


def test_fused_kernels_on_columns_longer_than_the_register_path(dev):
    """cfg row (48, 2, 6, 0.9, 43) of tests/cfg_grid.py: normConv columns of 27 * 43 = 1161 elements take the loop beyond WN_Q * 64 = 896."""
    m = _network(dev, row=(48, 2, 6, 0.9, 43))
    assert max(int(np.prod(L.vshape[:-1])) for L in m.layers) == 27 * 48 and any(int(np.prod(L.vshape[:-1])) == 1161 for L in m.layers)
    _fused_steps(dev, m, "nadam", False, ("normal", "cancel"))
    _fused_steps(dev, m, "nadam", True, ("mixed",))


# ---- 3. the host's schedule at a late step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("done", [0, 998, 249998])
def test_host_schedule_at_a_late_step(dev, done):
    """HipNadam restored through load_state_dict after `done` steps (momentum cache: the oracle's running product; seeded slots), three steps of
    class normal: per element against the statement with the ORACLE's coefficients -- mu_t, mu_{t+1}, the running product and both bias
    corrections as HipNadam.step computes them on the host are what is under test."""
    from probav_amd.trainClass import HipNadam
    n = 4099
    theta0 = oc.theta0(done + 3, n)
    m0, v0 = oc.slots0(done + 3, n, done + 1)
    p = torch.nn.Parameter(torch.as_tensor(theta0).to(dev))
    src = HipNadam([p], lr=oc.LR)
    if done:
        src.state[p] = {"step": done, "momentum_cache": oc.momentum_cache(done), "m": torch.as_tensor(m0).to(dev), "v": torch.as_tensor(v0).to(dev)}
    opt = HipNadam([p], lr=1.0)                                       # every hyperparameter comes back from the state dict
    opt.load_state_dict(src.state_dict())
    m_prev, v_prev = m0, v0
    for k in range(3):
        t = done + 1 + k
        b1, b2, eps, c_g, c_m, c_v = oc.coefficients("nadam", t)
        theta = _host(p)[0]
        g = oc.gradient("normal", done + k, m_prev, b1, c_g, c_m)
        p.grad = torch.as_tensor(g).to(dev)
        opt.step()
        st = opt.state[p]
        assert st["step"] == t and abs(st["momentum_cache"] - oc.momentum_cache(t)) <= 1e-12 * oc.momentum_cache(t)
        ref = oc.one_step(theta, g, m_prev, v_prev, oc.LR, b1, b2, eps, c_g, c_m, c_v)
        got = _host(p, st["m"], st["v"])
        r = oc.ratios(ref, *got)
        print("after %d steps, step %d: ratios (units of u) %s" % (done, t, {k_: round(x, 3) for k_, x in r.items()}))
        assert oc.within(r), (done, t, r)
        m_prev, v_prev = got[1], got[2]


# ---- 4. gradients whose square leaves fp32 ------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.mark.parametrize("mag", [3e19, 1e21], ids=["3e19", "1e21"])
@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("rule", oc.RULES)
def test_gradient_squares_beyond_fp32(dev, rule, guarded, mag):
    """g = +-3e19 on a handful of elements among normal ones: finite, g * g is not.
    SGD: Keras gives theta - lr g; the kernel must give fl32(theta - lr g) there and stay finite afterwards (with beta_2 = 0 it formed v = g * g
    = inf and sqrt(inf * 0) = NaN: HipSGD passes beta_2 = 1 since).
    Adam, Nadam: Keras squares first (v = inf, the update is finite / inf = 0, for good).  The kernel forms ((1 - b2) g) g, which at 3e19 is
    9e35 and FINITE: v follows the statement (4 u) and nothing is lost for good.  theta follows the statement too wherever v' c_v is an fp32
    number (Adam: c_v = 1); where it is not (Nadam at t = 1, 2: c_v = 1000, 500) sqrt(inf) makes the update exactly 0, which is what Keras
    does with such an element.  At 1e21 (1 - b2) g^2 itself leaves fp32: v = inf, update 0 at every step -- Keras's behaviour exactly.
    Every other element follows the statement as if the big ones were not there, and theta is never non-finite."""
    from probav_amd.trainClass import HipAdam, HipNadam, HipSGD
    n = 1031
    big = np.array([0, 255, 256, 700, n - 1])
    sign = np.array([1, -1, 1, -1, 1], np.float32)
    theta0 = oc.theta0(5, n)
    p = torch.nn.Parameter(torch.as_tensor(theta0).to(dev))
    cls = {"nadam": HipNadam, "adam": HipAdam, "sgd": HipSGD}[rule]
    opt = cls([p], lr=oc.LR, **(dict(use_ema=True, ema_momentum=EMA_MOM) if guarded else {}))      # (EMA only: the guarded kernel, no clip)
    m_prev, v_prev = np.zeros(n, np.float32), np.zeros(n, np.float32)
    is_big = np.zeros(n, bool)
    is_big[big] = True
    pick = lambda s, keep: s._replace(**{f: getattr(s, f)[keep] for f in ("theta", "m", "v", "A", "M", "g")})
    for k in range(3):
        b1, b2, eps, c_g, c_m, c_v = oc.coefficients(rule, 1 + k)
        theta = _host(p)[0]
        g = oc.gradient("normal", 40 + k, m_prev, b1, c_g, c_m)
        if k == 0:
            g[big] = sign * np.float32(mag)
            with np.errstate(over="ignore"):
                assert np.isfinite(g).all() and np.isinf(g[big] * g[big]).all()
        p.grad = torch.as_tensor(g).to(dev)
        opt.step()
        st = opt.state[p]
        got = _host(p, st["m"], st["v"])
        assert np.isfinite(got[0]).all(), (rule, k, np.flatnonzero(~np.isfinite(got[0])))
        with np.errstate(invalid="ignore", over="ignore"):
            ref = oc.one_step(theta, g, m_prev, v_prev, oc.LR, b1, b2, eps, c_g, c_m, c_v)
            v_inf = ref.v > FLT_MAX                                        # the exact v' is no fp32 number: the device holds inf
            over = ref.v * c_v > FLT_MAX                                   # sqrt's argument is none: the update is 0
        assert not (over & ~is_big).any()
        keep = ~over
        r = oc.ratios(pick(ref, keep), got[0][keep], got[1][keep], got[2][keep])
        print("%s |g| = %g step %d: %d elements with v' c_v beyond fp32 (%d with v' itself); the rest: %s"
              % (rule, mag, 1 + k, int(over.sum()), int(v_inf.sum()), {k_: round(x, 3) for k_, x in r.items()}))
        assert oc.within(r), (rule, k, r)
        assert _bits_equal(got[0][over], theta[over]) and np.isinf(got[2][v_inf]).all(), (rule, k)
        mid = over & ~v_inf
        assert (np.abs(got[2][mid].astype(np.float64) - ref.v[mid]) <= oc.K_V * oc.U * ref.v[mid]).all()
        if rule == "sgd":
            assert not over.any() and not got[2].any()                     # beta_2 = 1: the slot stays 0
            if k == 0:
                want = (theta[big].astype(np.float64) - oc.f32(oc.LR) * g[big].astype(np.float64)).astype(np.float32)
                assert _bits_equal(got[0][big], want), (got[0][big], want)
        elif mag > 1e20:
            assert over[big].all() and v_inf[big].all() and _bits_equal(got[0][big], theta0[big])
        elif rule == "adam":
            assert not over.any()
        else:
            assert over[big].all() == (k < 2) and not v_inf.any()
        m_prev, v_prev = got[1], got[2]
