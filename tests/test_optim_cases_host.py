"""tests/optim_cases.py on the host (no GPU): (a) an fp32 numpy evaluation of the update rule, every operation rounded on its own, stays
within the bounds the kernels are held to in tests/test_gpu_optim_rule.py -- on every gradient class, rule and step, from its own previous
state; (b) the fp64 statement, iterated, IS the pinned oracle (oracle/nadam_numpy.py constructed with the fp32 values of the hyperparameters);
(c) the statement with beta_2 = 0.999 in double would not fit: why the hyperparameters enter at their fp32 values."""
import numpy as np
import pytest

from oracle import nadam_numpy
from tests import optim_cases as oc

N = 4099


def _run(rule, cls, t0, seed, scale=1.0, mom=None, b2_override=None):
    theta, (m, v) = oc.theta0(seed, N), oc.slots0(seed, N, t0)
    ema = theta.copy() if mom is not None else None
    worst = {}
    for k in range(4):
        b1, b2, eps, c_g, c_m, c_v = oc.coefficients(rule, t0 + k)
        g = oc.gradient(cls, seed + 7 * k, m, b1, c_g, c_m)
        ref = oc.one_step(theta, g, m, v, oc.LR, b1, b2, eps, c_g, c_m, c_v, scale, ema, mom)
        if b2_override is not None:                         # the statement as it would be with a double beta_2 (one_step takes fp32 values: redo v)
            ref = _with_double_b2(ref, theta, m, v, b2_override, eps, c_g, c_m, c_v)
        prev = ema
        theta, m, v, ema = oc.emulate_step(theta, g, m, v, oc.LR, b1, b2, eps, c_g, c_m, c_v, scale, ema, mom)
        assert np.isfinite(theta).all() and np.isfinite(v).all()
        r = oc.ratios(ref, theta, m, v, ema, prev, mom)
        for key, val in r.items():
            worst[key] = max(worst.get(key, 0.0), val)
    return worst


def _with_double_b2(ref, theta, m, v, b2, eps, c_g, c_m, c_v):
    v1 = b2 * np.asarray(v, np.float64) + (1.0 - b2) * ref.g * ref.g
    den = np.sqrt(v1 * c_v) + oc.f32(eps)
    lr = oc.f32(oc.LR)
    return ref._replace(v=v1, theta=np.asarray(theta, np.float64) - lr * (c_g * ref.g + c_m * ref.m) / den,
                        A=ref.A * (np.sqrt(ref.v * c_v) + oc.f32(eps)) / den)


WORST = {}


@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("rule", oc.RULES)
def test_fp32_emulation_stays_within_the_bounds(rule, cls):
    for t0 in oc.STEPS:
        for scale, mom in ((1.0, None), (0.37, 0.99), (1.0, 0.3)):
            r = _run(rule, cls, t0, seed=100 + t0 % 97, scale=scale, mom=mom)
            for key, val in r.items():
                WORST[key] = max(WORST.get(key, 0.0), val)
            assert oc.within(r), (rule, cls, t0, scale, mom, r)
    print("worst so far (units of u):", {k: round(x, 2) for k, x in WORST.items()})


def test_a_double_beta_2_would_not_fit():
    """(1 - fl32(0.999)) / 0.001 - 1 = 1.3e-5 = 216 u: against a statement with the double 0.999 the same emulation is two hundred units off in v.
    The bound on v (4 u) is therefore sharp enough to see which beta_2 a kernel applies."""
    r = _run("nadam", "normal", 1, seed=5, b2_override=0.999)
    assert r["v"] > 100.0 and r["theta"] > oc.K_THETA, r


@pytest.mark.parametrize("rule, cls", [("nadam", nadam_numpy.Nadam), ("adam", nadam_numpy.Adam), ("sgd", nadam_numpy.SGD)])
def test_statement_iterated_is_the_oracle(rule, cls):
    rng = np.random.default_rng(9)
    theta = rng.normal(size=257) * 10.0 ** rng.integers(-4, 2, size=257)
    hyper = {} if rule == "sgd" else dict(beta_1=oc.f32(oc.BETA_1), beta_2=oc.f32(oc.BETA_2), epsilon=oc.f32(oc.EPSILON))
    ref = cls(lr=oc.f32(oc.LR), **hyper)
    a, b = theta.copy(), theta.copy()
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    for t in range(1, 21):
        g = rng.normal(size=theta.shape).astype(np.float32)
        b1, b2, eps, c_g, c_m, c_v = oc.coefficients(rule, t)
        s = oc.one_step(a, g, m, v, oc.LR, b1, b2, eps, c_g, c_m, c_v)
        a, m, v = s.theta, s.m, s.v
        b = ref.step(b, g)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (rule, t)
        if rule == "nadam":
            assert abs(oc.momentum_cache(t) - ref.m_schedule) <= 1e-15 * ref.m_schedule
        if rule != "sgd":
            assert np.abs(m - ref.m).max() <= 1e-12 * np.abs(ref.m).max() and np.abs(v - ref.v).max() <= 1e-12 * np.abs(ref.v).max()


def test_classes_are_what_they_say():
    m = oc.slots0(3, N, 2)[0]
    b1, _, _, c_g, c_m, _ = oc.coefficients("nadam", 1000)
    for cls in oc.CLASSES:
        g = oc.gradient(cls, 11, m, b1, c_g, c_m)
        assert g.dtype == np.float32 and g.shape == (N,) and np.isfinite(g).all()
        with np.errstate(over="ignore"):
            assert np.isfinite(g * g).all()                                       # (the squares beyond fp32 are a test of their own)
        assert (g == 0).all() == (cls == "zero")
    assert np.abs(oc.gradient("tiny", 11, m, b1, c_g, c_m)).max() < 1e-10 * oc.EPSILON * 1e7
    assert np.abs(oc.gradient("large", 11, m, b1, c_g, c_m)).max() > 1e17
    # cancel: the numerator is small against its two terms for a good part of the vector -- the case A exists for
    g = oc.gradient("cancel", 11, m, b1, c_g, c_m)
    s = oc.one_step(oc.theta0(3, N), g, m, oc.slots0(3, N, 2)[1], oc.LR, b1, oc.BETA_2, oc.EPSILON, c_g, c_m, 1.0)
    moved = np.abs(s.theta - oc.theta0(3, N).astype(np.float64))
    assert np.mean(moved < 1e-3 * s.A) > 0.15
    # and under every rule and from zero slots it never degenerates to zero
    for rule in oc.RULES:
        b1, _, _, c_g, c_m, _ = oc.coefficients(rule, 1)
        assert (oc.gradient("cancel", 11, np.zeros(N, np.float32), b1, c_g, c_m) != 0).all()
        assert (oc.gradient("cancel", 11, m, b1, c_g, c_m) != 0).all()
