"""The one-step statement of the optimizer update kernels (csrc/kernels_small.hip: nadam_kernel, nadam_guard_kernel, wn_forward_kernel<true>,
wn_forward_guard_kernel), in fp64, with the error bounds the device is held to per element.  One module serves
tests/test_optim_cases_host.py (an fp32 numpy emulation of the rule against the bounds, and the statement against oracle/nadam_numpy.py: no
GPU) and tests/test_gpu_optim_rule.py (the kernels).

The statement
    g' = fl32(g * scale)                      (only when a scale is given: the clip of the control block)
    m' = b1 m + (1 - b1) g'                   v' = b2 v + (1 - b2) g'^2
    theta' = theta - lr (c_g g' + c_m m') / (sqrt(v' c_v) + eps)
    ema'   = mom ema + (1 - mom) theta'
lr, b1, b2, eps and mom enter AT THEIR FP32 VALUES, as the C ABI passes them and as Keras holds its hyperparameters; 1 - b1 and 1 - b2 are
formed exactly from those values.  c_g, c_m, c_v are the host's doubles (their rounding on the way into the kernel is part of the bound).
With b2 = 0.999 in double the statement would be off by (1 - fl32(0.999)) / 0.001 - 1 = 1.3e-5 in v, 216 units of 2^-24: no tight bound
could hold.

The comparison is per step from the DEVICE'S OWN previous state (theta, m, v, ema read back before the step): nothing accumulates, and the
bounds are counted, not tuned.  u = 2^-24; A = lr (|c_g g'| + |c_m m'|) / (sqrt(v' c_v) + eps) (not |theta' - theta|: the numerator may
cancel); M = b1 |m| + (1 - b1) |g'|.  Where c_g = 0 (Adam) A takes M for |m'|: m' is then the WHOLE numerator, its own two terms may cancel
(b1 m = -(1 - b1) g', which N(0, 1) gradients reach to 1/40 within 4 099 elements at step 2), and the 1.5 u M that any fp32 evaluation of m'
is off by is then not small against |m'|: a correctly rounded evaluation misses 16 u A with |m'| by a factor of 8 there (host test).  With
c_g != 0 the same cancellation leaves c_g |g'| ~ 9 c_g |m| in A against a carried 2.7 u c_m |m|, and c_m <= 9 c_g throughout Nadam's schedule.

    |theta_dev - theta'| <= 16 u A + 1/2 ulp32(theta')
        numerator: c_g, c_m, two products, one sum, the product with lr; denominator: c_v, v c_v, the square root (halves the relative
        error of its argument), the sum with eps; the quotient; the carried errors of m' and v': under 12 u.  16 leaves room for the count,
        not for the kernel.  The 1/2 ulp is the final store.
    |m_dev - m'|         <= 3 u M                          (two products and a sum; fl32(1 - b1))
    |v_dev - v'|         <= 4 u v' + 2^-149                (three products and a sum; the floor is the fp32 denormal spacing)
    |ema_dev - ema'|     <= 3 u (mom |ema| + (1 - mom) |theta'|) + 16 u A
Fused multiply-adds only remove roundings.

Worst ratios seen (error beyond the 1/2 ulp or the denormal floor, over u times the bound's magnitude; the bounds are 16 / 3 / 4 / 3).  Device:
MI355X, every case of tests/test_gpu_optim_rule.py.  A device ratio above the bound is a finding to explain from the kernel's text, not a reason
to raise the bound.
                                                theta (u A)   m (u M)   v (u v')   ema
    fp32 numpy emulation, no fma (host test)    4.91          1.87      2.64       2.28
    nadam_kernel                                5.44          1.94      2.75       -
    nadam_guard_kernel                          5.19          1.94      2.76       2.06
    wn_forward_kernel<true>                     4.97          1.89      2.78       -
    wn_forward_guard_kernel                     4.91          1.90      2.82       1.97
"""
import collections
import functools

import numpy as np

U = 2.0 ** -24
DENORM = 2.0 ** -149
K_THETA, K_M, K_V, K_EMA = 16.0, 3.0, 4.0, 3.0

RULES = ("nadam", "adam", "sgd")
CLASSES = ("normal", "zero", "tiny", "mixed", "cancel", "large")
STEPS = (1, 2, 1000, 250001)
LR, BETA_1, BETA_2, EPSILON, SCHEDULE_DECAY = 5e-4, 0.9, 0.999, 1e-7, 0.004

Step = collections.namedtuple("Step", "theta m v ema A M g")


def f32(x):
    """The fp32 value of a hyperparameter, as a double."""
    return float(np.float32(x))


# ---- the schedule: oracle/nadam_numpy.py's formulas, hyperparameters at their fp32 values ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cache_table(upto, b1, decay):
    """Running products Pi_0 .. Pi_upto of mu_i = b1 (1 - 0.5 0.96^(i decay)), multiplied up in the oracle's order."""
    out = np.empty(upto + 1)
    p = 1.0
    out[0] = p
    for i in range(1, upto + 1):
        p = p * (b1 * (1.0 - 0.5 * 0.96 ** (i * decay)))
        out[i] = p
    return out


def momentum_cache(t, beta_1=BETA_1, schedule_decay=SCHEDULE_DECAY):
    """Pi_t: oracle.nadam_numpy.Nadam.m_schedule after t steps (Keras's `momentum_cache`)."""
    size = 1024 if t <= 1024 else 250016 if t <= 250016 else t
    return float(_cache_table(size, f32(beta_1), schedule_decay)[t])


def coefficients(rule, t, beta_1=BETA_1, beta_2=BETA_2, epsilon=EPSILON, schedule_decay=SCHEDULE_DECAY):
    """(b1, b2, eps, c_g, c_m, c_v) of step t >= 1 as trainClass.HipNadam / HipAdam / HipSGD pass them, from the oracle's schedule."""
    b1, b2 = f32(beta_1), f32(beta_2)
    if rule == "nadam":
        mu_t = b1 * (1.0 - 0.5 * 0.96 ** (t * schedule_decay))
        mu_t1 = b1 * (1.0 - 0.5 * 0.96 ** ((t + 1) * schedule_decay))
        pi_t = momentum_cache(t - 1, beta_1, schedule_decay) * mu_t
        pi_t1 = pi_t * mu_t1
        return b1, b2, epsilon, (1.0 - mu_t) / (1.0 - pi_t), mu_t1 / (1.0 - pi_t1), 1.0 / (1.0 - b2 ** t)
    if rule == "adam":
        return b1, b2, epsilon, 0.0, np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), 1.0
    assert rule == "sgd"
    return 0.0, 1.0, 1.0, 1.0, 0.0, 0.0


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------------
def one_step(theta, g, m, v, lr, b1, b2, eps, c_g, c_m, c_v, scale=1.0, ema=None, ema_mom=None):
    """One update in fp64 -> Step(theta', m', v', ema' or None, A, M, g')."""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    theta, m, v = (np.asarray(a, np.float64) for a in (theta, m, v))
    g = np.asarray(g, np.float32)
    if scale is not None and scale != 1.0:
        with np.errstate(over="ignore"):
            g = g * np.float32(scale)                                 # one fp32 rounding, as the guarded kernels multiply
    g = g.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        M = b1 * np.abs(m) + (1.0 - b1) * np.abs(g)
        m1 = b1 * m + (1.0 - b1) * g
        v1 = b2 * v + (1.0 - b2) * g * g
        den = np.sqrt(v1 * c_v) + eps
        theta1 = theta - lr * (c_g * g + c_m * m1) / den
        A = lr * (np.abs(c_g * g) + np.abs(c_m) * (np.abs(m1) if c_g != 0.0 else M)) / den      # (module docstring: c_g = 0)
    ema1 = None
    if ema is not None:
        mom = f32(ema_mom)
        ema1 = mom * np.asarray(ema, np.float64) + (1.0 - mom) * theta1
    return Step(theta1, m1, v1, ema1, A, M, g)


def ulp32(x):
    """Spacing of fp32 at |x| (x in fp64), no smaller than the denormal spacing."""
    with np.errstate(over="ignore"):
        return np.maximum(np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64), DENORM)


def ratios(ref, theta, m, v, ema=None, ema_prev=None, ema_mom=None):
    """Worst error of (theta, m, v, ema) against the statement `ref`, each as a multiple of u times its bound's magnitude (the 1/2 ulp and the
    denormal floor taken off first): {"theta", "m", "v", "ema"} -- to be held below K_THETA, K_M, K_V, K_EMA.  An error where the magnitude
    is zero and the floor does not cover it counts as inf."""
    def worst(err, floor, scale):
        over = np.maximum(np.abs(err) - floor, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(over == 0.0, 0.0, over / (U * scale))
        return float(np.max(r)) if r.size else 0.0
    out = {"theta": worst(np.asarray(theta, np.float64) - ref.theta, 0.5 * ulp32(ref.theta), ref.A),
           "m": worst(np.asarray(m, np.float64) - ref.m, 0.0, ref.M),
           "v": worst(np.asarray(v, np.float64) - ref.v, DENORM, ref.v)}
    if ema is not None:
        mom = f32(ema_mom)
        mag = mom * np.abs(np.asarray(ema_prev, np.float64)) + (1.0 - mom) * np.abs(ref.theta)
        out["ema"] = worst(np.asarray(ema, np.float64) - ref.ema, K_THETA * U * ref.A, mag)
    return out


def within(r):
    return r["theta"] <= K_THETA and r["m"] <= K_M and r["v"] <= K_V and r.get("ema", 0.0) <= K_EMA


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def theta0(seed, n):
    rng = np.random.default_rng([seed, 1])
    return (rng.normal(size=n) * 10.0 ** rng.integers(-4, 2, size=n)).astype(np.float32)


def slots0(seed, n, t):
    """(m, v) before step t: zero for t = 1 (a fresh optimizer), seeded otherwise (a restored one)."""
    if t == 1:
        return np.zeros(n, np.float32), np.zeros(n, np.float32)
    rng = np.random.default_rng([seed, 2])
    return (1e-2 * rng.normal(size=n)).astype(np.float32), (1e-4 * rng.normal(size=n) ** 2).astype(np.float32)


def gradient(cls, seed, m, b1, c_g, c_m):
    """The gradient of class `cls` for a step whose first moment is `m` (fp32, the device's own) and whose coefficients are b1, c_g, c_m.
      normal  N(0, 1)                         zero    0
      tiny    1e-12 N(0, 1)                   mixed   N(0, 1) 10^U{-18..9}
      large   1e17 N(0, 1): g^2 is finite in fp32 (5.5 sigma squared is 3e35)
      cancel  aims at the numerator c_g g + c_m m' = (c_g + c_m (1 - b1)) g + c_m b1 m.  First half of the vector: g = -c_m m / c_g (1 + d),
              the cancellation against the OLD moment; second half: g = -c_m b1 m / (c_g + c_m (1 - b1)) (1 + d), against the new one;
              d = +-10^U{-7..0}.  Where that is undefined or zero (c_g = 0: the first form under Adam; c_m = 0: SGD; m = 0: a fresh
              optimizer) the element is N(0, 1): the class never degenerates to `zero`."""
    n = m.size
    rng = np.random.default_rng([seed, 3])
    z = rng.normal(size=n)
    if cls == "normal":
        g = z
    elif cls == "zero":
        g = np.zeros(n)
    elif cls == "tiny":
        g = 1e-12 * z
    elif cls == "mixed":
        g = z * 10.0 ** rng.integers(-18, 10, size=n)
    elif cls == "large":
        g = 1e17 * z
    else:
        assert cls == "cancel"
        d = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.integers(-7, 1, size=n)
        md = np.asarray(m, np.float64)
        first = np.arange(n) < n // 2
        full = c_g + c_m * (1.0 - f32(b1))
        with np.errstate(divide="ignore", invalid="ignore"):
            old = -c_m * md / c_g * (1.0 + d) if c_g != 0.0 else np.zeros(n)
            new = -c_m * f32(b1) * md / full * (1.0 + d) if full != 0.0 else np.zeros(n)
        g = np.where(first & (c_g != 0.0), old, new)
        g = np.where(np.isfinite(g) & (g != 0.0), g, z)
    return g.astype(np.float32)


# ---- the rule in fp32, every operation rounded on its own (no fused multiply-add): the CPU stand-in for a kernel ----------------------------------
def emulate_step(theta, g, m, v, lr, b1, b2, eps, c_g, c_m, c_v, scale=1.0, ema=None, ema_mom=None):
    F = np.float32
    lr, b1, b2, eps, c_g, c_m, c_v = (F(x) for x in (lr, b1, b2, eps, c_g, c_m, c_v))
    theta, g, m, v = (np.asarray(a, F) for a in (theta, g, m, v))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if scale != 1.0:
            g = g * F(scale)
        m1 = b1 * m + (F(1) - b1) * g
        v1 = b2 * v + ((F(1) - b2) * g) * g
        theta1 = theta - (lr * (c_g * g + c_m * m1)) / (np.sqrt(v1 * c_v) + eps)
        ema1 = None
        if ema is not None:
            mom = F(ema_mom)
            ema1 = mom * np.asarray(ema, F) + (F(1) - mom) * theta1
    assert theta1.dtype == m1.dtype == v1.dtype == F
    return theta1, m1, v1, ema1
