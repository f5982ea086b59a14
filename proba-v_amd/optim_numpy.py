"""The guarded optimizer step stated in fp64 numpy: what `probav_grad_guard` and the `*_guarded` update launches compute, in the style of
`tiles.tile_blend_numpy` -- the definition the device is held to (tests/test_gpu_optim_guard.py), not a code path of the product.

One step, from the flat gradient g (all 132 tensors as one vector, as the trainer holds them):

    total = sum g^2           norm = sqrt(total)                                   tf.linalg.global_norm
    scale = clipnorm / max(norm, clipnorm)     (1 without clipping)                tf.clip_by_global_norm = Keras `global_clipnorm`
    skip  = skip_nonfinite and not isfinite(total)                                 (no Keras counterpart: the guard)
    g'    = g * scale
    m = b1 m + (1 - b1) g' ;  v = b2 v + (1 - b2) g'^2
    theta = theta - lr (c_g g' + c_m m) / (sqrt(c_v v) + eps)                      Keras Nadam / Adam / SGD by coefficients (`coefficients`)
    ema   = ema_momentum ema + (1 - ema_momentum) theta                            Keras `use_ema` / `ema_momentum`: no de-biasing, ema_0 = theta_0

A skipped step leaves theta, m, v and ema as they were and counts one in `skipped_total`.  The step counter t and the Nadam momentum
schedule are the HOST's: they advance on a skipped step too, because the host never learns whether a step was skipped (finding out would be
the synchronisation the device-side guard exists to avoid).  A non-finite total with clipping on and the guard off gives scale = NaN, hence
NaN parameters, as tf.clip_by_global_norm does.
"""
import numpy as np


def global_norm(g):
    """(total, norm) of the flat gradient in fp64.  A finite fp32 squared is below 2^256: the total is non-finite exactly when an element is."""
    g = np.asarray(g, np.float64).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        total = float(np.sum(g * g))
    return total, float(np.sqrt(total)) if total == total and total >= 0 else float("nan")


def clip_scale(norm, clipnorm):
    """clipnorm / max(norm, clipnorm) in fp64; 1 when clipping is off (None or <= 0); NaN for a non-finite norm (tf.clip_by_global_norm)."""
    if clipnorm is None or clipnorm <= 0:
        return 1.0
    if not np.isfinite(norm):
        return float("nan")
    return float(clipnorm) / max(float(norm), float(clipnorm))


def guard_control(g, global_clipnorm=None, skip_nonfinite=False):
    """The control block of one step: {norm, scale (fp64, before its one rounding to fp32), skip}."""
    total, norm = global_norm(g)
    return {"norm": norm, "scale": clip_scale(norm, global_clipnorm), "skip": bool(skip_nonfinite and not np.isfinite(total))}


def coefficients(name, t, momentum_cache=1.0, beta_1=0.9, beta_2=0.999, epsilon=1e-7, schedule_decay=0.004):
    """(b1, b2, eps, c_g, c_m, c_v, new momentum cache) of step t >= 1 for 'nadam', 'adam' or anything else (SGD): the coefficients
    trainClass.HipNadam / HipAdam / HipSGD hand to the one update kernel."""
    if name == "nadam":
        mu_t = beta_1 * (1.0 - 0.5 * 0.96 ** (t * schedule_decay))
        mu_t1 = beta_1 * (1.0 - 0.5 * 0.96 ** ((t + 1) * schedule_decay))
        pi_t = momentum_cache * mu_t
        return beta_1, beta_2, epsilon, (1.0 - mu_t) / (1.0 - pi_t), mu_t1 / (1.0 - pi_t * mu_t1), 1.0 / (1.0 - beta_2 ** t), pi_t
    if name == "adam":
        return beta_1, beta_2, epsilon, 0.0, (1.0 - beta_2 ** t) ** 0.5 / (1.0 - beta_1 ** t), 1.0, momentum_cache
    return 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, momentum_cache          # (beta_2 = 1: v stays 0 -- with 0 the fp32 kernel would form g * g, inf for |g| > 1.85e19)


def update(theta, g, m, v, lr, b1, b2, eps, c_g, c_m, c_v):
    """The one update rule (csrc/kernels_small.hip: opt_update) -> (theta, m, v)."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return theta - lr * (c_g * g + c_m * m) / (np.sqrt(v * c_v) + eps), m, v


def ema_update(ema, theta, ema_momentum):
    return ema_momentum * ema + (1.0 - ema_momentum) * theta


class GuardedOptimizer:
    """The trainer's optimizer with its options, step by step in fp64.  `step(theta, g)` returns the new parameters; `m`, `v`, `ema`, `t`,
    `skipped_total` and the last step's `control` are attributes."""

    def __init__(self, name, lr, global_clipnorm=None, skip_nonfinite=False, use_ema=False, ema_momentum=0.99, **hyper):
        self.name, self.lr, self.hyper = name, lr, hyper
        self.global_clipnorm, self.skip_nonfinite, self.use_ema, self.ema_momentum = global_clipnorm, skip_nonfinite, use_ema, ema_momentum
        self.t, self.momentum_cache, self.m, self.v, self.ema = 0, 1.0, None, None, None
        self.skipped_total, self.control = 0, None

    def step(self, theta, g):
        theta, g = np.asarray(theta, np.float64), np.asarray(g, np.float64)
        if self.m is None:
            self.m, self.v = np.zeros_like(theta), np.zeros_like(theta)
            self.ema = theta.copy() if self.use_ema else None
        self.t += 1                                                  # the host's count: a skipped step advances it (module docstring)
        b1, b2, eps, c_g, c_m, c_v, self.momentum_cache = coefficients(self.name, self.t, self.momentum_cache, **self.hyper)
        self.control = guard_control(g, self.global_clipnorm, self.skip_nonfinite)
        if self.control["skip"]:
            self.skipped_total += 1
            return theta
        with np.errstate(over="ignore", invalid="ignore"):
            theta, self.m, self.v = update(theta, g * self.control["scale"], self.m, self.v, self.lr, b1, b2, eps, c_g, c_m, c_v)
        if self.use_ema:
            self.ema = ema_update(self.ema, theta, self.ema_momentum)
        return theta
