"""Shared by tests/test_fusenet_host.py and tests/test_gpu_fusenet.py: inputs, the torch composition of FuseNet (float64 on the CPU as the check
of the numpy statement, float32 on the CPU as the independent fp32 evaluation the device's error is measured against), and the gates of a leg."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from probav_amd import fusenet_numpy as fn
from probav_amd import ops                               # noqa: F401  (registers torch.ops.probav.*)

SHAPES = [(1, 17, 17), (2, 48, 48), (1, 49, 83), (3, 40, 96)]           # (B, H, W); the shipped (1, 384, 384) is a case of its own


def params(seed=3, bias_scale=0.5):
    """Keras-range parameters with a NON-zero bias (it must have no effect) -- float32 values as float64 arrays."""
    K, bias, gamma, beta = fn.init_params(seed)
    bias = (np.random.default_rng(seed + 1).uniform(-bias_scale, bias_scale, fn.FILTERS)).astype(np.float32)
    return tuple(np.asarray(a, dtype=np.float64) for a in (K, bias, gamma, beta))


def image(shape, seed=5):
    """Integer DN in 0..16383 held as float32: a smooth field plus noise, like a stitched scene."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 6000.0 + 3000.0 * np.sin(rr / 7.0 + np.arange(B)[:, None, None]) * np.cos(cc / 11.0)
    x = np.clip(np.rint(base + rng.normal(0.0, 600.0, (B, H, W))), 0, 16383)
    return x.astype(np.float32)


def upstream(shape, seed=9):
    B, H, W = shape
    return (np.random.default_rng(seed).normal(0.0, 1.0, (B, H, W)) / (B * H * W)).astype(np.float32)


def flat_of(K, bias, gamma, beta):
    return fn.join_flat(K, bias, gamma, beta).astype(np.float32)


def torch_compose(x, K, bias, gamma, beta, dtype, g=None):
    """The network composed from torch ops on the CPU in `dtype` -> dict of numpy float64 arrays: y (with bias), a, m and, with g, the autograd
    gradients dK, dbias, dgamma, dbeta of sum(g * out)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    xt, Kt, bt, gt, be = t(x), t(K).requires_grad_(True), t(bias).requires_grad_(True), t(gamma).requires_grad_(True), t(beta).requires_grad_(True)
    xp = F.pad(xt[:, None], (fn.PAD_BEFORE, 24, fn.PAD_BEFORE, 24))
    y = F.conv2d(xp, Kt.permute(3, 2, 0, 1), bt)
    mu = y.mean((2, 3), keepdim=True)
    var = ((y - mu) ** 2).mean((2, 3), keepdim=True)
    xhat = (y - mu) / torch.sqrt(var + fn.EPS)
    a = gt.view(1, -1, 1, 1) * xhat + be.view(1, -1, 1, 1)
    m = torch.where(a >= 0, a, fn.LEAK * a).mean(1)
    out = dict(y=y, a=a, m=m)
    if g is not None:
        (m * t(g)).sum().backward()                             # d out / d params = d m / d params: x is data
        out.update(dK=Kt.grad, dbias=bt.grad, dgamma=gt.grad, dbeta=be.grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


def maxerr(a, b):
    """Max-norm error of a against b, relative to max |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def abserr(a, b):
    """Max-norm error, absolute: what the two fp32 legs are compared by (both against the same fp64 tensor)."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@functools.lru_cache(maxsize=None)
def case(shape, seed=5):
    """Everything the checks of one shape share, computed once: inputs, the fp64 statement and the CPU float32 leg with ITS errors against the
    statement (the backward judged at the float32 leg's own gates)."""
    P = params()
    x, g = image(shape, seed), upstream(shape)
    f = fn.forward(x, *P)
    c32 = torch_compose(x, *P, dtype=torch.float32, g=g)
    b32 = fn.backward(g, x, *P, gates=c32["a"] >= 0, fwd=f)
    return dict(P=P, x=x, g=g, fwd=f,
                e_cpu32_y=abserr(c32["y"], f["y"]), e_cpu32_dK=abserr(c32["dK"], b32["dK"]))


def device_gates(y_dev, stats_dev, gamma, beta):
    """The LeakyReLU gates the device took, from ITS y [B,H,W,64] and stats [B,64,2]: the kernels' float32 xhat = fl((y - mu) * rstd), then the
    sign of gamma * xhat + beta (a fused multiply-add keeps the sign of the exact value).  -> bool [B,64,H,W]."""
    y = np.asarray(y_dev, dtype=np.float32)
    mu, rs = np.asarray(stats_dev, dtype=np.float32)[:, None, None, :, 0], np.asarray(stats_dev, dtype=np.float32)[:, None, None, :, 1]
    xh = ((y - mu) * rs).astype(np.float64)
    a = np.asarray(gamma, dtype=np.float64) * xh + np.asarray(beta, dtype=np.float64)
    return (a >= 0).transpose(0, 3, 1, 2)
