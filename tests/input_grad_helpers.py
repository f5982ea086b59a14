"""References of the input-gradient tests (tests/test_gpu_input_grad.py): the fp64 autograd oracle taken down to the LR frames, and an fp64 numpy
statement of the formula probav_input_grad evaluates (include/probav_hip.h).  Test infrastructure: the product path imports nothing from here or
from `oracle`."""
import numpy as np
import torch

from oracle import wdsr_torch as ot


def oracle_input_grad(x, hr, mask, params, mean, std, T, gates=None):
    """-> (d loss / d x [B, H, H, T, C] float64, loss): x an fp64 LEAF, forward at `gates` (the device's ReLU decisions, or None: the oracle's own),
    shift-compensated L1 loss, torch.autograd.grad(loss, [x]) -- what tf.GradientTape gives for tape.gradient(loss, x)."""
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    pt = ot.to_torch_params(params, requires_grad=False)
    pred = ot.wdsr_forward(xt, pt, mean, std, numImgLR=T, gates=gates)
    loss = ot.shift_l1_loss(torch.tensor(np.asarray(hr)), torch.tensor(np.asarray(mask)), pred)
    (dx,) = torch.autograd.grad(loss, [xt])
    return dx.numpy(), float(loss.detach())


def input_grad_numpy(g, act0, wmain, d1, gate1, w1, std):
    """The formula, in fp64:  dx[n,h,w,t,c] = 1/std * ( sum_{a,b,d,co} G[n,h+1-a,w+1-b,t+1-d,co] wmain[a,b,d,c,co]
                                                      + 1/T sum_{a,b,co} D1[n,h-a,w-b,co] w1[a,b,0,c,co] ),  out-of-range indices contribute 0,
    G = g where act0 > 0 else 0, D1 = d1 where gate1 > 0 (gate1 None: d1).  -> (dx, main share, residual share), the shares already over std."""
    g, act0, wmain, d1, w1 = (np.asarray(a, dtype=np.float64) for a in (g, act0, wmain, d1, w1))
    B, H, W, T, _ = g.shape
    C = wmain.shape[3]
    G = np.where(act0 > 0, g, 0.0)
    Gp = np.pad(G, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))
    main = np.zeros((B, H, W, T, C))
    for a in range(3):
        for b in range(3):
            for d in range(3):
                main += np.einsum("nhwto,co->nhwtc", Gp[:, 2 - a:2 - a + H, 2 - b:2 - b + W, 2 - d:2 - d + T], wmain[a, b, d])
    D1 = d1 if gate1 is None else np.where(np.asarray(gate1, dtype=np.float64) > 0, d1, 0.0)
    Dp = np.pad(D1, ((0, 0), (2, 2), (2, 2), (0, 0)))
    res = np.zeros((B, H, W, C))
    for a in range(3):
        for b in range(3):
            res += np.einsum("nhwo,co->nhwc", Dp[:, 2 - a:2 - a + H, 2 - b:2 - b + W], w1[a, b, 0])
    res = np.broadcast_to(res[:, :, :, None, :] / T, main.shape)
    return (main + res) / std, main / std, res / std
