"""Weight normalisation at its edges, PER OUTPUT COLUMN: wn_forward_kernel<false> / wn_backward_kernel (probav_wn_forward / probav_wn_backward)
on columns that are exactly zero, clamped (sum v^2 below tf.nn.l2_normalize's epsilon 1e-12), just not clamped, huge, and on gains that are
zero or negative -- in a layer of every column length the kernels treat differently -- and a whole training step of a network that holds such
columns, on the default fp16-piece MFMA family (an all-zero filter column is a zero amax slot there) and on an fp32 MFMA family.

The bars are the project's (tests/test_gpu_parity.py::test_weight_norm_forward_backward: 2e-6 forward, 1e-5 backward), taken per column instead of
per layer -- under a per-layer maximum a small or dead column is invisible:
    weff, weffT   2e-6 max |w_column|                                 (a zero column, a zero gain: exactly 0)
    inv_norm      exactly 1e6 for a clamped or zero column (wn_backward_kernel decides the clamp by inv >= 1e6f); 2e-6 relative otherwise
    dg            1e-5 inv sum |dw v|       the size of what is summed, not |sum dw v|: that sum cancels (a random column of 675 elements reaches
                                            1/50 of its terms' size once in 60 columns), and no fp32 summation is accurate relative to a cancelled sum
    dv            1e-5 |g inv| max (|dw| + |v proj|) over its column
Reference: oracle.wdsr_torch.weight_norm in fp64 and its autograd for a random dweff; torch.clamp has zero slope below 1e-12, which is the
kernel's proj = 0."""
import numpy as np
import pytest
import torch

from oracle import wdsr_numpy as on
from oracle import wdsr_torch as ot
from probav_amd import synth
from tests.cfg_grid import arch_of

pytestmark = pytest.mark.gpu

ZERO, CLAMPED, NEAR, HUGE, GAIN0, GAINNEG = range(6)
KINDS = ("zero", "clamped", "near", "huge", "gain0", "gain<0")
LONG_ROW = (48, 2, 6, 0.9, 43)                         # tests/cfg_grid.py: normConv columns of 27 * 43 = 1161 > WN_Q * 64 = 896 take the loop branch


@pytest.fixture(autouse=True)
def _keep_workspaces(monkeypatch):
    """The gates are read from a pass's workspace after its backward has run."""
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")


def _plant(p, rng, kinds=range(6), first=0):
    """Columns first, first + 1, ... of the layer's parameters p = {"g", "v", "bias"} become the edge columns `kinds` (in place)."""
    v = p["v"].reshape(-1, p["v"].shape[-1])                       # a view: [K, Cout]
    K = v.shape[0]
    for j, kind in enumerate(kinds):
        c = first + j
        d = rng.normal(size=K)
        d /= np.sqrt((d * d).sum())
        if kind == ZERO:
            v[:, c] = 0.0
        elif kind == CLAMPED:
            v[:, c] = (d * np.sqrt(2.5e-13)).astype(np.float32)      # a factor 4 below the epsilon: no fp32 sum can flip the decision
        elif kind == NEAR:
            v[:, c] = (d * np.sqrt(4e-12)).astype(np.float32)        # a factor 4 above
        elif kind == HUGE:
            v[:, c] = (rng.normal(size=K) * 1e15).astype(np.float32)
        elif kind == GAIN0:
            p["g"][c] = 0.0
        elif kind == GAINNEG:
            p["g"][c] = -abs(p["g"][c]) - np.float32(0.25)
    return p


def _build(dev, params, row=None):
    from probav_amd.modelsTF import WDSRConv3D
    F, R, E, decay = (32, 12, 8, 0.8) if row is None else row[:4]
    m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, F, (3, 3, 3), R, E, decay, 9, 16, True, seed=0)
    m.load_variables(params)
    return m.to(dev)


PLANTED = {None: ("mainConv1", "expConv_3", "normConv_5", "convReducer_1", "residConv2"),      # K = 27 (less than a wave), 32, 675, 864, 81 (2-D)
           LONG_ROW: ("normConv_1", "convReducer_2", "decConv_0")}                              # K = 1161, 1296 (the loop branch), 288


@pytest.mark.parametrize("row", [None, LONG_ROW], ids=["shipped", "f48-d43"])
def test_edge_columns_forward_and_backward(dev, row):
    from probav_amd import _lib as L
    arch = {} if row is None else arch_of(row)
    params = synth.synth_params(seed=23, perturb=True, **arch)
    rng = np.random.default_rng(5)
    for name in PLANTED[row]:
        assert params[name]["g"].size >= 6
        _plant(params[name], rng)
    m = _build(dev, params, row)
    if row is None:
        assert m.flat.numel() == 535267
    h = m._handle()
    nw, nc = L.lib().probav_weff_count(h), L.lib().probav_cout_total(h)
    poison = float("nan")
    weff, weffT, invn = (torch.full((n,), poison, device=dev) for n in (nw, nw, nc))
    L.check(L.lib().probav_wn_forward(h, L.ptr(m.flat), L.ptr(weff), L.ptr(weffT), L.ptr(invn), L.current_stream()), "probav_wn_forward")
    dweff_h = np.random.default_rng(6).normal(size=nw).astype(np.float32)
    dweff = torch.as_tensor(dweff_h).to(dev)
    grads = torch.full_like(m.flat.detach(), poison)
    L.check(L.lib().probav_wn_backward(h, L.ptr(m.flat), L.ptr(dweff), L.ptr(invn), L.ptr(grads), L.current_stream()), "probav_wn_backward")
    weff, weffT, invn, grads = (t.cpu().double().numpy() for t in (weff, weffT, invn, grads))
    _compare(m.layers, params, PLANTED[row], dweff_h, weff, weffT, invn, grads)


def _compare(layers, params, planted, dweff_h, weff, weffT, invn, grads):
    """The device's four outputs (fp64 copies) against the fp64 reference, column by column, every layer."""
    nw, nc = weff.size, invn.size
    off = noff = 0
    worst = {"weff": 0.0, "weffT": 0.0, "dg": 0.0, "dv": 0.0}
    for Lh in layers:
        p = params[Lh.name]
        cout = Lh.cout
        v2 = p["v"].astype(np.float64).reshape(-1, cout)
        K, n = v2.shape[0], v2.size
        g = p["g"].astype(np.float64)
        cin = p["v"].shape[-2]
        taps = K // cin
        vt = torch.tensor(p["v"], dtype=torch.float64, requires_grad=True)
        gt = torch.tensor(p["g"], dtype=torch.float64, requires_grad=True)
        wt = ot.weight_norm(vt, gt)
        dw = dweff_h[off:off + n].astype(np.float64).reshape(K, cout)
        (wt * torch.tensor(dw.reshape(p["v"].shape))).sum().backward()
        w = wt.detach().numpy().reshape(K, cout)
        assert np.abs(w - on.weight_norm(p["v"], p["g"]).reshape(K, cout)).max() <= 1e-12 * max(np.abs(w).max(), 1e-300)      # the two oracles agree
        ss = (v2 * v2).sum(0)
        clamped = ss < 1e-12
        inv = 1.0 / np.sqrt(np.maximum(ss, 1e-12))
        dot = (dw * v2).sum(0)
        proj = np.where(clamped, 0.0, dot * inv * inv)
        top = np.abs(w).max(0)
        # forward
        got = weff[off:off + n].reshape(K, cout)
        gotT = weffT[off:off + n].reshape(taps, cout, cin)
        wT = w.reshape(taps, cin, cout)[::-1].transpose(0, 2, 1)                                    # flipped taps, [tap][co][ci]
        e_w, e_wT = np.abs(got - w).max(0), np.abs(gotT - wT).max(axis=(0, 2))
        assert (e_w <= 2e-6 * top).all(), (Lh.name, "weff", int(np.argmax(e_w - 2e-6 * top)))
        assert (e_wT <= 2e-6 * top).all(), (Lh.name, "weffT", int(np.argmax(e_wT - 2e-6 * top)))
        gi = invn[noff:noff + cout]
        assert (gi[clamped] == 1e6).all(), (Lh.name, "inv_norm of a clamped column", gi[clamped])
        assert (np.abs(gi - inv) <= 2e-6 * inv).all(), (Lh.name, "inv_norm")
        # backward
        dg_ref, dv_ref = gt.grad.numpy(), vt.grad.numpy().reshape(K, cout)
        assert np.abs(dg_ref - dot * inv).max() <= 1e-9 * max(np.abs(dg_ref).max(), 1e-300)        # autograd is the formula the bars are written in
        dg_bar = 1e-5 * inv * np.abs(dw * v2).sum(0)
        dv_bar = 1e-5 * np.abs(g * inv) * (np.abs(dw) + np.abs(v2 * proj)).max(0)
        e_dg = np.abs(grads[Lh.g_off:Lh.v_off] - dg_ref)
        e_dv = np.abs(grads[Lh.v_off:Lh.b_off].reshape(K, cout) - dv_ref).max(0)
        assert (e_dg <= dg_bar).all(), (Lh.name, "dg", int(np.argmax(e_dg - dg_bar)), e_dg.max())
        assert (e_dv <= dv_bar).all(), (Lh.name, "dv", int(np.argmax(e_dv - dv_bar)), e_dv.max())
        with np.errstate(divide="ignore", invalid="ignore"):
            for key, e, bar, unit in (("weff", e_w, top, 2e-6), ("weffT", e_wT, top, 2e-6), ("dg", e_dg, dg_bar, 1.0), ("dv", e_dv, dv_bar, 1.0)):
                worst[key] = max(worst[key], float(np.nanmax(np.where(bar > 0, e / (bar * unit), 0.0))))
        if Lh.name in planted:
            assert clamped[:2].all() and not clamped[2:].any() and ss[0] == 0.0 and g[GAIN0] == 0.0 and g[GAINNEG] < 0.0 and ss[HUGE] > 1e30
            assert not got[:, ZERO].any() and not got[:, GAIN0].any() and not gotT[:, GAIN0, :].any()
            assert not grads[Lh.v_off:Lh.b_off].reshape(K, cout)[:, GAIN0].any()                   # d loss / d v through a zero gain is 0, not NaN
            print("%s (K = %d): " % (Lh.name, K) + "  ".join(
                "%s weff %.2g dg %.2g dv %.2g" % (KINDS[c], e_w[c] / (2e-6 * top[c]) if top[c] else 0.0, e_dg[c] / dg_bar[c] if dg_bar[c] else 0.0,
                                                  e_dv[c] / dv_bar[c] if dv_bar[c] else 0.0) for c in range(6)) + "   (fractions of the bars)")
        off += n
        noff += cout
    assert off == nw and noff == nc
    assert all(np.isfinite(grads[Lh.g_off:Lh.b_off]).all() for Lh in layers)                      # (the bias gradients are not this kernel's)
    print("worst over all %d columns, as fractions of the bars: %s" % (nc, {k: round(x, 4) for k, x in worst.items()}))


def _edge_network():
    """The seeded parameters with a zero-gain column and a clamped column in a normConv and in an expConv."""
    params = synth.synth_params(seed=101, perturb=True)
    rng = np.random.default_rng(8)
    for name, first in (("normConv_4", 3), ("expConv_7", 100)):
        _plant(params[name], rng, kinds=(GAIN0, CLAMPED), first=first)
        ss = (params[name]["v"].astype(np.float64).reshape(-1, params[name]["g"].size) ** 2).sum(0)
        assert params[name]["g"][first] == 0.0 and ss[first + 1] < 1e-12 / 3 and params[name]["g"][first + 1] != 0.0
    return params


def test_training_step_with_dead_and_clamped_columns_h3(dev):
    """impl 4, B = 2, T = 9: forward (2e-5 of max |ref|), loss (1e-5) and all 132 gradients at the device's ReLU gates (1e-3 per tensor), through
    tests/test_gpu_parity.py's own path.  The zero-gain column of expConv_7 is an all-zero filter column: a zero amax slot under h3_exp_w."""
    from tests.test_gpu_parity import _gate_masked_parity
    _gate_masked_parity(dev, 4, 9, 2, 1, params=_edge_network())


def test_training_step_with_dead_and_clamped_columns_fp32_mfma(dev):
    """impl 2 on the same network.  The fp32-MFMA families do not expose the gates of their fused hidden tile (probav_debug_hidden refuses them), so
    the gate-masked comparison cannot be made there: forward and loss to the same bars, gradients in relative L2 per tensor against the un-gated
    fp64 oracle at the suite's bar for that comparison (tests/test_gpu_parity.py::_grad_l2_tol, as
    test_three_channel_input_branch_on_the_fp32_families does)."""
    from probav_amd.loss import Losses
    from tests import load_golden
    from tests.test_gpu_parity import _grad_l2_tol, _model
    z = load_golden("wdsr_t9_b2")
    params = _edge_network()
    m = _model(dev, 9, params)
    m.set_impl(2)
    pred = m(torch.as_tensor(z["x"]).to(dev), training=True)
    loss = Losses(targetShape=(48, 48, 1)).shiftCompensatedL1Loss(torch.as_tensor(z["hr"]).to(dev), torch.as_tensor(z["mask"]).to(dev), pred)
    loss.backward()
    ref = on.wdsr_forward(z["x"], params, synth.NIR_MEAN, synth.NIR_STD)
    e = np.abs(pred.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max()
    assert e < 2e-5, "output rel err %.3e" % e
    _, loss_o, grads_o = ot.train_step_grads(torch.tensor(z["x"], dtype=torch.float64), torch.tensor(z["hr"]), torch.tensor(z["mask"]),
                                             ot.to_torch_params(params), synth.NIR_MEAN, synth.NIR_STD, numImgLR=9)
    assert abs(float(loss.detach()) - float(loss_o)) < 1e-5 * float(loss_o)
    gdev = m.flat.grad.detach().cpu().double().numpy()
    assert np.isfinite(gdev).all()
    worst = (0.0, None)
    for L_ in m.layers:
        for key, lo_, hi_ in (("g", L_.g_off, L_.v_off), ("v", L_.v_off, L_.b_off), ("bias", L_.b_off, L_.b_off + L_.cout)):
            r = grads_o[L_.name][key].numpy().reshape(-1)
            err = np.sqrt(((gdev[lo_:hi_] - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + 1e-30)
            worst = max(worst, (err, L_.name + "/" + key))
            assert err < _grad_l2_tol(9, 2), (L_.name, key, err)
    print("impl 2: output rel err %.3g, worst per-tensor relative L2 gradient error %.3g (%s)" % (e, worst[0], worst[1]))
