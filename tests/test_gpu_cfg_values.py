"""cfg values other than the shipped ones -- `num_filters`, `num_res_blocks`, `exp_rate`, `decay_rate` -- against the fp64 oracle, whole network, on every
kernel family.  probav_engine_create accepts any positive value for them and the engine then routes each launch by its channel counts (conv_route /
wgrad_route / mfma_pw_supported in csrc/engine.hip): a predicate that says yes to a channel count its kernel mishandles would give wrong numbers silently.
tests/cfg_grid.py lists the configurations and why each is there; tests/test_gpu_parity.py holds the same channel counts kernel by kernel.

Bars (the suite's own, none fitted): network output 2e-5 of max |ref| (north star 1e-3), loss 1e-5 relative, gradients element-wise at the device's ReLU
gates 1e-3 of each tensor's max norm wherever the gates can be read (probav_amd.introspect.device_gates: families 3 / 4 on the fused pointwise pair, every
family on the un-fused one), otherwise relative L2 per tensor against the un-gated oracle (test_gpu_parity._grad_l2_tol, 5e-3).

Every case prints the launches per kernel class of one training step (probav_engine_profile), i.e. which kernels the bars were held on: INTEGRATION.md,
'What a cfg value other than the shipped one costs', carries that table."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import wdsr_numpy as on
from oracle import wdsr_torch as ot
from probav_amd import synth
from tests.cfg_grid import GRID, VARIANTS, arch_of, case_id, pw_fused

pytestmark = pytest.mark.gpu

IMPLS = [0, 1, 2, 3, 4]
GRAD_L2_TOL = 5e-3              # tests/test_gpu_parity.py::_grad_l2_tol: one fixed bar for every depth and family (where it comes from: the comment there)
CASES = [(row, 9, True, 2) for row, _ in GRID] + VARIANTS
# engine.hip's kernel classes, in the order probav_engine_profile_read reports them
CLASSES = ["wn", "small", "conv3_fwd", "conv3_bwd_data", "conv3_wgrad", "pw_fwd", "pw_bwd_data", "pw_wgrad",
           "conv3_fwd_x6", "conv3_bwd_data_x6", "conv3_wgrad_x6", "pw_fwd_x6", "pw_bwd_data_x6"]


@pytest.fixture(autouse=True)
def _keep_workspaces(monkeypatch):
    """The gates are read from a pass's workspace after its backward has run (modelsTF.WDSRModel.forward keeps only a weak reference by default)."""
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")


def _build(dev, row, T, gray, seed, P=16):
    from probav_amd.modelsTF import WDSRConv3D
    F, R, E, decay, D = row
    arch = arch_of(row, T, gray)
    params = synth.synth_params(seed=seed, perturb=True, **arch)
    m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, F, (3, 3, 3), R, E, decay, T, P, gray, seed=0)
    assert int(m.numFilters * m.decayRate) == D
    m.load_variables(params)
    return m.to(dev), params


_oracle_cache = {}


def _oracle(row, T, gray, B, P=16):
    """Inputs, weights and the un-gated fp64 results of one configuration (numpy forward; torch forward, loss and gradients), shared by its five families.
    P: patchSizeLR (inputs of P + 6, predictions of 3 P pixels a side)."""
    key = case_id(row, T, gray, B) + ("" if P == 16 else "-p%d" % P)
    if key not in _oracle_cache:
        _oracle_cache.clear()                                   # cases run configuration by configuration: keep one
        F, R, E, decay, D = row
        C = 1 if gray else 3
        seed = 7000 + 131 * F + 17 * R + 3 * E + D + T + C + B + (0 if P == 16 else 1000 * P)
        arch = arch_of(row, T, gray)
        x, hr, mask = synth.synth_batch(B, seed=seed + 1, numImgLR=T, inChannels=C, patchSizeLR=P)
        params = synth.synth_params(seed=seed, perturb=True, **arch)
        ref = on.wdsr_forward(x, params, synth.NIR_MEAN, synth.NIR_STD, numResBlocks=R, numImgLR=T)
        pred_o, loss_o, grads_o = ot.train_step_grads(torch.tensor(x, dtype=torch.float64), torch.tensor(hr), torch.tensor(mask), ot.to_torch_params(params),
                                                      synth.NIR_MEAN, synth.NIR_STD, numResBlocks=R, numImgLR=T)
        assert pred_o.shape == ref.shape == (B, 3 * P, 3 * P, 1)
        assert np.abs(pred_o.numpy() - ref).max() < 1e-9 * np.abs(ref).max()          # the two formulations of the oracle agree at these shapes
        _oracle_cache[key] = dict(seed=seed, x=x, hr=hr, mask=mask, params=params, ref=ref, loss=float(loss_o), grads=grads_o)
    return _oracle_cache[key]


def _tensors(m):
    for L_ in m.layers:
        for key, lo, hi in (("g", L_.g_off, L_.v_off), ("v", L_.v_off, L_.b_off), ("bias", L_.b_off, L_.b_off + L_.cout)):
            yield L_.name, key, lo, hi


def _route_record(m, step):
    """Launches per kernel class of one training step, everything on the caller's stream (launches on the engine's side stream are not bracketed)."""
    from probav_amd import _lib as L
    h = m._handle()
    m.set_side_stream_mode(0)
    L.check(L.lib().probav_engine_profile(h, 1, 4096), "probav_engine_profile")
    try:
        out = step()
        torch.cuda.synchronize()
        n = len(CLASSES)
        ms, macs, cnt = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_int64 * n)()
        L.check(L.lib().probav_engine_profile_read(h, n, ms, macs, cnt), "probav_engine_profile_read")
    finally:
        L.check(L.lib().probav_engine_profile(h, 0, 0), "probav_engine_profile")
        m.set_side_stream_mode(2)
    return out, {c: int(k) for c, k in zip(CLASSES, cnt) if k}


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", CASES, ids=[case_id(*c) for c in CASES])
def test_cfg_value_matches_the_oracle(dev, case, impl):
    """Forward against the fp64 numpy oracle, loss against the fp64 torch oracle, every gradient tensor against its autograd, and the properties the README
    claims for every family: training and inference predictions equal bit for bit, a repeated step equal bit for bit, a sample's result independent of its
    batch mates bit for bit."""
    row, T, gray, B = case
    _check_against_the_oracle(dev, row, T, gray, B, impl, 16, case_id(*case))


def _check_against_the_oracle(dev, row, T, gray, B, impl, P, label):
    from probav_amd.introspect import device_gates
    from probav_amd.loss import Losses
    F, R, E, decay, D = row
    o = _oracle(row, T, gray, B, P)
    m, params = _build(dev, row, T, gray, o["seed"], P)
    m.set_impl(impl)
    lo = Losses(targetShape=(3 * P, 3 * P, 1))
    x, hr, mask = (torch.as_tensor(o[k]).to(dev) for k in ("x", "hr", "mask"))

    def step():
        m.flat.grad = None
        p = m(x, training=True)
        l = lo.shiftCompensatedL1Loss(hr, mask, p)
        l.backward()
        return p.detach().clone(), float(l), m.flat.grad.detach().clone()

    pred, loss, grad = step()
    assert tuple(pred.shape) == (B, 3 * P, 3 * P, 1) and torch.isfinite(pred).all() and torch.isfinite(grad).all()
    fused = impl >= 1 and pw_fused(F, E, D)
    gated = (not fused) or impl >= 3
    gates = device_gates(m, m.flat.detach(), B, T) if gated else None            # (before the next pass replaces the workspace)
    e_pred = np.abs(pred.cpu().double().numpy() - o["ref"]).max() / np.abs(o["ref"]).max()
    e_loss = abs(loss - o["loss"]) / o["loss"]
    # bit-for-bit properties
    pred2, loss2, grad2 = step()
    assert torch.equal(pred, pred2) and loss == loss2, "a repeated step gives another prediction"
    assert torch.equal(grad, grad2), "a repeated step gives another gradient"
    with torch.no_grad():
        assert torch.equal(m(x, training=False), pred), "inference and training predictions differ"
        assert torch.equal(m(x[:1].contiguous(), training=False), pred[:1]), "sample 0 depends on its batch mates"
    (pred3, _, grad3), routes = _route_record(m, step)
    assert torch.equal(pred, pred3) and torch.equal(grad, grad3), "the side-stream mode changes the result"
    print("cfg %s impl %d: %s pointwise pair; launches per kernel class: %s" % (label, impl, "fused" if fused else "un-fused", routes))
    print("cfg %s impl %d: output err / max |ref| = %.3g, loss rel err = %.3g" % (label, impl, e_pred, e_loss))
    assert e_pred < 2e-5, "output rel err %.3e (bar 1e-3)" % e_pred
    assert e_loss < 1e-5, "loss rel err %.3e" % e_loss
    gdev = grad.cpu().double().numpy()
    worst = (0.0, None)
    if gated:
        report = {}
        _, _, grads_o = ot.train_step_grads(torch.tensor(o["x"], dtype=torch.float64), torch.tensor(o["hr"]), torch.tensor(o["mask"]), ot.to_torch_params(params),
                                            synth.NIR_MEAN, synth.NIR_STD, numResBlocks=R, numImgLR=T, gates=gates, gate_report=report)
        assert set(gates) == set(report) and len(gates) == 2 + R + (len(m.layers) - 5 - 3 * R)      # mainConv1, residConv1, every block, every reducer
        nflip = sum(r[0][0] for r in report.values())
        worst_margin = max((r[0][1] / max(r[0][2], 1e-30)) for r in report.values())
        print("cfg %s impl %d: %d of %d ReLU gates differ between the device and the fp64 evaluation; largest |pre-activation| among them = %.3g of the layer's rms"
              % (label, impl, nflip, sum(int(np.prod(g.shape)) for g in gates.values()), worst_margin))
        assert worst_margin < 1e-4, "a gate that differs is NOT a ~0 pre-activation: the forward itself is off"
        for name, key, a, b in _tensors(m):
            r = grads_o[name][key].numpy().reshape(-1)
            e = np.abs(gdev[a:b] - r).max() / (np.abs(r).max() + 1e-30)
            if e > worst[0]:
                worst = (e, name + "/" + key)
        print("cfg %s impl %d: worst per-tensor max-norm gradient error with the device's gates: %.3g (%s)" % (label, impl, worst[0], worst[1]))
        assert worst[0] < 1e-3, worst
    else:
        for name, key, a, b in _tensors(m):
            r = o["grads"][name][key].numpy().reshape(-1)
            e = np.sqrt(((gdev[a:b] - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + 1e-30)
            if e > worst[0]:
                worst = (e, name + "/" + key)
        print("cfg %s impl %d: worst un-gated relative-L2 gradient error per tensor: %.3g (%s)" % (label, impl, worst[0], worst[1]))
        assert worst[0] < GRAD_L2_TOL, worst


SHIPPED = (32, 12, 8, 0.8, 25)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("P", [24, 17, 4], ids=["p24", "p17", "p4"])
def test_patch_size_matches_the_oracle(dev, P, impl):
    """patchSizeLR is a cfg value too (`[Patches]`): the shipped network at patch sizes other than 16, whole network, against the oracle on every kernel family, with the bars
    and the bit-for-bit properties of test_cfg_value_matches_the_oracle (test_gpu_parity.py::test_other_patch_sizes_agree_across_engines compares impl 4 with impl 0 only, in
    relative L2 of the whole flat gradient).  24: 30-wide rows -- three column ranges in conv3_w4_kernel, the general backward-filter kernel; 17: odd 23-wide rows, which
    conv3_w4_kernel declines (tests/plan_cases.py holds both kernel by kernel); 4: 10 x 10 inputs and a 12-pixel prediction, whose loss crop of 6 x 6 = 36 pixels is the
    smallest of tests/loss_cases.py.  The oracle's two formulations are asserted to agree at each of these extents (_oracle)."""
    _check_against_the_oracle(dev, SHIPPED, 9, True, 2, impl, P, "%s-p%d" % (case_id(SHIPPED), P))


@pytest.mark.parametrize("row", [(32, 3, 8, 0.82, 26), (48, 2, 6, 0.9, 43)], ids=["fused-f32-r3-e8-d26", "unfused-f48-r2-e6-d43"])
def test_optimizer_step_and_weight_cache_at_other_cfg_values(dev, row):
    """The fused optimizer + weight-norm launch and the weight cache at a fused and an un-fused configuration, as
    test_gpu_ops.py::test_fused_optimizer_weight_norm_step holds them for the shipped shape: (1) the step against the fp64 restatement of Keras Nadam,
    (2) the cached effective weights against oracle.weight_norm of the updated parameters, (3) a pass from the cache equal to a pass that recomputes the
    weights, bit for bit."""
    from oracle.nadam_numpy import Nadam
    from probav_amd import _lib as L
    from probav_amd.loss import Losses
    from probav_amd.trainClass import HipNadam, make_optimizer
    m, _ = _build(dev, row, 9, True, 4100 + row[0])
    arch = arch_of(row)
    lo = Losses(targetShape=(48, 48, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(2, seed=4200 + row[0]))
    opt = make_optimizer("nadam", m, 5e-4)
    assert isinstance(opt, HipNadam) and opt.model is m
    ref = Nadam(lr=5e-4)
    theta = m.flat.detach().cpu().double().numpy()
    for k in range(2):
        m.flat.grad = None
        assert (m.weight_cache() is not None) == (k > 0)
        lo.shiftCompensatedL1Loss(hr, mask, m(x, training=True)).backward()
        g = m.flat.grad.detach().clone()
        opt.step()
        theta = ref.step(theta, g.cpu().double().numpy())
        assert np.abs(m.flat.detach().cpu().double().numpy() - theta).max() < 2e-6 * np.abs(theta).max()          # (1)
    wc = m.weight_cache()
    assert wc is not None
    params = synth.unflatten_params(m.flat.detach().cpu().numpy(), **arch)
    nw = L.lib().probav_weff_count(m._handle())
    weff = wc[:nw].cpu().double().numpy()
    off = 0
    for Lh in m.layers:                                                                                           # (2)
        w = on.weight_norm(params[Lh.name]["v"], params[Lh.name]["g"])
        assert np.abs(weff[off:off + w.size].reshape(w.shape) - w).max() < 2e-6 * np.abs(w).max(), Lh.name
        off += w.size
    assert off == nw
    m.flat.grad = None                                                                                            # (3)
    y_c = m(x, training=True)
    lo.shiftCompensatedL1Loss(hr, mask, y_c).backward()
    g_c = m.flat.grad.detach().clone()
    m._wcache_version = None                                            # drop the cache: the same parameters, everything recomputed
    m.flat.grad = None
    y_r = m(x, training=True)
    lo.shiftCompensatedL1Loss(hr, mask, y_r).backward()
    assert torch.equal(y_c, y_r) and torch.equal(g_c, m.flat.grad)
