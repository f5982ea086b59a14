"""The general matrix route on the 16-bit matrix pipe, on the device (csrc/kernels_gemm_x6.hip; include/probav_hip.h, 'the route on the 16-bit matrix pipe').

The kernel (gemm_conv_fwd_x6_kernel; the backward-filter stays the fp32 route's) has no single-operator entry point: it is reached, and held, through probav_forward / probav_backward* / probav_debug_hidden on engines
whose probav_engine_gemm_arith is 1 -- every test asserts that first (a library without the switch ignores PROBAV_GEMM_X6 and would pass the oracle checks on
the fp32 route).  The whole network against the fp64 oracle with tests/test_gpu_cfg_values.py's check and bars, unchanged; every route launch of a training
forward against the fp64 single-operator oracle of tests/test_gpu_parity.py at that module's bar; the x6 route against the fp32 route; the switch toggled
between steps and flipped between a forward and its backward; the guard bands of tests/bands.py; non-finite inputs and gradients; the CLIs.

Rows are (F, R, E, decay, D), T, gray, B, P -- the smallest shapes at which each tiling decision can go wrong: a K tail of 51 = 3 x 16 + 3, two N tiles and M
tiles that straddle samples (1), tails on both sides (2), H3 neighbours that want amax slots at impl 4 (3), less than one K chunk, fewer voxels than one M tile
and slabs with a ragged end (4: P = 4), depth 7 (5), three input channels, mirrored pads and depth 13 (6), and Cout = 72 / 144: the NT = 4 instance with a
tail, beyond the pair's range, so that the pointwise launches are x6 whatever the pair's switch (7)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests import bands
from tests.test_gemm_route_host import make_engine
from tests.test_gpu_gemm_pair import _L, _layer, _view
from tests.test_gpu_gemm_route import _same
from tests.test_gpu_parity import _oracle_conv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32

ROWS = [((64, 2, 8, 0.8, 51), 9, True, 3, 16), ((48, 2, 6, 0.9, 43), 9, True, 2, 16), ((32, 2, 8, 0.9, 28), 9, True, 2, 16), ((20, 1, 3, 0.5, 10), 9, True, 2, 4),
        ((16, 2, 8, 0.75, 12), 7, True, 2, 16), ((64, 1, 8, 0.8, 51), 13, False, 2, 16), ((72, 1, 2, 0.8, 57), 9, True, 2, 8)]
# reducers by frame count: (H/W pad, depth pad, mirrored H/W pad) of each 3x3x3 layer (csrc/engine.hip: redSpec)
REDUCERS = {9: [(1, 0, 1), (0, 0, 0), (0, 0, 0)], 13: [(1, 0, 1)] * 3 + [(0, 0, 0)] * 2, 7: [(0, 0, 0)] * 2}


def _id(c):
    return "f%d-r%d-e%d-d%d-t%d-b%d-p%d" % (c[0][0], c[0][1], c[0][2], c[0][4], c[1], c[3], c[4])


def _pair_takes(row):
    return row[0] <= 64 and row[4] <= 64


def _arith(m):
    return _L().lib().probav_engine_gemm_arith(m._handle())


def _kind(m):
    return _L().lib().probav_engine_pair_kind(m._handle())


def _model(dev, row, T=9, gray=True, seed=11, P=16, impl=None, pair=False, x6=True):
    """The network on the route in x6 arithmetic: probav_engine_gemm_arith == 1, or the test has nothing to say."""
    from tests import test_gpu_cfg_values as cv
    m = cv._build(dev, row, T, gray, seed, P)[0]
    if impl is not None:
        m.set_impl(impl)
    m.set_gemm_route(True)
    m.set_gemm_pair(pair)
    m.set_gemm_x6(x6)
    assert m.gemm_x6 is bool(x6) and _arith(m) == (1 if x6 else 0) and _kind(m) == (2 if pair and _pair_takes(row) else 0)
    return m


def _stepper(dev, m, B=2, T=9, C=1, P=16, seed=12):
    from probav_amd import synth
    from probav_amd.loss import Losses
    lo = Losses(targetShape=(3 * P, 3 * P, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=seed, numImgLR=T, inChannels=C, patchSizeLR=P))

    def step():
        m.flat.grad = None
        p = m(x, training=True)
        l = lo.shiftCompensatedL1Loss(hr, mask, p)
        l.backward()
        return p.detach().clone(), float(l), m.flat.grad.detach().clone()
    return step


@pytest.fixture(autouse=True)
def _keep_workspaces(monkeypatch):
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")                      # the gates and the saved activations are read from a pass's workspace


@pytest.fixture(scope="module", autouse=True)
def _release_the_arena(dev):
    yield
    bands.release(dev)


# ---- 1. the whole network against the fp64 oracle ---------------------------------------------------------------------------------------------------
NET = [(c, impl, pair) for c in ROWS for pair in (False, True) if not pair or _pair_takes(c[0]) for impl in (1, 4)]      # (row outermost: one oracle per row)


@pytest.mark.parametrize("case,impl,pair", NET, ids=["%s-impl%d-pair%d" % (_id(c), i, p) for c, i, p in NET])
def test_whole_network_in_x6_matches_the_oracle(dev, case, impl, pair, monkeypatch):
    """tests/test_gpu_cfg_values.py::_check_against_the_oracle, unchanged, on engines created with PROBAV_GEMM_ROUTE=1 PROBAV_GEMM_X6=1 (and PROBAV_GEMM_PAIR=1):
    output 2e-5, loss 1e-5, every gradient tensor 1e-3 at the device's gates, and its bit-for-bit properties: repeated step, training = inference, sample alone,
    side-stream mode."""
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    monkeypatch.setenv("PROBAV_GEMM_ROUTE", "1")
    monkeypatch.setenv("PROBAV_GEMM_X6", "1")
    if pair:
        monkeypatch.setenv("PROBAV_GEMM_PAIR", "1")
    else:
        monkeypatch.delenv("PROBAV_GEMM_PAIR", raising=False)
    lib = _L().lib()
    h = make_engine(lib, row[0], row[1], row[2], row[4], T, 1 if gray else 3, P)
    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_gemm_arith(h) == 1 and lib.probav_engine_pair_kind(h) == (2 if pair else 0)
    lib.probav_engine_destroy(h)
    built = []
    build = cv._build
    monkeypatch.setattr(cv, "_build", lambda *a, **kw: built.append(build(*a, **kw)) or built[-1])
    cv._check_against_the_oracle(dev, row, T, gray, B, impl, P, "gemm-x6 %s pair %d" % (_id(case), pair))
    assert len(built) == 1 and _arith(built[0][0]) == 1 and built[0][0].gemm_x6 is True and _kind(built[0][0]) == (2 if pair else 0)       # the engine the check ran on


# ---- 2. layer by layer ------------------------------------------------------------------------------------------------------------------------------
def _err(y, ref):
    return float(np.abs(y.cpu().double().numpy().reshape(ref.shape) - ref).max() / np.abs(ref).max())


LAYERED = [(ROWS[0], 4, False), (ROWS[0], 1, True), (ROWS[3], 4, False), (ROWS[5], 4, False), (ROWS[6], 1, False), (ROWS[6], 4, True)]


@pytest.mark.parametrize("case,impl,pair", LAYERED, ids=["%s-impl%d-pair%d" % (_id(c), i, p) for c, i, p in LAYERED])
def test_every_route_launch_of_a_forward_matches_the_single_operator_oracle(dev, case, impl, pair):
    """After a training forward: normConv_i of the saved DEC[i] with its effective filter, bias and skip ACT[i] against ACT[i + 1]; every reducer from its input;
    with the pair un-fused, expConv_i (the hidden tensor, as probav_debug_hidden recomputes it with the route's launch) from ACT[i] and decConv_i from it against
    DEC[i].  tests/test_gpu_parity.py::_oracle_conv in fp64, bar 2e-6 of max |ref|: the route's own single-operator bar, which the x6 kernels of impl 3 meet there."""
    from probav_amd import introspect
    row, T, gray, B, P = case
    F, R, E, decay, D = row
    H, hin = F * E, P + 6
    m = _model(dev, row, T, gray, P=P, impl=impl, pair=pair)
    fused = _kind(m) == 2
    _stepper(dev, m, B, T, 1 if gray else 3, P)()
    assert _arith(m) == 1
    L = _L()
    flat = m.flat.detach()
    weff = introspect._effective_weights(m, flat, m.weight_cache())

    def filt(name):
        Lh, off = _layer(m, name)
        n = Lh.b_off - Lh.v_off
        return weff[off: off + n].cpu().numpy().reshape(Lh.vshape), flat[Lh.b_off: Lh.b_off + Lh.cout].cpu().numpy()

    def act(kind, i, C, h=hin, t=T):
        return _view(m, B, kind, i).cpu().numpy().reshape(B, h, h, t, C)
    worst = 0.0
    for i in range(R):
        a0, dec = act(0, i, F), act(1, i, D)
        w, b = filt("normConv_%d" % i)
        e = _err(_view(m, B, 0, i + 1), _oracle_conv(dec, None, w, b, a0, (1, 1, 1), 0, 0, (hin, hin, T)))
        print("gemm x6 %s impl %d normConv_%d: err / max |ref| = %.3g" % (_id(case), impl, i, e))
        worst = max(worst, e)
        if not fused:
            ws = m._workspace(B, True)
            hid = torch.full((B * hin * hin * T * H,), float("nan"), device=dev)
            scr = torch.empty(B * hin * hin * T * D, device=dev)
            L.check(L.lib().probav_debug_hidden(m._handle(), L.ptr(flat), L.ptr(ws), ws.numel() * 4, B, i, L.ptr(hid), L.ptr(scr), L.ptr(m.weight_cache()), L.current_stream()),
                    "probav_debug_hidden")
            w1, b1 = filt("expConv_%d" % i)
            w2, b2 = filt("decConv_%d" % i)
            eh = _err(hid, _oracle_conv(a0, None, w1, b1, None, (0, 0, 0), 0, 1, (hin, hin, T)))
            ed = _err(_view(m, B, 1, i), _oracle_conv(hid.cpu().numpy().reshape(B, hin, hin, T, H), None, w2, b2, None, (0, 0, 0), 0, 0, (hin, hin, T)))
            print("gemm x6 %s impl %d expConv_%d: %.3g, decConv_%d: %.3g" % (_id(case), impl, i, eh, i, ed))
            worst = max(worst, eh, ed)
    x, h, t = act(0, R, F), hin, T
    for k, (p, pt, refl) in enumerate(REDUCERS[T]):
        ho, to = h + 2 * p - 2, t + 2 * pt - 2
        w, b = filt("convReducer_%d" % (k + 1))
        y = _view(m, B, 2, k)
        e = _err(y, _oracle_conv(x, None, w, b, None, (p, p, pt), refl, 1, (ho, ho, to)))
        print("gemm x6 %s impl %d convReducer_%d: err / max |ref| = %.3g" % (_id(case), impl, k + 1, e))
        worst = max(worst, e)
        x, h, t = y.cpu().numpy().reshape(B, ho, ho, to, F), ho, to
    assert worst < 2e-6, worst


# ---- 3. against the fp32 route ----------------------------------------------------------------------------------------------------------------------
AGAINST = [(ROWS[3], 1, False), (ROWS[3], 4, True), (ROWS[4], 4, False), (ROWS[6], 4, False)]


@pytest.mark.parametrize("case,impl,pair", AGAINST, ids=["%s-impl%d-pair%d" % (_id(c), i, p) for c, i, p in AGAINST])
def test_x6_against_the_fp32_route(dev, case, impl, pair):
    """The same weights and inputs with the switch off -- the behaviour before the switch existed: prediction within 2e-6 of its max norm, every gradient tensor
    within 1e-5 of its max norm (tests/test_gpu_gemm_pair.py's bar for the same comparison).  The two forwards differ by rounding, so a ReLU gate could differ and
    move a gradient by a whole term: the test first asserts that every gate (mainConv1, the hidden tensors, the reducers, residConv1) is the same on both engines
    for its fixed seed -- a failure there says so, and calls for another fixed seed, not for a wider bar."""
    from probav_amd.introspect import device_gates
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    res, gates = {}, {}
    for x6 in (True, False):
        m = _model(dev, row, T, gray, P=P, impl=impl, pair=pair, x6=x6)
        res[x6] = _stepper(dev, m, B, T, 1 if gray else 3, P)()
        gates[x6] = device_gates(m, m.flat.detach(), B, T)
    assert set(gates[True]) == set(gates[False]) and len(gates[True]) >= 3
    differ = {k: int((gates[True][k] != gates[False][k]).sum()) for k in gates[True] if (gates[True][k] != gates[False][k]).any()}
    assert not differ, "ReLU gates differ between the x6 and the fp32 route for this seed (choose another fixed seed; the bars stay): %s" % differ
    on, off = res[True], res[False]
    e_pred = float((on[0] - off[0]).abs().max() / off[0].abs().max())
    worst = (0.0, None)
    for name, key, a, b in cv._tensors(m):
        e = float((on[2][a:b] - off[2][a:b]).abs().max() / (off[2][a:b].abs().max() + 1e-30))
        if e > worst[0]:
            worst = (e, name + "/" + key)
    print("gemm x6 %s impl %d pair %d against the fp32 route: prediction %.3g of its max norm; worst gradient tensor %.3g of its max norm (%s)"
          % (_id(case), impl, pair, e_pred, worst[0], worst[1]))
    assert not torch.equal(on[0], off[0]), "the switch changed nothing: the x6 kernels did not run"
    assert e_pred < 2e-6, e_pred
    assert worst[0] < 1e-5, worst


# ---- 4. switch handling -----------------------------------------------------------------------------------------------------------------------------
def test_toggling_the_switch_between_two_steps(dev):
    row = (64, 1, 8, 0.8, 51)
    always_on = _stepper(dev, _model(dev, row, impl=1))()
    always_off = _stepper(dev, _model(dev, row, impl=1, x6=False))()
    assert not _same(always_on, always_off)
    m = _model(dev, row, impl=1, x6=False)
    step = _stepper(dev, m)
    assert _same(step(), always_off)
    m.set_gemm_x6(True)
    assert _arith(m) == 1 and _same(step(), always_on)
    m.set_gemm_x6(False)
    assert _arith(m) == 0 and _same(step(), always_off)
    m.set_gemm_x6(True)
    assert _same(step(), always_on)
    m.set_impl(4)                                                   # set_impl keeps the wish ...
    assert m.gemm_x6 is True and _arith(m) == 1
    m.set_gemm_pair(True)                                           # ... so does the pair's switch ...
    assert m.gemm_x6 is True and _arith(m) == 1 and _kind(m) == 2
    m.set_gemm_route(False)                                         # ... and the route's, which decides whether the wish takes effect
    assert m.gemm_x6 is True and _arith(m) == 0
    m.set_gemm_route(True)
    m.set_impl(0)                                                   # family 0 never sees the switch
    assert m.gemm_x6 is True and _arith(m) == 0


def test_a_flip_between_forward_and_backward_is_refused(dev):
    from probav_amd import synth
    L, lib = _L(), _L().lib()
    B = 2
    m = _model(dev, (20, 1, 3, 0.5, 10), impl=1)
    h = m._handle()
    x = torch.as_tensor(synth.synth_batch(B, seed=3)[0]).to(dev)
    dy = torch.ones(B * 48 * 48, device=dev)
    y = torch.empty(B * 48 * 48, device=dev)
    flat = m.flat.detach()
    nbytes = lib.probav_workspace_bytes(h, B, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)         # (the switch moves no size)
    for first in (1, 0):
        assert lib.probav_engine_set_gemm_x6(h, first) == 0 and lib.probav_engine_gemm_arith(h) == first and lib.probav_workspace_bytes(h, B, 1) == nbytes
        L.check(lib.probav_forward(h, L.ptr(flat), L.ptr(x), L.ptr(y), L.ptr(ws), ws.numel(), B, 1, L.current_stream()), "probav_forward")
        assert lib.probav_engine_set_gemm_x6(h, 1 - first) == 0
        grads = torch.full((flat.numel(),), 7.0, device=dev)
        rc = lib.probav_backward(h, L.ptr(flat), L.ptr(dy), L.ptr(grads), L.ptr(ws), ws.numel(), B, L.current_stream())
        torch.cuda.synchronize()
        assert rc == L.PROBAV_EINVAL and bool((grads == 7.0).all()), (first, rc)
        assert lib.probav_engine_set_gemm_x6(h, first) == 0         # flipped back: the backward of that forward runs
        L.check(lib.probav_backward(h, L.ptr(flat), L.ptr(dy), L.ptr(grads), L.ptr(ws), ws.numel(), B, L.current_stream()), "probav_backward")
        torch.cuda.synchronize()
        assert torch.isfinite(grads).all() and not bool((grads == 7.0).any())


# ---- 5. guard bands ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ROWS[3], ROWS[0]], ids=[_id(ROWS[3]), _id(ROWS[0])])
def test_bands_of_a_training_step_in_x6(dev, case):
    """probav_forward(training = 1) + probav_backward_split in the arena of tests/bands.py: 0xFF / 0x00 fills of outputs and scratch, equal outputs, untouched
    bands and inputs, and the run on the late stream -- the x6 kernel writes inside its output only, and on the stream it was given."""
    from probav_amd import synth
    row, T, gray, B, P = case
    L, lib = _L(), _L().lib()
    m = _model(dev, row, T, gray, P=P, impl=4)
    h = m._handle()
    Pp, S = L.ptr, L.current_stream
    flat = m.flat.detach().cpu().numpy().copy()
    x = np.ascontiguousarray(synth.synth_batch(B, seed=3, numImgLR=T, patchSizeLR=P)[0], dtype=np.float32)
    out = 3 * P
    dy = np.random.default_rng(4).standard_normal((B, out, out, 1)).astype(np.float32)
    saved, scr = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.probav_workspace_split(h, B, ctypes.byref(saved), ctypes.byref(scr)) == 0
    saved, scr = saved.value, scr.value
    bufs = [bands.inp("params", flat), bands.inp("x", x), bands.inp("dy", dy), bands.out("y", F32, B * out * out, lead_count=out * out),
            bands.out("grads", F32, flat.size), bands.scratch("saved", saved), bands.scratch("scratch", scr)]

    def step(t):
        rc = lib.probav_forward(h, Pp(t["params"]), Pp(t["x"]), Pp(t["y"]), Pp(t["saved"]), saved, B, 1, S())
        return rc or lib.probav_backward_split(h, Pp(t["params"]), Pp(t["dy"]), Pp(t["grads"]), Pp(t["saved"]), saved, Pp(t["scratch"]), scr, B, None, 0, S())
    assert lib.probav_engine_gemm_arith(h) == 1
    rep = bands.check(bufs, step, dev)
    assert torch.isfinite(rep.outputs["grads"].view(F32)).all()
    bands.check_refusal(bufs, lambda t: lib.probav_backward_split(h, Pp(t["params"]), Pp(t["dy"]), Pp(t["grads"]), Pp(t["saved"]), saved, Pp(t["scratch"]), scr - 1, B, None, 0, S()),
                        dev, L.PROBAV_ENOSPACE)


# ---- 6. non-finite values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 4])
def test_non_finite_values_in_x6(dev, impl):
    """In the forms of tests/nonfinite_cases.py (values, the poisoned sample, the pixels): a NaN or an inf LR pixel of sample 1 reaches the loss and the gradient;
    its clean batch mates' predictions are the clean batch's bit for bit, and so is their share of the gradient -- the step with the upstream gradient of the
    poisoned sample's mates alone cannot be formed without that sample's NaN (0 x NaN), so the share is taken where it is one: the clean mates alone as a batch.
    A non-finite upstream gradient leaves the prediction alone and reaches the filter gradient of every layer behind an x6 backward-data launch.  (Which TAPS it
    reaches is the contract of the backward-filter kernel, which the switch leaves to the fp32 route: tests/test_gpu_gemm_route.py asserts it tap by tap on that
    kernel.  What the x6 kernel itself owes -- exactly the windows that read an element -- is asserted element by element in the two tests below.)"""
    from probav_amd import synth
    from tests import nonfinite_cases as nc
    row, T, gray, _, _ = ROWS[0]
    B = nc.BATCH
    m = _model(dev, row, T, gray, impl=impl)
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=nc.BATCH_SEED))
    dy = torch.as_tensor(nc.upstream()).to(dev)

    def step(xx, up):
        m.flat.grad = None
        p = m(xx, training=True)
        p.backward(up)
        return p.detach().clone(), m.flat.grad.detach().clone()
    clean = step(x, dy)
    assert _arith(m) == 1 and torch.isfinite(clean[0]).all() and torch.isfinite(clean[1]).all()
    mates = [s for s in range(B) if s != nc.POISONED]
    alone = step(x[mates].contiguous(), dy[mates].contiguous())
    assert torch.equal(alone[0], clean[0][mates])
    for valname, value in nc.VALUES:
        xp = x.clone()
        xp[nc.PIXEL] = value
        pred, grad = step(xp, dy)
        assert torch.equal(pred[mates], clean[0][mates]), "%s: a clean sample changed beside a poisoned one" % valname
        assert not torch.isfinite(pred[nc.POISONED]).all() and not torch.isfinite(grad).all(), valname
        again = step(xp[mates].contiguous(), dy[mates].contiguous())           # the mates' share of the gradient: theirs alone, bit for bit the clean batch's
        assert _same((again[0], 0, again[1]), (alone[0], 0, alone[1])), valname
        if valname != "-inf":
            up = dy.clone()
            up[nc.DY_PIXEL] = value
            pred, grad = step(x, up)
            assert torch.equal(pred, clean[0]) and not torch.isfinite(grad).all(), valname
            for name in ["normConv_0", "normConv_1", "convReducer_1", "expConv_0", "decConv_1"]:      # ... through every route launch of the reverse pass
                Lh = next(l for l in m.layers if l.name == name)
                assert not torch.isfinite(grad[Lh.v_off: Lh.b_off]).all(), (valname, name)
    assert _same((lambda r: (r[0], 0, r[1]))(step(x, dy)), (clean[0], 0, clean[1]))


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_pixel_reaches_exactly_its_windows_in_the_x6_kernel(dev, value):
    """The route's contract for its convolution ('Non-finite values': exactly the outputs whose windows read the element, all Cout of them; every
    other element keeps the clean run's bits; a tap on the zero padding is multiplied by zero pieces and poisons nothing), on the x6 kernel where one element can be
    presented to it: with three input channels mainConv1 (3 -> 64, 3x3x3, zero pads of 1) is a launch of the route, its input is the network's, and its output is
    the saved ACT 0.  One LR pixel at the sample's first voxel (windows clipped by the pads on all three axes), its last, and an interior one."""
    from probav_amd import synth
    row, T, gray, B, P = ROWS[5]
    F, hin = row[0], P + 6
    x = torch.as_tensor(synth.synth_batch(B, seed=12, numImgLR=T, inChannels=3)[0]).to(dev)

    def act0(m, xx):
        m(xx, training=True)
        return _view(m, B, 0, 0).clone().view(B, hin, hin, T, F)
    m = _model(dev, row, T, gray, impl=4)
    clean = act0(m, x)
    assert _arith(m) == 1 and torch.isfinite(clean).all()
    m.set_gemm_x6(False)
    assert not torch.equal(act0(m, x), clean), "mainConv1 of three channels is not a launch of the x6 route: the test has nothing to say"
    m.set_gemm_x6(True)
    for n, h, w, t, c in ((1, 0, 0, 0, 0), (1, hin - 1, hin - 1, T - 1, 2), (1, 5, 11, 6, 1), (0, 0, hin - 1, 3, 1)):
        xp = x.clone()
        xp[n, h, w, t, c] = value
        y = act0(m, xp)
        want = np.zeros((B, hin, hin, T), bool)
        want[n, max(h - 1, 0):h + 2, max(w - 1, 0):w + 2, max(t - 1, 0):t + 2] = True
        bad = ~torch.isfinite(y).cpu().numpy()
        assert (bad == want[..., None]).all(), "non-finite outputs: %d, windows that read the value: %d x %d" % (bad.sum(), want.sum(), F)
        keep = torch.as_tensor(~want, device=dev)
        assert torch.equal(y[keep], clean[keep]), "an element outside the windows changed"


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_activation_reaches_exactly_its_voxel_in_the_x6_pointwise_launch(dev, value):
    """The same contract on a 1x1x1 launch (the NT = 4 instance: 72 -> 144): probav_debug_hidden runs the route's expConv launch on the saved block input, which is
    the caller's buffer -- one element of it poisoned gives that voxel's hidden row, all of it, and leaves every other row's bits."""
    row, T, gray, B, P = ROWS[6]
    F, H, hin = row[0], row[0] * row[2], P + 6
    m = _model(dev, row, T, gray, P=P, impl=4)
    _stepper(dev, m, B, T, 1, P)()
    L = _L()
    flat, ws = m.flat.detach(), m._workspace(B, True)
    nvox = B * hin * hin * T
    scr = torch.empty(nvox * row[4], device=dev)

    def hidden():
        hid = torch.full((nvox * H,), float("nan"), device=dev)
        L.check(L.lib().probav_debug_hidden(m._handle(), L.ptr(flat), L.ptr(ws), ws.numel() * 4, B, 0, L.ptr(hid), L.ptr(scr), L.ptr(m.weight_cache()), L.current_stream()),
                "probav_debug_hidden")
        return hid.view(nvox, H)
    clean = hidden()
    assert _arith(m) == 1 and _kind(m) == 0 and torch.isfinite(clean).all()
    act = _view(m, B, 0, 0)                                         # (a view of the workspace: written through)
    for v, c in ((0, 0), (nvox - 1, F - 1), (nvox // 2 + 5, 17), (127, 64), (128, 71)):      # first, last, interior; the two sides of an M tile's edge, the K tail
        keep = act[v * F + c].clone()
        act[v * F + c] = value
        try:
            hid = hidden()
        finally:
            act[v * F + c] = keep
        bad = ~torch.isfinite(hid)
        assert bool(bad[v].all()) and int(bad.sum()) == H, (v, c, int(bad.sum()))
        rest = torch.ones(nvox, dtype=torch.bool, device=dev)
        rest[v] = False
        assert torch.equal(hid[rest], clean[rest]), "a row beside the poisoned voxel changed"
    assert torch.equal(hidden(), clean)


def test_a_non_finite_pixel_reaches_the_loss_in_x6(dev):
    from probav_amd import synth
    from probav_amd.loss import Losses
    from tests import nonfinite_cases as nc
    row, T, gray, _, _ = ROWS[3]
    m = _model(dev, row, T, gray, impl=4)
    lo = Losses(targetShape=(48, 48, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(nc.BATCH, seed=nc.BATCH_SEED))
    for valname, value in nc.VALUES[:2]:
        xp = x.clone()
        xp[nc.PIXEL] = value
        m.flat.grad = None
        p = m(xp, training=True)
        l = lo.shiftCompensatedL1Loss(hr, mask, p)
        l.backward()
        assert _arith(m) == 1 and not np.isfinite(float(l)) and not torch.isfinite(m.flat.grad).all(), valname


# ---- 7. the CLIs ------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_then_test_py_with_the_flags(dev, tmp_path):
    """The harness of tests/test_gpu_gemm_route.py::test_train_py_then_test_py_with_the_flag: train.py --gemm-route --gemm-x6 runs two steps and resumes from a
    checkpoint written without the flags; test.py --gemm-route --gemm-x6 reads that checkpoint and its PNGs are within one grey level of test.py --gemm-route's."""
    from probav_amd import synth
    from probav_amd.pngio import imread_uint16
    from tests.test_gpu_cli import CFG, _run
    d = str(tmp_path)
    aug, res = os.path.join(d, "pre", "augmentedPatchesDir"), os.path.join(d, "pre", "resolverDir")
    os.makedirs(aug), os.makedirs(res)
    x, hr, mask = synth.synth_batch(4, seed=5)
    for tag, k in (("TRAIN", 4), ("TRAINVAL", 2)):
        np.ma.masked_array(x[:k], mask=np.zeros(x[:k].shape, bool)).dump(os.path.join(aug, "%spatchesLR_NIR.npy" % tag))
        np.ma.masked_array(hr[:k], mask=~mask[:k].astype(bool)).dump(os.path.join(aug, "%spatchesHR_NIR.npy" % tag))
    sets = 2
    test_patches = synth.synth_batch(sets * 64, seed=6)[0].reshape(sets, 64, 22, 22, 9, 1)
    np.ma.masked_array(test_patches.transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((sets, 64, 9, 1, 22, 22), bool)).dump(os.path.join(res, "TESTpatchesLR_NIR.npy"))
    cfg = os.path.join(d, "f64.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d).replace("num_filters=32", "num_filters=64").replace("num_res_blocks=12", "num_res_blocks=2").replace("batch_size=1", "batch_size=2"))
    lib = _L().lib()
    h = make_engine(lib, 64, 2, 8, 51, 9)
    assert lib.probav_engine_set_gemm_route(h, 1) == 0 and lib.probav_engine_set_gemm_x6(h, 1) == 0 and lib.probav_engine_gemm_arith(h) == 1      # what the flags set
    lib.probav_engine_destroy(h)
    flags = ["--gemm-route", "--gemm-x6"]
    out = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
    assert "[ EPOCH 0/1 ] - [ STEP " in out.stderr and "/2 ]" in out.stderr, out.stderr[-2000:]          # two steps of batch 2
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.trainClass import ModelTrainer
    ck = os.path.join(d, "modelInfo", "ckpt_f64", "NIR")
    m = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, 64, (3, 3, 3), 2, 8, 0.8, 9, 16, True, seed=3).to(dev)
    assert m.gemm_x6 is False and ModelTrainer(m, None, None, None, ck, os.path.join(d, "lg")).save() == "ckpt-1.pt"      # a checkpoint written without the flags
    images = []
    for fl in (flags, ["--gemm-route"]):
        for p in glob.glob(os.path.join(d, "testout_f64", "*.png")):
            os.remove(p)
        _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR"] + fl, cwd=d)
        pngs = sorted(glob.glob(os.path.join(d, "testout_f64", "*.png")))
        assert len(pngs) == sets, pngs
        images.append([imread_uint16(p).astype(np.int64) for p in pngs])
    for a, b in zip(*images):
        assert np.abs(a - b).max() <= 1
    out2 = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
    assert "Model restored from checkpoint at step 0" in out2.stdout
