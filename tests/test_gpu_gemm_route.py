"""The general matrix route on the device (csrc/kernels_gemm.hip; include/probav_hip.h, 'the general matrix route').

Single operators -- probav_gemm_conv3d_forward on every row of test_gpu_parity.CONV_CASES the route takes, probav_gemm_conv3d_wgrad on every row of
WGRAD_CASES -- against that module's fp64 oracles with ITS bars (forward 2e-6 of max |ref|, dw and db 1e-5: the fp32-MFMA kernels of impl 1 meet them, and this
is the same arithmetic), plus the smallest shapes that reach the kernels' hazards: a K chunk's tail (Cin = 51, 43, 10, 9, 1), an N tile's tail (Cout = 51, 43,
9, 1), Cout beyond one N tile (512, 288), M tiles that straddle samples and end ragged, every pad mode at the border.  Then the bitwise properties, what a
non-finite input does ('Non-finite values'), the guard bands of tests/bands.py, and the whole network with the switch on:
tests/test_gpu_cfg_values.py's check, unchanged, with its bars."""
import ctypes
import glob
import os
import zlib

import numpy as np
import pytest
import torch

from tests import bands
from tests.test_gemm_route_host import make_engine
from tests.test_gpu_parity import CONV_CASES, WGRAD_CASES, _geom, _oracle_conv, _out_dims, _t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32

# name, N, (Hi, Wi, Ti), Cin, Cout, k, pad, reflect, relu, use_gate, use_skip: the hazard rows
EXTRA = [
    ("gemm: same 9->51, gate + skip, three samples in one M tile", 3, (7, 5, 3), 9, 51, (3, 3, 3), (1, 1, 1), 0, 0, 1, 1),
    ("gemm: 1x1x1 51->9", 2, (6, 5, 9), 51, 9, (1, 1, 1), (0, 0, 0), 0, 0, 0, 0),
    ("gemm: valid 1->1", 1, (5, 4, 3), 1, 1, (3, 3, 3), (0, 0, 0), 0, 0, 0, 0),
    ("gemm: full 10->43 gated (pads of 2)", 2, (4, 4, 3), 10, 43, (3, 3, 3), (2, 2, 2), 0, 0, 1, 0),
    ("gemm: mirrored pads 20->20 relu", 2, (6, 6, 3), 20, 20, (3, 3, 3), (1, 1, 0), 1, 1, 0, 0),
    ("gemm: 1x1x1 64->512, 315 voxels (no multiple of a tile)", 3, (7, 5, 3), 64, 512, (1, 1, 1), (0, 0, 0), 0, 1, 0, 0),
]


def _exotic_conv(c):
    k, pad, reflect = c[5], c[6], c[7]
    return max(pad) > 2 or (k != (1, 1, 1) and k[0] != 3) or (reflect and pad[0] > 1)


FWD_CASES = [c for c in CONV_CASES if not _exotic_conv(c)] + EXTRA
BWF_CASES = WGRAD_CASES + [c for c in EXTRA if max(c[6]) <= 1]


# entry point that takes a stream -> the test of this module that runs it in the arena, late stream included (tests/test_gpu_bands.py: STREAMED holds the other 50)
STREAMED = {"probav_gemm_conv3d_forward": "test_bands_forward_and_backward_data", "probav_gemm_conv3d_wgrad": "test_bands_backward_filter"}


def _L():
    from probav_amd import _lib as L
    return L


def _fwd_inputs(case, seed_off=0):
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip = case
    rng = np.random.default_rng(zlib.crc32(name.encode()) + seed_off)
    ho = _out_dims(hwt, k, pad, reflect)
    x = rng.normal(size=(N,) + hwt + (Cin,)).astype(np.float32)
    w = (rng.normal(size=k + (Cin, Cout)) / np.sqrt(np.prod(k) * Cin)).astype(np.float32)
    bias = rng.normal(size=Cout).astype(np.float32)
    gate = rng.normal(size=x.shape).astype(np.float32) if use_gate else None
    skip = rng.normal(size=(N,) + ho + (Cout,)).astype(np.float32) if use_skip else None
    return x, gate, w, bias, skip, ho


def _fwd(dev, case, x, gate, w, bias, skip, ho, n=None):
    """probav_gemm_conv3d_forward on the first n samples -> y (device tensor, NaN-filled before the call)."""
    name, N, hwt, Cin, Cout, k, pad, reflect, relu = case[:9]
    n = N if n is None else n
    g = _geom(n, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    L = _L()
    y = torch.full((n,) + ho + (Cout,), float("nan"), device=dev)
    args = [_t(a[:n] if i in (0, 1, 4) else a, dev) if a is not None else None for i, a in enumerate((x, gate, w, bias, skip))]
    L.check(L.lib().probav_gemm_conv3d_forward(ctypes.byref(g), *[L.ptr(a) for a in args], L.ptr(y), L.current_stream()), "probav_gemm_conv3d_forward")
    return y


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_matches_the_oracle(dev, case):
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip = case
    x, gate, w, bias, skip, ho = _fwd_inputs(case)
    y = _fwd(dev, case, x, gate, w, bias, skip, ho)
    ref = _oracle_conv(x, gate, w, bias, skip, pad, reflect, relu, ho)
    err = np.abs(y.cpu().double().numpy() - ref).max() / np.abs(ref).max()
    print("gemm forward %s: max err / max |ref| = %.3g" % (name, err))
    assert err < 2e-6, "%s: rel err %.3e" % (name, err)
    assert torch.equal(y, _fwd(dev, case, x, gate, w, bias, skip, ho)), "the same call twice gives other bits"
    if "bwd-data" in name or use_gate:
        # the engine's backward-data launch: the same call without a bias
        y0 = _fwd(dev, case, x, gate, w, None, skip, ho)
        ref0 = _oracle_conv(x, gate, w, None, skip, pad, reflect, relu, ho)
        err0 = np.abs(y0.cpu().double().numpy() - ref0).max() / np.abs(ref0).max()
        print("gemm backward-data form %s: max err / max |ref| = %.3g" % (name, err0))
        assert err0 < 2e-6, "%s (no bias): rel err %.3e" % (name, err0)


def _wgrad(dev, g, xd, dyd, gd, k, Cin, Cout):
    L = _L()
    nbytes = L.lib().probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(g))
    assert nbytes > 0
    scratch = torch.empty(nbytes // 4, device=dev)
    dw = torch.full(k + (Cin, Cout), float("nan"), device=dev)
    db = torch.full((Cout,), float("nan"), device=dev)
    L.check(L.lib().probav_gemm_conv3d_wgrad(ctypes.byref(g), L.ptr(xd), L.ptr(dyd), L.ptr(gd), L.ptr(dw), L.ptr(db), L.ptr(scratch), nbytes, L.current_stream()),
            "probav_gemm_conv3d_wgrad")
    return dw, db


@pytest.mark.parametrize("case", BWF_CASES, ids=[c[0] for c in BWF_CASES])
def test_backward_filter_matches_autograd(dev, case):
    """The inputs and the oracle of test_gpu_parity.py::test_conv3d_wgrad_matches_autograd."""
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, _, _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    ho = _out_dims(hwt, k, pad, reflect)
    x = rng.normal(size=(N,) + hwt + (Cin,)).astype(np.float32)
    dy = rng.normal(size=(N,) + ho + (Cout,)).astype(np.float32)
    gate = rng.normal(size=dy.shape).astype(np.float32) if relu else None
    if reflect:
        xp = torch.tensor(np.pad(x.astype(np.float64), [(0, 0), (pad[0],) * 2, (pad[1],) * 2, (0, 0), (0, 0)], mode="reflect"))
        xp = torch.nn.functional.pad(xp, (0, 0, pad[2], pad[2]))
    else:
        xp = torch.nn.functional.pad(torch.tensor(x, dtype=torch.float64), (0, 0, pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    wt = torch.zeros(k + (Cin, Cout), dtype=torch.float64, requires_grad=True)
    yt = torch.nn.functional.conv3d(xp.permute(0, 4, 1, 2, 3), wt.permute(4, 3, 0, 1, 2)).permute(0, 2, 3, 4, 1)
    dyg = torch.tensor(dy, dtype=torch.float64) * (torch.tensor(gate) > 0 if gate is not None else 1.0)
    (yt * dyg).sum().backward()
    g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    xd, dyd, gd = _t(x, dev), _t(dy, dev), (_t(gate, dev) if gate is not None else None)
    dw, db = _wgrad(dev, g, xd, dyd, gd, k, Cin, Cout)
    ref_w, ref_b = wt.grad.numpy(), dyg.sum(dim=(0, 1, 2, 3)).numpy()
    e_w = np.abs(dw.cpu().double().numpy() - ref_w).max() / np.abs(ref_w).max()
    e_b = np.abs(db.cpu().double().numpy() - ref_b).max() / np.abs(ref_b).max()
    print("gemm wgrad %s: dw err %.3g db err %.3g" % (name, e_w, e_b))
    assert e_w < 1e-5 and e_b < 1e-5, (e_w, e_b)
    dw2, db2 = _wgrad(dev, g, xd, dyd, gd, k, Cin, Cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "dw twice gives other bits"


def test_a_sample_does_not_depend_on_its_batch_mates(dev):
    """Sample 0 of an N = 3 call against the call with that sample alone, bit for bit: forward (three samples of 105 voxels in one 128-voxel tile) and the
    backward-data form (no bias, gated, pads of 2)."""
    fwd = EXTRA[0]
    bwd = ("gemm: full 10->43 gated, three samples", 3, (4, 4, 3), 10, 43, (3, 3, 3), (2, 2, 2), 0, 0, 1, 0)
    for case, with_bias in ((fwd, True), (bwd, False)):
        x, gate, w, bias, skip, ho = _fwd_inputs(case)
        b = bias if with_bias else None
        y3 = _fwd(dev, case, x, gate, w, b, skip, ho)
        y1 = _fwd(dev, case, x, gate, w, b, skip, ho, n=1)
        assert torch.isfinite(y3).all() and torch.equal(y3[:1], y1), case[0]


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_non_finite_input_reaches_its_windows_and_nothing_else(dev, value):
    """INTEGRATION.md, 'Non-finite values', the row of this operator: as the direct kernel on probav_conv3d_forward without a ReLU, a non-finite x makes every
    output whose window reads it non-finite -- and here exactly those: every other element, the poisoned sample's and its batch mates', keeps the clean run's
    bits.  Under a closed gate the value is selected away (x * [gate > 0] is a select): the clean run's bits everywhere."""
    case = ("gemm: same 9->51 + skip, non-finite", 3, (7, 5, 3), 9, 51, (3, 3, 3), (1, 1, 1), 0, 0, 0, 1)
    N, hwt, Cout = case[1], case[2], case[4]
    x, gate, w, bias, skip, ho = _fwd_inputs(case)
    clean = _fwd(dev, case, x, gate, w, bias, skip, ho)
    assert torch.isfinite(clean).all()
    for n, h, wc, t, ci in ((1, 0, 0, 0, 0), (1, 6, 4, 2, 8), (1, 3, 2, 1, 4), (2, 6, 4, 2, 8)):      # the sample's first voxel, its last, an interior one; the batch's last
        xp = x.copy()
        xp[n, h, wc, t, ci] = value
        y = _fwd(dev, case, xp, gate, w, bias, skip, ho)
        want = np.zeros((N,) + ho, bool)
        want[n, max(h - 1, 0):h + 2, max(wc - 1, 0):wc + 2, max(t - 1, 0):t + 2] = True
        bad = ~torch.isfinite(y).cpu().numpy()
        assert (bad == want[..., None]).all(), "non-finite outputs: %d, windows that read the value: %d x %d" % (bad.sum(), want.sum(), Cout)
        keep = torch.as_tensor(~want, device=dev)
        assert torch.equal(y[keep], clean[keep]), "an element outside the windows changed"
        # a closed gate over the poisoned element
        gt = np.ones_like(x)
        gt[n, h, wc, t, ci] = -1.0
        xz = x.copy()
        xz[n, h, wc, t, ci] = 0.0
        gated_case = case[:9] + (1, 1)
        assert torch.equal(_fwd(dev, gated_case, xp, gt, w, bias, skip, ho), _fwd(dev, gated_case, xz, gt, w, bias, skip, ho))


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_gradient_in_the_backward_filter(dev, value):
    """dY = NaN or inf under an open gate marks db[co] and the [ci] slices of dw[.., co] of the taps whose windows read a real input -- a tap on the zero padding is a zero in
    BOTH operands (the direct kernel skips it), so at a corner voxel the taps that fall outside stay finite; under a closed gate the value is selected away."""
    N, hwt, Cin, Cout, k, pad = 2, (5, 4, 3), 9, 20, (3, 3, 3), (1, 1, 1)
    rng = np.random.default_rng(77)
    x = rng.normal(size=(N,) + hwt + (Cin,)).astype(np.float32)
    dy = rng.normal(size=(N,) + hwt + (Cout,)).astype(np.float32)
    gate = np.ones_like(dy)
    g = _geom(N, *hwt, Cin, *hwt, Cout, k, pad, 0, 1)
    dw0, db0 = _wgrad(dev, g, _t(x, dev), _t(dy, dev), _t(gate, dev), k, Cin, Cout)
    assert torch.isfinite(dw0).all() and torch.isfinite(db0).all()
    dyp = dy.copy()
    dyp[1, 0, 0, 0, 7] = value                                    # the corner voxel: taps with a, b or c = 0 read the padding
    dw, db = _wgrad(dev, g, _t(x, dev), _t(dyp, dev), _t(gate, dev), k, Cin, Cout)
    want = np.zeros(k + (Cin, Cout), bool)
    want[1:, 1:, 1:, :, 7] = True
    bad = ~torch.isfinite(dw).cpu().numpy()
    assert (bad == want).all(), (bad.sum(), want.sum())
    assert (~torch.isfinite(db).cpu().numpy() == (np.arange(Cout) == 7)).all()
    keep = torch.as_tensor(~want, device=dev)
    assert torch.equal(dw[keep], dw0[keep])
    gate[1, 0, 0, 0, 7] = -1.0
    dyz = dy.copy()
    dyz[1, 0, 0, 0, 7] = 0.0
    a = _wgrad(dev, g, _t(x, dev), _t(dyp, dev), _t(gate, dev), k, Cin, Cout)
    b = _wgrad(dev, g, _t(x, dev), _t(dyz, dev), _t(gate, dev), k, Cin, Cout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all()


# ---- guard bands (tests/bands.py) -------------------------------------------------------------------------------------------------------------
def _P(t):
    return _L().ptr(t)


def _opt(name, a):
    return [] if a is None else [bands.inp(name, a)]


@pytest.mark.parametrize("case", [EXTRA[0], EXTRA[3], EXTRA[5]], ids=[EXTRA[0][0], EXTRA[3][0], EXTRA[5][0]])
def test_bands_forward_and_backward_data(dev, case):
    """probav_gemm_conv3d_forward with a bias and, as the engine launches backward-data, without one: nothing outside y is written, y does not depend on what it
    held.  A geometry the route refuses is refused with nothing written."""
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip = case
    x, gate, w, bias, skip, ho = _fwd_inputs(case)
    L, S = _L(), _L().current_stream
    per = int(np.prod(ho)) * Cout
    for b in (bias, None):
        g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
        bufs = [bands.inp("x", x)] + _opt("gate", gate) + [bands.inp("w", w)] + _opt("bias", b) + _opt("skip", skip) + [bands.out("y", F32, N * per, lead_count=per)]
        call = lambda t, g=g: L.lib().probav_gemm_conv3d_forward(ctypes.byref(g), _P(t["x"]), _P(t.get("gate")), _P(t["w"]), _P(t.get("bias")), _P(t.get("skip")),
                                                                   _P(t["y"]), S())
        bands.check(bufs, call, dev)
    # refused: a mirrored depth pad cannot be said through the ABI; pads of 3 can
    gx = _geom(N, hwt[0], hwt[1], hwt[2], Cin, hwt[0] + 4, hwt[1] + 4, hwt[2] + 4, Cout, (3, 3, 3), (3, 3, 3), 0, 0)
    perx = (hwt[0] + 4) * (hwt[1] + 4) * (hwt[2] + 4) * Cout
    wx = np.zeros((3, 3, 3, Cin, Cout), np.float32)
    bufs = [bands.inp("x", x), bands.inp("w", wx), bands.out("y", F32, N * perx, lead_count=perx)]
    bands.check_refusal(bufs, lambda t: L.lib().probav_gemm_conv3d_forward(ctypes.byref(gx), _P(t["x"]), None, _P(t["w"]), None, None, _P(t["y"]), S()), dev, L.PROBAV_EINVAL)


@pytest.mark.parametrize("case", [EXTRA[0], EXTRA[4], EXTRA[5]], ids=[EXTRA[0][0], EXTRA[4][0], EXTRA[5][0]])
def test_bands_backward_filter(dev, case):
    """probav_gemm_conv3d_wgrad: bands, fills, plain tensors; a scratch declared one byte short is refused as probav_conv3d_wgrad refuses it, nothing written."""
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, _, _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 2)
    ho = _out_dims(hwt, k, pad, reflect)
    x = rng.normal(size=(N,) + hwt + (Cin,)).astype(np.float32)
    dy = rng.normal(size=(N,) + ho + (Cout,)).astype(np.float32)
    gate = rng.normal(size=dy.shape).astype(np.float32) if relu else None
    g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    L, S = _L(), _L().current_stream
    nbytes = L.lib().probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(g))
    assert nbytes > 0
    bufs = [bands.inp("x", x), bands.inp("dy", dy)] + _opt("gate", gate) + [bands.out("dw", F32, int(np.prod(k)) * Cin * Cout), bands.out("db", F32, Cout),
                                                                            bands.scratch("scratch", nbytes)]
    call = lambda nb: (lambda t: L.lib().probav_gemm_conv3d_wgrad(ctypes.byref(g), _P(t["x"]), _P(t["dy"]), _P(t.get("gate")), _P(t["dw"]), _P(t["db"]),
                                                                   _P(t["scratch"]), nb, S()))
    bands.check(bufs, call(nbytes), dev)
    bands.check_refusal(bufs, call(nbytes - 1), dev, L.PROBAV_ENOSPACE)
    # pads of 2 are the backward-filter's exotic: refused, nothing written
    g2 = _geom(N, hwt[0], hwt[1], hwt[2], Cin, hwt[0] + 2, hwt[1] + 2, hwt[2] + 2, Cout, (3, 3, 3), (2, 2, 2), 0, 0)
    assert L.lib().probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(g2)) == 0
    bands.check_refusal(bufs, lambda t: L.lib().probav_gemm_conv3d_wgrad(ctypes.byref(g2), _P(t["x"]), _P(t["dy"]), None, _P(t["dw"]), _P(t["db"]), _P(t["scratch"]), nbytes, S()),
                        dev, L.PROBAV_EINVAL)


@pytest.fixture(scope="module", autouse=True)
def _release_the_arena(dev):
    yield
    bands.release(dev)


# ---- the whole network ---------------------------------------------------------------------------------------------------------------------------
# (row = (F, R, E, decay, D), T, gray, B): tests/cfg_grid.py's form
NET_CASES = [((64, 2, 8, 0.8, 51), 9, True, 3), ((48, 2, 6, 0.9, 43), 9, True, 2), ((32, 2, 8, 0.5, 16), 9, True, 2), ((32, 2, 8, 0.9, 28), 9, True, 2),
             ((20, 1, 3, 0.5, 10), 9, True, 2), ((64, 1, 8, 0.8, 51), 13, False, 2)]


def _route_counts(row, T, gray, B, impl, on):
    lib = _L().lib()
    F, R, E, decay, D = row
    h = make_engine(lib, F, R, E, D, T, 1 if gray else 3)
    try:
        assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, int(on)) == 0
        c = (ctypes.c_int32 * 4)()
        assert lib.probav_engine_route_counts(h, B, ctypes.byref(c)) == 0
        return tuple(c)
    finally:
        lib.probav_engine_destroy(h)


@pytest.mark.parametrize("impl", [1, 4])
@pytest.mark.parametrize("case", NET_CASES, ids=["f%d-r%d-e%d-d%d-t%d-b%d" % (c[0][0], c[0][1], c[0][2], c[0][4], c[1], c[3]) for c in NET_CASES])
def test_whole_network_on_the_route_matches_the_oracle(dev, case, impl, monkeypatch):
    """tests/test_gpu_cfg_values.py::_check_against_the_oracle, unchanged, on engines created with PROBAV_GEMM_ROUTE=1: output 2e-5, loss 1e-5, gradients 1e-3 at the
    device's gates (or GRAD_L2_TOL), and its bit-for-bit properties -- repeated step, training = inference, sample alone, side-stream mode."""
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B = case
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")                      # (that module's own autouse fixture: the gates are read from the pass's workspace)
    monkeypatch.setenv("PROBAV_GEMM_ROUTE", "1")
    off, on = _route_counts(row, T, gray, B, impl, False), _route_counts(row, T, gray, B, impl, True)
    print("route counts %s impl %d: off %s on %s" % (case, impl, off, on))
    # (decay 0.5 at 32 filters: the convolutions stay on the fp32 row-tile MFMA kernel and the fused pair, only normConv's backward-filter comes to the route)
    assert on[3] > 0 and on[0] == 0 and on[2] == 0 and (on[1] > 0 or row[0] == 32), "the route does not serve this step"
    assert off[1] == 0 and off[3] == 0 and off[0] == on[1] and off[2] == on[3]
    cv._check_against_the_oracle(dev, row, T, gray, B, impl, 16, "gemm-route f%d-r%d-e%d-d%d-t%d" % (row[0], row[1], row[2], row[4], T))


@pytest.mark.parametrize("impl", [1, 4])
@pytest.mark.parametrize("case", NET_CASES + [((32, 12, 8, 0.8, 25), 9, True, 2)],
                         ids=lambda c: "f%d-r%d-e%d-d%d-t%d" % (c[0][0], c[0][1], c[0][2], c[0][4], c[1]) if isinstance(c, tuple) else None)
def test_the_census_is_what_a_step_launches(dev, case, impl):
    """probav_engine_route_counts routes the engine's launch list; probav_engine_launched_counts counts where forward and backward actually launch, each launch
    fetched from that list.  After one training step the two agree, switch off and on -- at the cfg values above and the shipped network -- so a pass that
    skips a launch of the list, or issues one twice, fails here."""
    row, T, gray, B = case
    lib = _L().lib()
    m = _model(dev, row, T, gray)
    m.set_impl(impl)
    step = _stepper(dev, m, B, T, 1 if gray else 3)
    for on in (False, True):
        m.set_gemm_route(on)
        got, want = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
        assert lib.probav_engine_launched_counts(m._handle(), ctypes.byref(got), 1) == 0           # (clear)
        step()
        assert lib.probav_engine_launched_counts(m._handle(), ctypes.byref(got), 1) == 0
        assert lib.probav_engine_route_counts(m._handle(), B, ctypes.byref(want)) == 0
        print("census %s impl %d route %s: %s" % (case, impl, on, tuple(want)))
        assert tuple(got) == tuple(want), (on, tuple(got), tuple(want))
        assert lib.probav_engine_launched_counts(m._handle(), ctypes.byref(got), 0) == 0 and tuple(got) == (0, 0, 0, 0)      # the read cleared them


def _model(dev, row, T=9, gray=True, seed=11):
    from tests import test_gpu_cfg_values as cv
    return cv._build(dev, row, T, gray, seed)[0]


def _stepper(dev, m, B=2, T=9, C=1):
    from probav_amd import synth
    from probav_amd.loss import Losses
    lo = Losses(targetShape=(48, 48, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=12, numImgLR=T, inChannels=C))

    def step():
        m.flat.grad = None
        p = m(x, training=True)
        l = lo.shiftCompensatedL1Loss(hr, mask, p)
        l.backward()
        return p.detach().clone(), float(l), m.flat.grad.detach().clone()
    return step


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2])


def test_family_0_and_the_shipped_network_do_not_see_the_switch(dev):
    """Family 0 with the switch on is family 0; the shipped network at family 4 launches what it launched: prediction, loss and flat gradient bit for bit."""
    for row, impl in (((64, 1, 8, 0.8, 51), 0), ((32, 12, 8, 0.8, 25), 4)):
        m = _model(dev, row)
        m.set_impl(impl)
        step = _stepper(dev, m)
        assert m.gemm_route is False
        off = step()
        m.set_gemm_route(True)
        assert m.gemm_route is True
        assert _same(step(), off), (row, impl)


def test_toggling_the_switch_between_two_steps(dev):
    m = _model(dev, (64, 1, 8, 0.8, 51))
    m.set_impl(1)
    step = _stepper(dev, m)
    off = step()
    m.set_gemm_route(True)
    on = step()
    assert not _same(on, off)                                       # another order of additions
    assert (on[0] - off[0]).abs().max() < 2e-5 * off[0].abs().max() and abs(on[1] - off[1]) < 1e-5 * abs(off[1])
    m.set_gemm_route(False)
    assert _same(step(), off)
    m.set_gemm_route(True)
    assert _same(step(), on)
    m.set_impl(4)                                                   # set_impl keeps the switch
    assert m.gemm_route is True


def test_optimizer_steps_and_the_weight_cache_on_the_route(dev):
    """test_gpu_cfg_values.py::test_optimizer_step_and_weight_cache_at_other_cfg_values, part (3), with the route on: after two fused optimizer steps a pass from
    the weight cache equals the pass that recomputes the weights, bit for bit -- the route reads weff / weffT, cached or not."""
    from probav_amd.trainClass import make_optimizer
    m = _model(dev, (64, 1, 8, 0.8, 51), seed=4164)
    m.set_gemm_route(True)
    step = _stepper(dev, m)
    opt = make_optimizer("nadam", m, 5e-4)
    for k in range(2):
        assert (m.weight_cache() is not None) == (k > 0)
        step()
        opt.step()
    assert m.weight_cache() is not None
    cached = step()
    m._wcache_version = None
    assert m.weight_cache() is None
    assert _same(step(), cached)


# ---- the CLIs -----------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_then_test_py_with_the_flag(dev, tmp_path):
    """train.py --cfg <a 64-filter cfg> --gemm-route, two steps on synthetic dumps; a checkpoint of that network in the cfg's directory (the trainer saves every 1000
    steps: saved here, as tests/test_gpu_fusenet.py does); test.py --gemm-route writes the PNGs from it and train.py --gemm-route resumes from it.  The harness of
    tests/test_gpu_cli.py."""
    from probav_amd import synth
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
    out = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR", "--gemm-route"], cwd=d)
    assert "[ EPOCH 0/1 ] - [ STEP " in out.stderr and "/2 ]" in out.stderr, out.stderr[-2000:]          # two steps of batch 2
    from probav_amd import testClass
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.pngio import imread_uint16
    from probav_amd.trainClass import ModelTrainer
    ck = os.path.join(d, "modelInfo", "ckpt_f64", "NIR")
    m = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, 64, (3, 3, 3), 2, 8, 0.8, 9, 16, True, seed=3).to(dev)
    assert ModelTrainer(m, None, None, None, ck, os.path.join(d, "lg")).save() == "ckpt-1.pt"
    _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR", "--gemm-route"], cwd=d)
    pngs = sorted(glob.glob(os.path.join(d, "testout_f64", "*.png")))
    assert len(pngs) == sets, pngs
    # pixels: the same model with the switch on, through the reference-shaped host loop; the checkpoint does not know the route, and with the switch off the images
    # agree to the rounding of a prediction
    m.set_gemm_route(True)
    for p, w in zip(pngs, testClass.evaluate(m, test_patches, batch_size=16)):
        np.testing.assert_array_equal(imread_uint16(p), w[:, :, 0].astype(np.uint16))
    m.set_gemm_route(False)
    for p, w in zip(pngs, testClass.evaluate(m, test_patches, batch_size=16)):
        assert np.abs(imread_uint16(p).astype(np.int64) - w[:, :, 0].astype(np.int64)).max() <= 1
    out2 = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR", "--gemm-route"], cwd=d)
    assert "Model restored from checkpoint at step 0" in out2.stdout
