"""Every row of tests/plan_cases.py on the device, against the fp64 oracle: the launch plans a batch of 128 (and 24, 32, 43, 64, 256, 257) takes, kernel by kernel.

tests/test_plan_cases_host.py proves on the host that each row reaches the plan class it names; here the row runs through probav_conv3d_forward /
probav_conv3d_wgrad / probav_pw_forward / probav_pw_backward on the impls it names, and once on the cross-check (impl 0, the direct kernels; the pointwise pair has
none and takes impl 2, the fp32-MFMA pair).  Outputs are filled with NaN before the call; a repeated call must give the same bits.

Bars (the suite's own, none fitted):
  forward and backward-data   2e-6 of max |ref| per (sample, output channel) slice (tests/test_gpu_h3_range.py::_slice_err): one wrong strip in one of 128 samples fails
  filter gradient             1e-5 of max |ref| on dW and on db (tests/test_gpu_parity.py::test_conv3d_wgrad_matches_autograd)
  fused pointwise pair        2e-6 forward, 5e-6 on each of dx, dW1, db1, dW2, db2 (tests/test_gpu_parity.py::_fused_pointwise_case, with its decided_gates redraw)
Slices behind a ReLU.  ReLU is exact; what a kernel rounds is the pre-activation, a sum of 27 x Cin products.  With 256 x 32 slices some channel's bias sits three
standard deviations below zero for a sample: the slice keeps a handful of small positive values, and against THEIR maximum the rounding of the sum is not small -- the
unpadded reducer at N = 256 showed 7.4e-6 in conv3_pp_kernel and 2.4e-5 in the direct kernel on the same slices, with the whole tensor at 3.2e-7 and 9.4e-7.  A slice of
a layer with a ReLU is therefore judged against the largest |pre-activation| of the slice in the fp64 reference (tests/test_gpu_h3_range.py has no ReLU in its cases);
without a ReLU that is max |ref|, _slice_err itself.
The cross-check.  impl 0 sums the 27 x Cin products of an output in ONE fp32 accumulator, one after the other.  Over 128 x 32 slices of 10 000 values the worst slice
of such a sum sits above 2e-6 of its own maximum whoever evaluates it: on the mirrored-pad reducer at N = 128 the CPU gives 3.3e-6 (numpy fp32, taps and channels in
order) and 3.55e-6 (torch fp32 conv3d) against the fp64 reference, the direct kernel 3.55e-6; the whole tensor is at 1.0e-6 / 1.1e-6 / 1.1e-6.  The matrix kernels add
partial sums of 16 or 32 products and stay below 1.5e-6 per slice.  So impl 0 is held to the bar the suite already holds it to, 2e-6 of the WHOLE tensor's maximum
(tests/test_gpu_parity.py::test_conv3d_forward_matches_oracle) -- a wrong strip is an error of order one under either norm -- and its per-slice figure is printed.
References: fp64 F.conv3d / fp64 autograd on the CPU, fp64 numpy for the pair; one geometry's rows share inputs and oracle (the row at N is the first N samples).
At the hand-overs (tests/plan_cases.py::HANDOVERS) both sides are rows of their own, and on the samples they share the forward results of one kernel are equal bit for bit.

Worst measured figure per class of rows (MI355X; the per-case figures are printed):
  forward 25->32 + skip    cw4 1.04e-6 (N = 256 | 257; 9.7e-7 at the shipped plan, 9.6e-7 at SR 6 and 11, 7.8e-7 on three column ranges), pstrip 5.4e-7 (23-wide), strip (impl 2) 6.9e-7
  backward-data 32->25     cw4 1.25e-6 (shipped plan and N = 256; 1.08e-6 at SR 8 and 11, 8.8e-7 on three column ranges), pstrip 8.3e-7, pp 1.12e-6 (gated, depth 13, 3 and 4 ranges)
  reducers forward         pp 6.4e-7 per slice against the pre-activation (mirrored pads, unpadded, N = 128 ... 257)
  cross-check (impl 0)     whole tensor 1.09e-6 forward, 1.33e-6 backward-data
  filter gradient          wg4 dW 4.0e-7 db 3.0e-7 (every mode, SR 2 ... 22, column halves); general x6 kernel behind the hand-over dW 1.24e-6 (N = 257) db 4.9e-7; x6 (impl 3) 3.0e-7;
                           mfma (impl 1) 2.5e-7; direct 3.9e-7 -- all far inside 1e-5: no case needed the CPU fp32 evaluation
  pointwise pair           forward pf4 4.9e-7 (impl 2: 6.0e-7); reverse pw4 dx 2.7e-7, dW1 6.3e-7, dW2 3.5e-7, db2 2.1e-7, db1 7.3e-7 (2.9e-7 at the shipped 128 x 4 356; it was
                           5.41e-6 there, over the bar, until pw_bwd_w4_kernel alternated the sign of its product (b): test_pointwise_plan_backward_matches_oracle)
  hand-overs               the samples both sides share are the same bits on every impl whose report names one kernel for both sides
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import plan_cases as pc
from tests.test_gpu_h3_range import _slice_err

pytestmark = pytest.mark.gpu

FWD_BAR, WGRAD_BAR, PW_FWD_BAR, PW_BWD_BAR = 2e-6, 1e-5, 2e-6, 5e-6


def _L():
    from probav_amd import _lib as L
    return L


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)


# ---- the oracle: one geometry at a time ---------------------------------------------------------------------------------------------------------------
_oracle_cache = {}


def _group(row):
    key = pc.group_key(row)
    if _oracle_cache.get("key") != key:
        _oracle_cache.clear()
        _oracle_cache["key"] = key
    return _oracle_cache


def _padded(x, gate, pad, reflect):
    """The layer's input in fp64 as F.conv3d reads it ([N, C, H, W, T], gate applied, pads laid out: mirrored in rows / columns where the layer mirrors, zeros elsewhere)."""
    x = torch.as_tensor(x, dtype=torch.float64)
    if gate is not None:
        x = x * (torch.as_tensor(gate) > 0)
    x = x.permute(0, 4, 1, 2, 3)
    if reflect:
        x = torch.nn.functional.pad(x, (0, 0, pad[1], pad[1], pad[0], pad[0]), mode="reflect")
        return torch.nn.functional.pad(x, (pad[2], pad[2]))
    return torch.nn.functional.pad(x, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))


def _group_rows(row, op):
    return sorted((r for r in pc.CONV_ROWS if pc.group_key(r) == pc.group_key(row) and any(run[0] == op for run in r[10])), key=lambda r: r[1])


def _oracle_forward(row, op):
    """fp64 reference of the row's forward ('fwd': with the bias) or backward-data launch ('bwd': without), and the scale of every (sample, channel) slice: max |ref|, or
    max |pre-activation| where the layer has a ReLU (the module docstring, 'Slices behind a ReLU').  A sample's result does not depend on its batch: the rows of one
    geometry come in ascending N and each computes only the samples the rows before it have not."""
    cache = _group(row)
    big = _group_rows(row, op)[-1]
    name, N, hwt, Cin, Cout, pad, reflect, relu, gate, skip = big[:10]
    if op not in cache:
        cache[op] = dict(n=0, out=np.empty((N,) + pc.out_dims(hwt, pad) + (Cout,)), scale=np.empty((N, Cout)))
    st, d = cache[op], pc.inputs(big)
    w = torch.as_tensor(d["w"], dtype=torch.float64).permute(4, 3, 0, 1, 2)
    while st["n"] < row[1]:
        a, b = st["n"], min(row[1], st["n"] + 64)
        y = torch.nn.functional.conv3d(_padded(d["x"][a:b], None if d["gate"] is None else d["gate"][a:b], pad, reflect), w).permute(0, 2, 3, 4, 1)
        if op == "fwd":
            y = y + torch.as_tensor(d["bias"], dtype=torch.float64)
        pre = y
        if relu:
            y = torch.relu(y)
        if d["skip"] is not None:
            y = y + torch.as_tensor(d["skip"][a:b], dtype=torch.float64)
        st["out"][a:b] = y.numpy()
        st["scale"][a:b] = (pre if relu else y).abs().amax(dim=(1, 2, 3)).numpy()
        st["n"] = b
    return st["out"][:row[1]], st["scale"][:row[1]]


def _oracle_wgrad(row):
    """fp64 autograd of sum(conv(x, w) * dY [ygate > 0]) with respect to w, and sum(dY [ygate > 0]).  Both are sums over the samples: the rows of one geometry come in
    ascending N and each adds only the samples the rows before it have not."""
    cache = _group(row)
    big = _group_rows(row, "wgrad")[-1]
    name, N, hwt, Cin, Cout, pad, reflect, relu, gate, skip = big[:10]
    if "wgrad" not in cache:
        cache["wgrad"] = dict(n=0, dw=np.zeros(pc.K3 + (Cin, Cout)), db=np.zeros(Cout), at={})
    st, d = cache["wgrad"], pc.inputs(big)
    if row[1] < st["n"] and row[1] not in st["at"]:                  # (asked out of order: start over)
        st.update(n=0, dw=np.zeros_like(st["dw"]), db=np.zeros_like(st["db"]))
    while st["n"] < row[1]:
        a, b = st["n"], min(row[1], st["n"] + 64)
        wt = torch.zeros(pc.K3 + (Cin, Cout), dtype=torch.float64, requires_grad=True)
        yt = torch.nn.functional.conv3d(_padded(d["x"][a:b], None, pad, reflect), wt.permute(4, 3, 0, 1, 2)).permute(0, 2, 3, 4, 1)
        dyg = torch.as_tensor(d["dy"][a:b], dtype=torch.float64)
        if d["ygate"] is not None:
            dyg = dyg * (torch.as_tensor(d["ygate"][a:b]) > 0)
        (yt * dyg).sum().backward()
        st["dw"] += wt.grad.numpy()
        st["db"] += dyg.sum(dim=(0, 1, 2, 3)).numpy()
        st["n"] = b
    st["at"].setdefault(row[1], (st["dw"].copy(), st["db"].copy()))
    return st["at"][row[1]]


_dev_inputs = {}


def _device_inputs(row, dev):
    key = (pc.group_key(row), row[1])
    if key not in _dev_inputs:
        _dev_inputs.clear()
        _dev_inputs[key] = {k: _t(v, dev) for k, v in pc.inputs(row).items()}
    return _dev_inputs[key]


def _forward(row, op, impl, d):
    L = _L()
    name, N, hwt, Cin, Cout, pad, reflect, relu, gate, skip = row[:10]
    y = torch.full((N,) + pc.out_dims(hwt, pad) + (Cout,), float("nan"), device=d["x"].device)
    g = pc.geom(N, hwt, Cin, Cout, pad, reflect, relu)
    L.check(L.lib().probav_conv3d_forward(ctypes.byref(g), L.ptr(d["x"]), L.ptr(d["gate"]), L.ptr(d["w"]), L.ptr(d["bias"] if op == "fwd" else None), L.ptr(d["skip"]),
                                          L.ptr(y), impl, L.current_stream()), "probav_conv3d_forward")
    return y


def _wgrad(row, impl, d):
    L = _L()
    name, N, hwt, Cin, Cout, pad, reflect, relu, gate, skip = row[:10]
    g = pc.geom(N, hwt, Cin, Cout, pad, reflect, relu)
    nbytes = L.lib().probav_conv3d_wgrad_scratch_bytes(ctypes.byref(g), impl)
    assert nbytes > 0, "the backward-filter kernel of impl %d refuses the geometry" % impl
    dev = d["x"].device
    scratch = torch.empty(nbytes // 4 + 1, device=dev)
    dw, db = torch.full(pc.K3 + (Cin, Cout), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)
    L.check(L.lib().probav_conv3d_wgrad(ctypes.byref(g), L.ptr(d["x"]), L.ptr(d["dy"]), L.ptr(d["ygate"]), L.ptr(dw), L.ptr(db), L.ptr(scratch), nbytes, impl,
                                        L.current_stream()), "probav_conv3d_wgrad")
    return dw, db


CONV_TESTS = [(row, op) for row in pc.CONV_ROWS for op in ("fwd", "bwd", "wgrad") if any(run[0] == op for run in row[10])]


@pytest.mark.parametrize("row,op", CONV_TESTS, ids=["%s | %s" % (r[0], o) for r, o in CONV_TESTS])
def test_conv_plan_matches_oracle(dev, row, op):
    impls = [0] + sorted({run[1] for run in row[10] if run[0] == op})
    d = _device_inputs(row, dev)
    if op == "wgrad":
        ref_w, ref_b = _oracle_wgrad(row)
    else:
        ref, scale = _oracle_forward(row, op)
    failed = []
    for impl in impls:
        rep = pc.conv_report(row, op, impl)
        plan = "%s nsplit %d nstrips %d SR %d grid %d" % (rep["kernel"], rep["nsplit"], rep["nstrips"], rep["SR"], rep["grid"])
        if op == "wgrad":
            dw, db = _wgrad(row, impl, d)
            dw2, db2 = _wgrad(row, impl, d)
            e_w = np.abs(dw.cpu().double().numpy() - ref_w).max() / np.abs(ref_w).max()
            e_b = np.abs(db.cpu().double().numpy() - ref_b).max() / np.abs(ref_b).max()
            print("plan %s | wgrad impl %d (%s): dw err %.3g db err %.3g" % (row[0], impl, plan, e_w, e_b))
            assert torch.equal(dw, dw2) and torch.equal(db, db2), "a repeated call gives other bits (impl %d)" % impl
            if not (e_w < WGRAD_BAR and e_b < WGRAD_BAR):
                failed.append((impl, e_w, e_b))
        else:
            y = _forward(row, op, impl, d)
            y2 = _forward(row, op, impl, d)
            got = y.cpu().numpy()
            e = _slice_err(got, ref, (1, 2, 3)) if not row[7] else float((np.abs(got - ref).max(axis=(1, 2, 3)) / scale).max())
            e_all = float(np.abs(got - ref).max() / np.abs(ref).max())
            print("plan %s | %s impl %d (%s): worst (sample, channel) slice error %.3g, whole tensor %.3g" % (row[0], op, impl, plan, e, e_all))
            assert torch.equal(y, y2), "a repeated call gives other bits (impl %d)" % impl
            if not (e_all if impl == 0 else e) < FWD_BAR:             # (impl 0: the module docstring, 'The cross-check')
                failed.append((impl, e, e_all))
    assert not failed, (row[0], op, failed)


# ---- the fused pointwise pair -------------------------------------------------------------------------------------------------------------------------
def _pw_oracle(row):
    """fp64 numpy, in chunks of voxels (the hidden tensor of 128 x 4 356 voxels is 1.1 GB in fp64)."""
    x, w1, b1, w2, b2, ddec, dskip = pc.pw_inputs(row)
    W1, W2 = w1.astype(np.float64), w2.astype(np.float64)
    nvox, D = x.shape[0], w2.shape[1]
    dec, dx = np.empty((nvox, D)), np.empty((nvox, 32))
    dw1, db1, dw2, db2 = np.zeros((32, 256)), np.zeros(256), np.zeros((256, D)), np.zeros(D)
    for a in range(0, nvox, 1 << 16):
        X, DD = x[a:a + (1 << 16)].astype(np.float64), ddec[a:a + (1 << 16)].astype(np.float64)
        pre = X @ W1 + b1
        Hh = np.maximum(pre, 0)
        dec[a:a + len(X)] = Hh @ W2 + b2
        dH = (DD @ W2.T) * (pre > 0)
        dx[a:a + len(X)] = dskip[a:a + len(X)] + dH @ W1.T
        dw1 += X.T @ dH
        db1 += dH.sum(0)
        dw2 += Hh.T @ DD
        db2 += DD.sum(0)
    return dict(dec=dec, dx=dx, dw1=dw1, db1=db1, dw2=dw2, db2=db2)


def _pw_forward(row, impl, t):
    L = _L()
    nvox, D = t[0].shape[0], row[3]
    dec = torch.full((nvox, D), float("nan"), device=t[0].device)
    x, w1, b1, w2, b2 = t[:5]
    L.check(L.lib().probav_pw_forward(L.ptr(x), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(dec), nvox, row[2], D, impl, L.current_stream()), "probav_pw_forward")
    return dec


def _pw_backward(row, impl, t):
    L = _L()
    nvox, D, dev = t[0].shape[0], row[3], t[0].device
    x, w1, b1, w2, b2, ddec, dskip = t
    nbytes = L.lib().probav_pw_backward_scratch_bytes(D)
    scratch = torch.empty(nbytes // 4 + 1, device=dev)
    out = {k: torch.full(s, float("nan"), device=dev) for k, s in (("dx", (nvox, 32)), ("dw1", (32, 256)), ("db1", (256,)), ("dw2", (256, D)), ("db2", (D,)))}
    L.check(L.lib().probav_pw_backward(L.ptr(x), L.ptr(ddec), L.ptr(dskip), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(out["dx"]), L.ptr(out["dw1"]), L.ptr(out["db1"]),
                                       L.ptr(out["dw2"]), L.ptr(out["db2"]), L.ptr(scratch), nbytes, nvox, row[2], D, impl, L.current_stream()), "probav_pw_backward")
    return out


_pw_cache = {}


def _pw_case(row, dev):
    """The row's device results on the cross-check (impl 2) and on the impls it names, each call made twice, beside the oracle: shared by the row's tests, one row kept."""
    if row[0] not in _pw_cache:
        _pw_cache.clear()
        t = [_t(a, dev) for a in pc.pw_inputs(row)]
        res = {}
        for impl in [2] + sorted({run[1] for run in row[4]}):
            res[impl] = dict(dec=[_pw_forward(row, impl, t) for _ in range(2)], bwd=[_pw_backward(row, impl, t) for _ in range(2)])
        _pw_cache[row[0]] = (_pw_oracle(row), res)
    return _pw_cache[row[0]]


@pytest.mark.parametrize("row", pc.PW_ROWS, ids=[r[0] for r in pc.PW_ROWS])
def test_pointwise_plan_forward_matches_oracle(dev, row):
    ref, res = _pw_case(row, dev)
    failed = []
    for impl, r in res.items():
        assert torch.equal(r["dec"][0], r["dec"][1]), "a repeated forward call gives other bits (impl %d)" % impl
        e = np.abs(r["dec"][0].cpu().double().numpy() - ref["dec"]).max() / np.abs(ref["dec"]).max()
        print("plan %s | fwd impl %d (%s): max err / max |ref| = %.3g" % (row[0], impl, pc.pw_report(row, "fwd", impl)["kernel"], e))
        if not e < PW_FWD_BAR:
            failed.append((impl, e))
    assert not failed, (row[0], failed)


@pytest.mark.parametrize("what", ["dx", "dw1", "db1", "dw2", "db2"])
@pytest.mark.parametrize("row", pc.PW_ROWS, ids=[r[0] for r in pc.PW_ROWS])
def test_pointwise_plan_backward_matches_oracle(dev, row, what):
    """The case that forced a kernel fix: db1 of the shipped shape (128 samples of 4 356 voxels) read 5.41e-6 on impl 4 (pw_bwd_w4_kernel) against 2.19e-7 on impl 2, over
    the suite's 5e-6.  Cause, from the device's numbers: every output of the bf16 / fp16 MFMA pipe carries a one-sided error -- the mean signed error of the forward output is
    -1.4e-8 of mean |value| on impl 3 and 4 and -2e-10 on impl 2 (the fp32 MFMA), same inputs -- far below one fp32 rounding per element and invisible in any product that
    multiplies it by a value of either sign.  db1[h] = sum over ALL voxels of dH'[v, h] is the one plain sum of such outputs: the error of channel h was
    -1.3e-8 sum_v |dH'[v, h]| (correlation -0.87 over the 256 channels, every channel negative), which grows with the voxel count N while db1 grows with sqrt(N): 5.4e-7 of
    max |db1| at one sample, 1.5e-6 at 16, 2.3e-6 at 64, 5.4e-6 at 128.  pw_bwd_w4_kernel now runs product (b) of every other tile on the negated dT fragments and takes the
    sign back in the gate's multiply (csrc/kernels_pw4.hip, gate1): the one-sided term changes sign with the tile and db1 reads 2.9e-7 at this shape.  The general forms
    (pw_bwd_x6_kernel: impl 3, and impl 4 above 1 024 samples) still sum it plainly: 5.2e-6 on impl 3 at this shape, which no row names."""
    ref, res = _pw_case(row, dev)
    failed = []
    for impl, r in res.items():
        kb = pc.pw_report(row, "bwd", impl)
        assert torch.equal(r["bwd"][0][what], r["bwd"][1][what]), "a repeated backward call gives other bits (impl %d)" % impl
        e = np.abs(r["bwd"][0][what].cpu().double().numpy() - ref[what]).max() / np.abs(ref[what]).max()
        print("plan %s | bwd impl %d (%s, wps %d) %s: max err / max |ref| = %.3g" % (row[0], impl, kb["kernel"], kb["wps"], what, e))
        if not e < PW_BWD_BAR:
            failed.append((impl, e))
    assert not failed, (row[0], what, failed)


# ---- the hand-overs -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", pc.HANDOVERS, ids=[a for a, _ in pc.HANDOVERS])
def test_handover_sides_share_their_samples_bit_for_bit(dev, pair):
    """N and N + 1 samples: wherever the report names one kernel for both sides, the forward results of the N samples they share are the same bits (a sample's result
    does not depend on its batch mates, nor on which strip partition its batch takes)."""
    lo, hi = (pc.row_by_name(n) for n in pair)
    checked = 0
    if lo in pc.PW_ROWS:
        t_hi = [_t(a, dev) for a in pc.pw_inputs(hi)]
        n = lo[1] * lo[2]
        t_lo = [a[:n] if a.shape[0] == hi[1] * hi[2] else a for a in t_hi]
        for impl in (2, 3, 4):
            if pc.pw_report(lo, "fwd", impl)["kernel"] == pc.pw_report(hi, "fwd", impl)["kernel"]:
                assert torch.equal(_pw_forward(lo, impl, t_lo), _pw_forward(hi, impl, t_hi)[:n]), impl
                checked += 1
    else:
        d_hi = {k: _t(v, dev) for k, v in pc.inputs(hi).items()}
        d_lo = {k: (v[:lo[1]].contiguous() if v is not None and k not in ("w", "bias") else v) for k, v in d_hi.items()}
        for impl in (0, 1, 2, 3, 4):
            ka, kb = pc.conv_report(lo, "fwd", impl), pc.conv_report(hi, "fwd", impl)
            if ka["kernel"] == kb["kernel"] != "none":
                assert torch.equal(_forward(lo, "fwd", impl, d_lo), _forward(hi, "fwd", impl, d_hi)[:lo[1]]), (impl, ka, kb)
                checked += 1
    assert checked >= 3
