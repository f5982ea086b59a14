"""The non-finite contracts on the device ('Non-finite values'): what every exported operator and every kernel family does
with a NaN, a +inf or a -inf in each operand, and whether a training step that meets one shows it to the guard.

The cases, their inputs and their references live in tests/nonfinite_cases.py; tests/test_nonfinite_host.py proves on the host that every
reference is non-finite where its case says so.  Non-finite floats in a buffer are data: nothing here can fault a kernel.

What is asserted (contracts of the section):
  S  a sample whose own input is clean is bit for bit the clean launch's, whatever its batch mates hold           (every forward operator)
  .  convolutions, with or without a ReLU: every output element the reference has non-finite (NaN included) is non-finite on the device
  .  the fused pointwise pair: dec and dw2 lie behind the hidden tile's `fmaxf`, the documented exception contract P exists for -- an inf of x
     is kept by the fp32-MFMA family and asserted there; the finite results the section documents elsewhere are asserted as documented
  .  backward-filter (the detector): every [ci] slice of dw and entry of db the reference has non-finite is non-finite on the device; the
     shipped shapes must reach the default family's kernels (no skip)
  T  reference loss or gradient non-finite (fp32 oracle) => device loss non-finite or probav_grad_guard sets skip
  I  reference prediction of a sample non-finite => device prediction of that sample holds a non-finite element
Every test prints `NFTABLE ...` lines before it asserts: the per-operator table of the section is filled from them."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from probav_amd import synth
from tests import nonfinite_cases as nc

pytestmark = pytest.mark.gpu

IMPLS = [0, 1, 2, 3, 4]
NAN32 = float("nan")


def _L():
    from probav_amd import _lib
    return _lib


def _t(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _tsame(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _bad(a):
    return ~np.isfinite(a)


def _row(*fields):
    print("NFTABLE " + " | ".join(str(f) for f in fields))


# ---- 3a. probav_conv3d_forward ----------------------------------------------------------------------------------------------------------------
def _conv_launch(dev, name, d, impl):
    from tests.test_gpu_parity import _geom
    L = _L()
    _, N, hwt, Cin, Cout, k, pad, reflect, relu = nc.conv_case(name)[:9]
    ho = d["ho"]
    g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    y = torch.full((N,) + tuple(ho) + (Cout,), 12345.0, device=dev)                     # (finite fill: an element nobody wrote must not pass for a NaN)
    args = [_t(d[key], dev) for key in ("x", "gate", "w", "bias", "skip")]
    rc = L.lib().probav_conv3d_forward(ctypes.byref(g), *[L.ptr(a) for a in args], L.ptr(y), impl, L.current_stream())
    return rc, y.cpu().numpy()


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", nc.CONV_NAMES)
def test_conv3d_forward_nonfinite(dev, name, impl):
    L = _L()
    c = nc.conv_case(name)
    relu = c[8]
    rc, clean = _conv_launch(dev, name, nc.conv_inputs(name), impl)
    if impl >= 1 and rc == L.PROBAV_EINVAL:
        assert not (impl == 4 and name in nc.CONV_ON_IMPL4), "a shipped-layer shape must run on the default family: the routing emptied this test"
        pytest.skip("geometry not covered by this MFMA kernel (the engine falls back)")
    L.check(rc, "probav_conv3d_forward")
    assert np.isfinite(clean).all()
    failures = []
    for operand in nc.conv_operands(name):
        whole = operand in ("w", "bias")
        positions = [p for p, _ in nc.conv_positions(c[2])] if not whole else [None]
        for valname, value in nc.VALUES:
            marked = needed = nan_ref = nan_kept = 0
            for posname in positions:
                rc, y = _conv_launch(dev, name, nc.conv_poisoned(name, operand, posname, value), impl)
                assert rc == 0, (operand, posname, valname, rc)                                                   # 1. the return code
                if not whole:                                                                                     # 2. contract S
                    for n in range(y.shape[0]):
                        if n != nc.POISONED and not _same(y[n], clean[n]):
                            failures.append("S: sample %d changed with %s in %s at %s of sample %d" % (n, valname, operand, posname, nc.POISONED))
                ref = nc.conv_reference(name, operand, posname, valname)
                got = y if whole else y[nc.POISONED:nc.POISONED + 1]
                need = _bad(ref)                    # 3. / 4.: +inf, -inf AND NaN, behind a ReLU too: every output epilogue lets NaN through
                miss = need & np.isfinite(got)
                needed += int(need.sum())
                marked += int((need & _bad(got)).sum())
                nan_ref += int(np.isnan(ref).sum())
                nan_kept += int((np.isnan(ref) & _bad(got)).sum())
                if miss.any():
                    failures.append("%s in %s at %s: %d of %d required elements are finite on the device" % (valname, operand, posname, int(miss.sum()), int(need.sum())))
            _row("conv3d_forward", name, "impl %d" % impl, "relu" if relu else "plain", operand, valname,
                 "required non-finite %d, device %d" % (needed, marked), "reference NaN %d, device non-finite there %d" % (nan_ref, nan_kept))
    assert not failures, failures


# ---- 3a. the fused pointwise pair ---------------------------------------------------------------------------------------------------------------
def _pw_run(dev, d, nvox, vps, impl, backward=True):
    L = _L()
    D = d["w2"].shape[1]
    t = {k: _t(d[k], dev) for k in ("x", "w1", "b1", "w2", "b2", "ddec", "dskip")}
    out = {"dec": torch.full((nvox, D), 12345.0, device=dev)}
    L.check(L.lib().probav_pw_forward(L.ptr(t["x"]), L.ptr(t["w1"]), L.ptr(t["b1"]), L.ptr(t["w2"]), L.ptr(t["b2"]), L.ptr(out["dec"]), nvox, vps, D, impl,
                                      L.current_stream()), "probav_pw_forward")
    if backward:
        nbytes = L.lib().probav_pw_backward_scratch_bytes(D)
        scratch = torch.empty(nbytes // 4 + 1, device=dev)
        for key, shape in (("dx", (nvox, 32)), ("dw1", (32, 256)), ("db1", (256,)), ("dw2", (256, D)), ("db2", (D,))):
            out[key] = torch.full(shape, 12345.0, device=dev)
        L.check(L.lib().probav_pw_backward(L.ptr(t["x"]), L.ptr(t["ddec"]), L.ptr(t["dskip"]), L.ptr(t["w1"]), L.ptr(t["b1"]), L.ptr(t["w2"]), L.ptr(out["dx"]),
                                           L.ptr(out["dw1"]), L.ptr(out["db1"]), L.ptr(out["dw2"]), L.ptr(out["db2"]), L.ptr(scratch), nbytes, nvox, vps, D, impl,
                                           L.current_stream()), "probav_pw_backward")
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("impl", [2, 3, 4])
@pytest.mark.parametrize("nvox,vps", nc.PW_SHAPES)
def test_pointwise_pair_nonfinite(dev, nvox, vps, impl):
    clean = _pw_run(dev, nc.pw_inputs(nvox), nvox, vps, impl)
    assert all(np.isfinite(a).all() for a in clean.values())
    others = np.ones(nvox, bool)
    others[nc.POISONED * vps:(nc.POISONED + 1) * vps] = False
    failures = []
    for valname, _ in nc.VALUES:
        for zero_dy in (False, True):
            tally = {k: [0, 0] for k in ("dec", "dw1", "db1", "dw2", "db2")}
            for posname, _v in nc.pw_positions(vps):
                got = _pw_run(dev, nc.pw_poisoned(nvox, vps, posname, valname, zero_dy), nvox, vps, impl)
                ref = nc.pw_reference(nvox, vps, posname, valname, zero_dy)
                for key in ("dec", "dx"):                                                                         # contract S, forward and reverse
                    if not _same(got[key][others], clean[key][others]):
                        failures.append("S: %s of a clean sample changed (%s at %s, zero_dy %s)" % (key, valname, posname, zero_dy))
                # dec and dw2 lie behind the hidden tile's ReLU, which is `fmaxf` (the documented exception).  What the table says is
                # held, both ways, so that a change of either side has to change the other:
                #   an inf of x on the fp32-MFMA family (impl 2): hidden values of +-inf, no NaN enters the ReLU -> everything the reference marks is marked
                #   a NaN of x (every family), an inf of x on the split families (impl 3, 4: its pieces are (inf, NaN)): the hidden ReLU drops the NaN
                #   -> dec and dw2 are finite where the reference is not.  x itself goes on over the block's skip connection, and dw1 sees it.
                kept = valname != "nan" and impl == 2
                for key in ("dec", "dw2"):
                    rb, gb = _bad(ref[key]), _bad(got[key])
                    if kept and (rb & ~gb).any():
                        failures.append("%s: %s at %s: %d elements the reference has non-finite are finite on the device" % (key, valname, posname, int((rb & ~gb).sum())))
                    if not kept and gb.any():
                        failures.append("%s: %s at %s: %d non-finite elements where INTEGRATION.md documents a finite result" % (key, valname, posname, int(gb.sum())))
                assert np.isfinite(ref["dx"]).all()
                # the detector: dw1 = x^T dH holds x's channel times dH -- inf * dH, and inf * 0 = NaN where the gate or d_dec is zero: the whole row of
                # that channel, in every family, for every value, d_dec random or zero; db1 and db2 never see x
                for key in ("dw1", "db1", "db2"):
                    rb, gb = _bad(ref[key]), _bad(got[key])
                    if (rb & ~gb).any():
                        failures.append("detector %s: %s at %s, zero_dy %s: %d of the reference's %d non-finite entries are finite on the device"
                                        % (key, valname, posname, zero_dy, int((rb & ~gb).sum()), int(rb.sum())))
                if not _bad(got["dw1"][31]).all():
                    failures.append("detector: %s at %s, zero_dy %s: the dw1 row of x's channel is not non-finite throughout" % (valname, posname, zero_dy))
                for k in tally:
                    tally[k][0] += int(_bad(ref[k]).sum())
                    tally[k][1] += int((_bad(ref[k]) & _bad(got[k])).sum())
            _row("pw_forward/backward", "nvox %d vps %d" % (nvox, vps), "impl %d" % impl, "x", valname, "d_dec zero at the voxel" if zero_dy else "d_dec random",
                 "  ".join("%s ref %d dev %d" % (k, a, b) for k, (a, b) in tally.items()))
    assert not failures, failures


# ---- 3a. backward-filter: the detector -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1, 3, 4])
@pytest.mark.parametrize("name", nc.WGRAD_NAMES)
def test_conv3d_wgrad_detects(dev, name, impl):
    from tests.test_gpu_parity import _geom
    L = _L()
    _, N, hwt, Cin, Cout, k, pad, reflect, relu = nc.conv_case(name)[:9]
    ho = nc.conv_inputs(name)["ho"]
    g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    nbytes = L.lib().probav_conv3d_wgrad_scratch_bytes(ctypes.byref(g), impl)
    if impl != 0 and nbytes == 0:
        assert not (impl == 4 and name in nc.WGRAD_ON_IMPL4), "a shipped-layer shape must reach the default family's backward-filter: the routing emptied this test"
        pytest.skip("geometry not covered by this MFMA backward-filter kernel (the engine falls back)")
    scratch = torch.empty(nbytes // 4 + 1, device=dev)
    failures = []
    for kind, valname in nc.WGRAD_VARIANTS:
        if kind == "dy-closed" and not relu:
            continue                                                                   # (no gate: the same launch as dy-open)
        d = nc.wgrad_inputs(name, kind, valname)
        dw, db = torch.full(k + (Cin, Cout), 12345.0, device=dev), torch.full((Cout,), 12345.0, device=dev)
        xd, dyd, gd = _t(d["x"], dev), _t(d["dy"], dev), _t(d["gate"], dev)
        L.check(L.lib().probav_conv3d_wgrad(ctypes.byref(g), L.ptr(xd), L.ptr(dyd), L.ptr(gd), L.ptr(dw), L.ptr(db), L.ptr(scratch), nbytes, impl,
                                            L.current_stream()), "probav_conv3d_wgrad")
        dw, db = dw.cpu().numpy(), db.cpu().numpy()
        ref_w, ref_b = nc.wgrad_reference(name, kind, valname)
        ref_ci = _bad(ref_w).any(axis=(0, 1, 2, 4))
        dev_ci = _bad(dw).any(axis=(0, 1, 2, 4))
        _row("conv3d_wgrad", name, "impl %d" % impl, kind, valname, "reference: %d [ci] slices of dw, %d of db non-finite" % (int(ref_ci.sum()), int(_bad(ref_b).sum())),
             "device marks %d of those slices, %d of db" % (int((ref_ci & dev_ci).sum()), int((_bad(ref_b) & _bad(db)).sum())))
        if (_bad(ref_w).any() or _bad(ref_b).any()) and not (_bad(dw).any() or _bad(db).any()):
            failures.append("%s %s: the reference's dw / db is non-finite, the device's is finite throughout" % (kind, valname))
        if (ref_ci & ~dev_ci).any() or (_bad(ref_b) & ~_bad(db)).any():                  # (more than the contract's "at least one": what the table says)
            failures.append("%s %s: %d [ci] slices / %d db entries the reference marks are finite on the device"
                            % (kind, valname, int((ref_ci & ~dev_ci).sum()), int((_bad(ref_b) & ~_bad(db)).sum())))
    assert not failures, failures


# ---- 3a. weight normalisation ----------------------------------------------------------------------------------------------------------------------
def _small_model(dev, params, impl=None):
    from probav_amd.modelsTF import WDSRConv3D
    a = nc.ARCH
    m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, a["numFilters"], (3, 3, 3), a["numResBlocks"], a["expRate"], a["decayRate"],
                                                                      a["numImgLR"], 16, True, seed=0)
    m.load_variables(params)
    m = m.to(dev)
    if impl is not None:
        m.set_impl(impl)
    return m


def _wn_run(dev, m, flat, dweff):
    L, h = _L(), m._handle()
    nw, ncout = L.lib().probav_weff_count(h), L.lib().probav_cout_total(h)
    weff, weffT, invn = (torch.full((n,), 12345.0, device=dev) for n in (nw, nw, ncout))
    L.check(L.lib().probav_wn_forward(h, L.ptr(flat), L.ptr(weff), L.ptr(weffT), L.ptr(invn), L.current_stream()), "probav_wn_forward")
    grads = torch.zeros_like(flat)
    L.check(L.lib().probav_wn_backward(h, L.ptr(flat), L.ptr(dweff), L.ptr(invn), L.ptr(grads), L.current_stream()), "probav_wn_backward")
    return weff.cpu().numpy(), grads.cpu().numpy()


def test_weight_norm_nonfinite(dev):
    from oracle import wdsr_torch as ot
    params = nc.clean_inputs()[3]
    m = _small_model(dev, params)
    woff, off = {}, 0
    for Lh in m.layers:
        woff[Lh.name] = off
        off += int(np.prod(Lh.vshape))
    flat0 = m.flat.detach().clone()
    dweff0 = torch.as_tensor(np.random.default_rng(7).normal(size=off).astype(np.float32)).to(dev)
    weff_c, grads_c = _wn_run(dev, m, flat0, dweff0)
    assert np.isfinite(weff_c).all() and np.isfinite(grads_c).all()
    failures = []
    for layer in ("normConv_1", "expConv_0"):                                          # a 3x3x3 layer and a 1x1x1 layer
        Lh = next(q for q in m.layers if q.name == layer)
        n, col, k = int(np.prod(Lh.vshape)), 3, 5
        for target in ("g", "v", "dweff"):
            for valname, value in nc.VALUES:
                flat, dweff = flat0.clone(), dweff0.clone()
                if target == "g":
                    flat[Lh.g_off + col] = value
                elif target == "v":
                    flat[Lh.v_off + k * Lh.cout + col] = value
                else:
                    dweff[woff[layer] + k * Lh.cout + col] = value
                weff, grads = _wn_run(dev, m, flat, dweff)
                fl = flat.cpu().numpy()
                vt = torch.tensor(fl[Lh.v_off:Lh.b_off].reshape(Lh.vshape), dtype=torch.float64, requires_grad=True)
                gt = torch.tensor(fl[Lh.g_off:Lh.v_off], dtype=torch.float64, requires_grad=True)
                wt = ot.weight_norm(vt, gt)
                (wt * torch.tensor(dweff.cpu().numpy()[woff[layer]:woff[layer] + n].reshape(Lh.vshape), dtype=torch.float64)).sum().backward()
                ref_w, ref_g = _bad(wt.detach().numpy().reshape(-1)), _bad(np.concatenate([gt.grad.numpy(), vt.grad.numpy().reshape(-1)]))
                dev_w, dev_g = _bad(weff[woff[layer]:woff[layer] + n]), _bad(grads[Lh.g_off:Lh.b_off])
                _row("wn_forward/backward", layer, target, valname, "weff: reference %d, device marks %d of them (%d in all)" % (ref_w.sum(), (ref_w & dev_w).sum(), dev_w.sum()),
                     "dg|dv: reference %d, device marks %d of them (%d in all)" % (ref_g.sum(), (ref_g & dev_g).sum(), dev_g.sum()))
                if (ref_w & ~dev_w).any():
                    failures.append("%s %s %s: weff does not cover the reference's non-finite pattern" % (layer, target, valname))
                if (ref_g & ~dev_g).any():
                    failures.append("%s %s %s: the gradient slice does not cover the reference's non-finite pattern" % (layer, target, valname))
                for other in m.layers:                                                   # every other layer: bit for bit the clean run
                    if other.name == layer:
                        continue
                    no = int(np.prod(other.vshape))
                    if not _same(weff[woff[other.name]:woff[other.name] + no], weff_c[woff[other.name]:woff[other.name] + no]) \
                            or not _same(grads[other.g_off:other.b_off], grads_c[other.g_off:other.b_off]):
                        failures.append("%s %s %s: layer %s changed" % (layer, target, valname, other.name))
    assert not failures, failures


# ---- 3a. the three losses ------------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [("shift", 30), ("shift", 5), ("edge", 30), ("edge", 7), ("revssim", 30), ("revssim", 6)]      # B = 3, border = 2; the smallest crop each accepts: 1, 3, 2


def _loss_outputs(dev, case, hd, mu8, pd):
    """Every output of the loss's forward and backward entry points for one pred, as numpy: {name: array}."""
    from tests import test_gpu_losses as tl
    out = {}
    if case["loss"] == "shift":
        rc, f, arg, means = tl._c_shift_forward(dev, hd, mu8, pd, case)
        assert rc == 0
        out.update(l1=f[0], l2=f[1], cpsnr=f[2], arg_l1=arg[0], arg_l2=arg[1], means=means)
        for which in (1, 2):
            rc, dp = tl._c_shift_backward(dev, hd, mu8, pd, arg[which - 1].contiguous(), case, which, None)
            assert rc == 0
            out["grad_l%d" % which] = dp
    elif case["loss"] == "edge":
        rc, loss, arg, mean = tl._c_edge_forward(dev, hd, mu8, pd, case)
        assert rc == 0
        rc, dp = tl._c_edge_backward(dev, hd, mu8, pd, arg, case, None)
        assert rc == 0
        out.update(loss=loss, arg=arg, means=mean[:1], grad=dp)
    else:
        rc, loss, arg, dp, _ = tl._c_revssim(dev, hd, mu8, pd, case, None)
        assert rc == 0
        out.update(loss=loss, arg=arg, grad=dp)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("loss,S", LOSS_SHAPES, ids=["%s-S%d" % s for s in LOSS_SHAPES])
def test_losses_nonfinite(dev, loss, S):
    from tests import loss_cases as lc
    B, border = 3, 2
    case = lc._case(loss, S, border, B, 900 + S, kind="faint" if loss == "revssim" else "random", mask="random" if S == 30 else "full")
    hr, mask, pred = lc.inputs(case)
    hd, mu8 = torch.as_tensor(hr).to(dev), torch.as_tensor(mask).to(dev).contiguous().view(torch.uint8)
    clean = _loss_outputs(dev, case, hd, mu8, torch.as_tensor(pred).to(dev))
    assert all(np.isfinite(v).all() for k, v in clean.items() if k != "cpsnr")         # (a crop of one pixel: l2 = 0 exactly, its cPSNR is +inf)
    L_ = S - 2 * border
    ring = np.ones((S, S), bool)
    ring[border:S - border, border:S - border] = False
    b = nc.POISONED
    mates = [n for n in range(B) if n != b]
    for valname, value in nc.VALUES[:2]:                                               # NaN and +inf
        for where, pos in (("crop", (b, border + L_ // 2, border + L_ // 2, 0)), ("ring", (b, 0, S // 2, 0))):
            p2 = pred.copy()
            p2[pos] = value
            got = _loss_outputs(dev, case, hd, mu8, torch.as_tensor(p2).to(dev))
            if where == "ring":                                                        # never read: everything is the clean run, bit for bit
                for key in clean:
                    same = np.array_equal(got[key], clean[key]) if clean[key].dtype.kind == "i" else _same(got[key], clean[key])
                    assert same, (valname, "ring", key)
                continue
            grads = [key for key in got if key.startswith("grad")]
            if loss == "revssim":                                                      # one scalar for the batch
                _row("revssim", "S %d" % S, valname, "loss %r" % float(got["loss"][0]), "gradient: %d of %d elements non-finite" % (_bad(got["grad"]).sum(), got["grad"].size))
                assert not np.isfinite(got["loss"][0])
                continue
            per = ("l1", "l2", "cpsnr") if loss == "shift" else ("loss",)
            _row(loss, "S %d" % S, valname, "  ".join("%s[%d] %r" % (key, b, float(got[key][b])) for key in per), "means %s" % got["means"].tolist(),
                 "  ".join("%s: crop %d of %d non-finite" % (key, _bad(got[key][b, ~ring]).sum(), (~ring).sum()) for key in grads))
            for key in per:
                assert not np.isfinite(got[key][b]), (valname, key)                    # the sample's loss
                assert _same(got[key][mates], clean[key][mates]), (valname, key)       # its batch mates' outputs
            assert not np.isfinite(got["means"]).any()                                 # the batch means hold the sample
            for key in [q for q in got if q.startswith("arg")]:
                assert np.array_equal(got[key][mates], clean[key][mates])
            for key in grads:
                gk = got[key][..., 0]
                assert _bad(gk[b][~ring]).all(), (valname, key, "the gradient of the sample is non-finite inside the crop")
                assert (gk[b][ring] == 0).all(), (valname, key, "and exactly 0 on the ring")
                assert _same(gk[mates], clean[key][..., 0][mates]), (valname, key, "the other samples' gradients are the clean run's")


def test_clip_round_nonfinite(dev):
    """probav_clip_round is rint(min(max(x, lo), hi)) with fmaxf / fminf: NaN -> lo, +inf -> hi, -inf -> lo.  Kept and documented: the
    three rint(clip(...)) statements of ensemble.py, tiles.py and frame_windows.py and their numpy mirrors say the same, and a NaN prediction is refused
    earlier -- contract P at the parameters, contract I at the prediction, which test.py's caller can check before the clip."""
    L = _L()
    x = torch.tensor([NAN32, float("inf"), float("-inf"), 12.5, -3.0], device=dev)
    y = torch.full_like(x, 777.0)
    L.check(L.lib().probav_clip_round(L.ptr(x), L.ptr(y), x.numel(), 0.0, 65536.0, L.current_stream()))
    _row("clip_round", "lo 0 hi 65536", "nan -> %r, +inf -> %r, -inf -> %r" % tuple(y.tolist()[:3]))
    assert y.tolist() == [0.0, 65536.0, 0.0, 12.0, 0.0]


# ---- 3b. the whole step ------------------------------------------------------------------------------------------------------------------------------
def _losses():
    from probav_amd.loss import Losses
    return Losses(targetShape=(48, 48, 1))


def _guard_skip(g):
    """A real probav_grad_guard call with skip_nonfinite = 1 on the device gradient -> the control block's skip word."""
    from probav_amd import ops
    ctl = torch.zeros(ops.GUARD_CTL_WORDS, dtype=torch.int32, device=g.device)
    scratch = torch.empty(ops.guard_scratch_doubles(g.numel()), dtype=torch.float64, device=g.device)
    torch.ops.probav.grad_guard(g, ctl, scratch, 0.0, True)
    return int(ctl.cpu()[1])


def _device_step(m, case, xd, hd, md, dyd):
    """One forward + backward on the device -> (prediction, loss or None, flat gradient)."""
    m.flat.grad = None
    pred = m(xd, training=True)
    if case["site"] == "dy":
        (g,) = torch.autograd.grad(pred, m.flat, dyd)
        return pred.detach(), None, g
    loss = _losses().shiftCompensatedL1Loss(hd, md, pred)
    loss.backward()
    return pred.detach(), float(loss.detach()), m.flat.grad.detach().clone()


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", nc.STEP_CASES, ids=nc.ids(nc.STEP_CASES))
def test_training_step_shows_nonfinite_to_the_guard(dev, case, impl):
    """Contract T through probav_grad_guard and through make_optimizer(..., skip_nonfinite=True).step(), side-stream modes 0 and 2; contracts S and I
    on the training pass's own prediction (which normalises its weights itself: no weight cache)."""
    from probav_amd.trainClass import make_optimizer
    ref = nc.reference_step(case)
    assert nc.step_is_nonfinite(ref)
    x, hr, mask, params = nc.clean_inputs()
    xs, ps, dy = nc.apply_case(case, x, params, nc.upstream() if case["site"] == "dy" else None)
    m = _small_model(dev, ps, impl)
    xd, hd, md, dyd = _t(xs, dev), _t(hr, dev), torch.as_tensor(mask).to(dev), _t(dy, dev)
    for mode in (0, 2):
        m.set_side_stream_mode(mode)
        pred, loss, g = _device_step(m, case, xd, hd, md, dyd)
        skip = _guard_skip(g)
        nbad = int((~torch.isfinite(g)).sum())
        _row("step", case["id"], "impl %d" % impl, "side-stream mode %d" % mode, "reference: loss %r, %d non-finite gradient elements" % (ref["loss"], int(_bad(ref["grad"]).sum())),
             "device: loss %r, %d non-finite gradient elements, skip %d" % (loss, nbad, skip),
             "prediction non-finite in samples %s (reference %s)" % ([b for b in range(nc.BATCH) if not bool(torch.isfinite(pred[b]).all())], nc.poisoned_samples(ref)))
        assert (loss is not None and not np.isfinite(loss)) or skip == 1, "contract T: the reference's step is non-finite and the device shows nothing"
        for b in nc.poisoned_samples(ref):                                              # contract I on the training pass
            assert not bool(torch.isfinite(pred[b]).all()), "contract I (training pass): sample %d" % b
        if case["site"] == "input":                                                     # contract S, training and inference
            clean_train = m(_t(x, dev), training=True).detach()
            with torch.no_grad():
                clean_inf, pois_inf = m(_t(x, dev)), m(xd)
            for b in (0, 2):
                assert _tsame(pred[b], clean_train[b]) and _tsame(pois_inf[b], clean_inf[b]) and _tsame(clean_inf[b], clean_train[b]), "contract S: sample %d" % b
    # the optimizer path: two steps with this gradient; the first creates the state, across the second everything must stand still
    before = m.flat.detach().clone()
    opt = make_optimizer("nadam", m, 5e-4, skip_nonfinite=True)
    m.flat.grad = g.clone()
    opt.step()
    st = opt.state[m.flat]
    keep = {"m": st["m"].clone(), "v": st["v"].clone(), "wc": m.weight_cache_buffer().clone()}
    assert int(opt._ctl.cpu()[1]) == 1 and _tsame(m.flat, before)
    assert not bool(st["m"].any()) and not bool(st["v"].any())
    m.flat.grad = g.clone()
    opt.step()
    c = opt._ctl.cpu()
    assert int(c[1]) == 1 and int(c[2]) == 2
    assert _tsame(m.flat, before) and _tsame(st["m"], keep["m"]) and _tsame(st["v"], keep["v"])
    assert m.weight_cache() is not None and _tsame(m.weight_cache_buffer(), keep["wc"])


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", nc.FORWARD_CASES, ids=nc.ids(nc.FORWARD_CASES))
def test_inference_shows_nonfinite(dev, case, impl):
    """Contract I with training=False: the pass runs from the weight cache (built on the first call), and again from a weights_from scope."""
    ref = nc.reference_step(case)
    want = nc.poisoned_samples(ref)
    assert want
    x, hr, mask, params = nc.clean_inputs()
    xs, ps, _ = nc.apply_case(case, x, params)
    m = _small_model(dev, ps, impl)
    with torch.no_grad():
        y = m(_t(xs, dev))
        assert m.weight_cache() is not None
        with m.weights_from(m.flat.detach().clone()):
            y2 = m(_t(xs, dev))
    assert _tsame(y, y2)
    got = [b for b in range(nc.BATCH) if not bool(torch.isfinite(y[b]).all())]
    _row("inference", case["id"], "impl %d" % impl, "reference: samples %s non-finite" % want, "device: samples %s, %d elements" % (got, int((~torch.isfinite(y)).sum())))
    assert set(want) <= set(got), "contract I: the reference's prediction of samples %s is non-finite, the device's only of %s" % (want, got)
    if case["site"] == "input":
        assert got == want                                                              # and contract S says the others are clean


@pytest.mark.parametrize("impl", IMPLS)
def test_large_but_finite_stays_finite(dev, impl):
    """(e): the gain of normConv_0 times 2^40.  Both references are finite; the device must be, within the suite's 2e-5 of max |ref|: the scale
    arithmetic of the H3 family (amax slots, exponents) must not manufacture an inf."""
    case = nc.LARGE_CASE
    ref = nc.reference_step(case, torch.float64)
    x, hr, mask, params = nc.clean_inputs()
    xs, ps, _ = nc.apply_case(case, x, params)
    m = _small_model(dev, ps, impl)
    pred, loss, g = _device_step(m, case, _t(xs, dev), _t(hr, dev), torch.as_tensor(mask).to(dev), None)
    e = float(np.abs(pred.cpu().double().numpy() - ref["pred"]).max() / np.abs(ref["pred"]).max())
    _row("step", case["id"], "impl %d" % impl, "prediction err / max |ref| %.3g" % e, "loss %r (reference %r)" % (loss, ref["loss"]),
         "%d non-finite gradient elements" % int((~torch.isfinite(g)).sum()))
    assert bool(torch.isfinite(pred).all()) and np.isfinite(loss) and bool(torch.isfinite(g).all()) and _guard_skip(g) == 0
    assert e < 2e-5 and abs(loss - ref["loss"]) < 1e-5 * abs(ref["loss"])


def test_trainer_drops_the_overflowing_step_and_goes_on(dev, tmp_path):
    """Three trainer steps in the style of tests/test_gpu_optim_guard.py::test_trainer_with_all_three_options; before the second one the gains are
    scaled as in (b) (finite parameters, the fp32 network overflows), before the third they are put back.  Skipped steps: 0, 1, 1."""
    from probav_amd.trainClass import ModelTrainer, make_optimizer
    case = nc.by_id("b-overflow-normConv_0")
    x, hr, mask, params = nc.clean_inputs()
    _, scaled, _ = nc.apply_case(case, x, params)
    m = _small_model(dev, params)
    lo = _losses()
    opt = make_optimizer("nadam", m, 5e-4, skip_nonfinite=True)
    tr = ModelTrainer(m, lo.shiftCompensatedL1Loss, lo.shiftCompensatedcPSNR, opt, str(tmp_path / "ck"), str(tmp_path / "lg"), evalStep=100)
    tr.tune_side_stream = False
    calls, saved = [0], {}
    gains = [(L.name, L.g_off, L.v_off) for L in m.layers if not np.array_equal(scaled[L.name]["g"], params[L.name]["g"])]
    assert {n for n, _, _ in gains} == {"normConv_0", "decConv_0"}

    def before_forward(module, args, kwargs):
        if not kwargs.get("training"):
            return None
        calls[0] += 1
        with torch.no_grad():
            for name, lo_, hi_ in gains:
                if calls[0] == 2:                                                       # site (b) goes in
                    saved[name] = m.flat[lo_:hi_].clone()
                    m.flat[lo_:hi_] = torch.as_tensor(scaled[name]["g"]).to(dev)
                elif calls[0] == 3:                                                     # ... and out: the dropped step left the parameters alone
                    assert _tsame(m.flat[lo_:hi_], torch.as_tensor(scaled[name]["g"]).to(dev))
                    m.flat[lo_:hi_] = saved[name]
        return None
    m.register_forward_pre_hook(before_forward, with_kwargs=True)
    X = np.concatenate([x, x[::-1], x])
    H, M = np.concatenate([hr, hr[::-1], hr]), np.concatenate([mask, mask[::-1], mask])
    tr.fitTrainData(X, [H, M], nc.BATCH, 1, [X[:3], H[:3], M[:3]], valSteps=1, saveBestOnly=False)
    assert tr.step == 3 and calls[0] == 3
    events = [json.loads(l) for l in open(os.path.join(str(tmp_path / "lg"), "events.jsonl"))]
    skipped = [e["value"] for e in events if e["tag"] == "Skipped steps"]
    norms = [e["value"] for e in events if e["tag"] == "Grad norm"]
    print("Skipped steps %s  Grad norm %s" % (skipped, norms))
    assert skipped == [0.0, 1.0, 1.0], skipped
    assert np.isfinite(norms[0]) and not np.isfinite(norms[1]) and np.isfinite(norms[2])
    assert bool(torch.isfinite(m.flat).all())
    st = opt.state[m.flat]
    assert bool(torch.isfinite(st["m"]).all()) and bool(torch.isfinite(st["v"]).all())
