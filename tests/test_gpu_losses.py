"""The shift-compensated losses (csrc/kernels_loss.hip: L1 / L2 / cPSNR, sobel_l1_mix, l1msssim) on the device against the fp64 oracle, at
the shapes where the kernels take another path: every case of tests/loss_cases.py, whose conditions tests/test_loss_cases_host.py proves
on the host -- so nothing is skipped here and no pixel or sample is left out.

Bars (the project's own): values and per-sample values 1e-5 relative; L1 / L2 / edge gradients 1e-5 of the gradient's max-abs; l1msssim
gradient 1e-4 of its max-abs; arg-mins equal.  A batch mean is also held to the fp64 mean of the device's own per-sample floats within one
fp32 rounding (2^-23: the kernel sums the floats in fp64 and rounds once).  Every test prints its measured figures (`LOSSFIG ...`) before it
asserts.

Measured on an MI355X, maxima over all cases (relative, the bar in brackets):
  L1 / L2 / cPSNR   per-sample l1 5.9e-8, l2 5.9e-8, cpsnr 5.4e-8 (1e-5); means against the oracle 6.1e-8 / 4.6e-8 (1e-5), against the fp64 mean of
                    the device's own floats 5.7e-8 / 3.9e-8 (2^-23 = 1.2e-7); gradients l1 1.3e-7, l2 1.3e-7 (1e-5)
  sobel_l1_mix      per-sample 6.4e-8, mean 5.5e-8 (own floats 4.7e-8), gradient 1.1e-7 (1e-5); pi = 1 against the shift kernels' L1: 0 (1e-6)
  l1msssim          value 4.8e-8 (1e-5), gradient 5.5e-8 (1e-4)
Every arg-min equal.  The cases that failed before the fixes this suite came with: the sobel_l1_mix backward at crops 66, 90 and 100 and the
l1msssim backward at crops 90 and 140 (refused: "bad shape"), the three samples-without-a-clear-pixel cases (+inf for NaN), the forwards'
refusals past the limits (accepted), and the shift backward at a patch without a crop (accepted: it returned 0 and launched)."""
import numpy as np
import pytest
import torch

from oracle import wdsr_numpy as on
from tests import loss_cases as lc

pytestmark = pytest.mark.gpu

VAL, GRAD, GRAD_SSIM, ONE_ROUNDING = 1e-5, 1e-5, 1e-4, 2.0 ** -23
NAN32 = float("nan")


def _L():
    from probav_amd import _lib
    return _lib


def _fig(case, name, value):
    print("LOSSFIG %-48s %-16s %.3e" % (case["id"], name, value))


def _dev_inputs(case, dev, mask_dtype=torch.bool):
    hr, mask, pred = lc.inputs(case)
    return (hr, mask, pred), (torch.as_tensor(hr).to(dev), torch.as_tensor(mask).to(dev).to(mask_dtype), torch.as_tensor(pred).to(dev))


def _losses(case):
    from probav_amd.loss import Losses
    lo = Losses(targetShape=(case["S"], case["S"], 1), cropBorder=case["border"], bitDepth=case["bit_depth"])
    lo.pi, lo.eta = case.get("pi", lo.pi), case.get("eta", lo.eta)
    return lo


def _value_err(dev_v, ref_v):
    """Largest elementwise relative error; an exact 0 / inf / NaN of the oracle must be reproduced exactly (-> error 0 or inf)."""
    d, r = np.asarray(dev_v, np.float64).reshape(-1), np.asarray(ref_v, np.float64).reshape(-1)
    special = ~np.isfinite(r) | (r == 0)
    same = (d[special] == r[special]) | (np.isnan(d[special]) & np.isnan(r[special]))
    if not same.all():
        return float("inf")
    if special.all():
        return 0.0
    return float((np.abs(d[~special] - r[~special]) / np.abs(r[~special])).max())


def _grad_err(case, g, gref, name):
    """Gradient error of the samples with a clear pixel, relative to the oracle's max-abs (an identically zero oracle gradient must be
    reproduced exactly).  A sample without a clear pixel: NaN inside the crop, 0 on the ring.  The ring is exactly 0 everywhere."""
    g = np.asarray(g, np.float64)
    c, S = case["border"], case["S"]
    ring = np.ones((S, S), bool)
    ring[c:S - c, c:S - c] = False
    assert (g[:, ring] == 0).all(), "%s: gradient on the border ring" % name
    dead = lc.empty_samples(case)
    live = [b for b in range(case["B"]) if b not in dead]
    for b in dead:
        assert np.isnan(g[b][~ring]).all(), "%s: a sample without a clear pixel has a NaN gradient inside the crop" % name
    assert np.isfinite(g[live]).all()
    gmax = np.abs(gref[live]).max()
    err = np.abs(g[live] - gref[live]).max()
    return float(err / gmax) if gmax > 0 else (0.0 if err == 0 else float("inf"))


def _mean_checks(case, name, mean_dev, per_dev, per_ref):
    if lc.empty_samples(case):
        assert np.isnan(mean_dev), "%s: the batch mean over a sample without a clear pixel is NaN" % name
        return
    own = float(np.asarray(per_dev, np.float64).mean())
    e_own = abs(mean_dev - own) / abs(own) if own else abs(mean_dev)
    e_ref = _value_err([mean_dev], [np.asarray(per_ref, np.float64).mean()])
    _fig(case, name + "_vs_own", e_own)
    _fig(case, name + "_vs_oracle", e_ref)
    assert e_own <= ONE_ROUNDING and e_ref <= VAL, (name, e_own, e_ref)


# ---- the C entry points, with every output pre-filled: NaN for floats, -7 for arg-mins ------------------------------------------------
def _c_shift_forward(dev, hd, md_u8, pd, case):
    L, B = _L(), case["B"]
    f = torch.full((3, B), NAN32, device=dev)
    arg = torch.full((2, B), -7, dtype=torch.int32, device=dev)
    means = torch.full((2,), NAN32, device=dev)
    rc = L.lib().probav_shift_loss_forward(L.ptr(hd), L.ptr(md_u8), L.ptr(pd), B, case["S"], case["border"], case["bit_depth"], L.ptr(f[0]), L.ptr(f[1]),
                                           L.ptr(f[2]), L.ptr(arg[0]), L.ptr(arg[1]), L.ptr(means[0:1]), L.ptr(means[1:2]), L.current_stream())
    return rc, f, arg, means


def _c_shift_backward(dev, hd, md_u8, pd, arg, case, which, upstream):
    L = _L()
    dpred = torch.full_like(pd, NAN32)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=dev)
    rc = L.lib().probav_shift_loss_backward(L.ptr(hd), L.ptr(md_u8), L.ptr(pd), L.ptr(arg), case["B"], case["S"], case["border"], which, L.ptr(up),
                                            L.ptr(dpred), L.current_stream())
    return rc, dpred


def _c_edge_forward(dev, hd, md_u8, pd, case):
    L, B = _L(), case["B"]
    loss = torch.full((B,), NAN32, device=dev)
    arg = torch.full((B,), -7, dtype=torch.int32, device=dev)
    mean = torch.full((2,), NAN32, device=dev)
    rc = L.lib().probav_shift_l1edge_forward(L.ptr(hd), L.ptr(md_u8), L.ptr(pd), B, case["S"], case["border"], case["pi"], L.ptr(loss), L.ptr(arg),
                                             L.ptr(mean), L.current_stream())
    return rc, loss, arg, mean


def _c_edge_backward(dev, hd, md_u8, pd, arg, case, upstream):
    L = _L()
    dpred = torch.full_like(pd, NAN32)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=dev)
    rc = L.lib().probav_shift_l1edge_backward(L.ptr(hd), L.ptr(md_u8), L.ptr(pd), L.ptr(arg), case["B"], case["S"], case["border"], case["pi"], L.ptr(up),
                                              L.ptr(dpred), L.current_stream())
    return rc, dpred


def _c_revssim(dev, hd, md_u8, pd, case, upstream, short=0):
    L, B = _L(), case["B"]
    nbytes = L.lib().probav_revssim_scratch_bytes(B, case["border"])
    scratch = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    loss = torch.full((1,), NAN32, device=dev)
    arg = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = L.lib().probav_revssim_forward(L.ptr(hd), L.ptr(md_u8), L.ptr(pd), B, case["S"], case["border"], case["bit_depth"], case["eta"], L.ptr(scratch),
                                        nbytes - short, L.ptr(loss), L.ptr(arg), L.current_stream())
    if rc:
        return rc, loss, arg, None, scratch
    dpred = torch.full_like(pd, NAN32)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=dev)
    rc = L.lib().probav_revssim_backward(L.ptr(hd), L.ptr(md_u8), L.ptr(pd), L.ptr(arg), L.ptr(scratch), B, case["S"], case["border"], case["bit_depth"],
                                         case["eta"], L.ptr(up), L.ptr(dpred), L.current_stream())
    return rc, loss, arg, dpred, scratch


def _u8(md):
    return md.contiguous().view(torch.uint8)


# ---- L1 / L2 / cPSNR ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.SHIFT_CASES, ids=lc.ids(lc.SHIFT_CASES))
def test_shift_losses_per_sample_means_and_gradients(dev, case):
    (hr, mask, pred), (hd, md, pd) = _dev_inputs(case, dev)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = on.shift_per_sample(hr, mask, pred, case["border"], case["bit_depth"])
        gref = lc.oracle_gradients(case, hr, mask, pred)
    lo = _losses(case)
    out = {k: v.cpu().numpy() for k, v in lo.evaluate_all(hd, md, pd).items()}
    assert (out["arg_l1"] == ref["arg_l1"]).all() and (out["arg_l2"] == ref["arg_l2"]).all()
    for k in ("l1", "l2", "cpsnr"):
        e = _value_err(out[k], ref[k])
        _fig(case, k, e)
        assert e <= VAL, (k, e)
    _mean_checks(case, "mean_l1", float(out["mean_l1"]), out["l1"], ref["l1"])
    _mean_checks(case, "mean_l2", float(out["mean_l2"]), out["l2"], ref["l2"])
    np.testing.assert_array_equal(lo.shiftCompensatedcPSNR(hd, md, pd).cpu().numpy(), out["cpsnr"])
    up = case["upstream"]
    for which, name, fn in ((1, "l1", lo.shiftCompensatedL1Loss), (2, "l2", lo.shiftCompensatedL2Loss)):
        p = pd.clone().requires_grad_(True)
        loss = fn(hd, md, p)
        (up * loss).backward()
        assert np.array_equal(loss.detach().cpu().numpy(), out["mean_" + name], equal_nan=True)       # the same launch: the same bits
        e = _grad_err(case, p.grad.cpu().numpy(), gref[name][1], name)
        _fig(case, "grad_" + name, e)
        assert e <= GRAD, (name, e)
        # the C entry point on a NaN-filled buffer: every element written, the same bits
        rc, dp = _c_shift_backward(dev, hd, _u8(md), pd, torch.as_tensor(out["arg_" + name]).to(dev), case, which, up)
        assert rc == 0
        assert np.array_equal(dp.cpu().numpy(), p.grad.cpu().numpy(), equal_nan=True)


MASK_BYTE_CASES = [lc.by_id("shift-S12-b1-B3-random-cloud-up1.7"), lc.by_id("shift-S48-b3-B3-random-cloud-up1.7")]


@pytest.mark.parametrize("case", MASK_BYTE_CASES, ids=lc.ids(MASK_BYTE_CASES))
def test_shift_losses_mask_bytes_and_dtypes(dev, case):
    """The C ABI's masks are 'non-zero = clear': raw bytes 1, 2 and 255 give the bits of the 0 / 1 mask.  Through Losses a float mask and a
    bool mask give the same bits."""
    (hr, mask, pred), (hd, md, pd) = _dev_inputs(case, dev)
    rng = np.random.default_rng(1)
    raw = torch.as_tensor(np.where(mask, rng.choice(np.array([1, 2, 255], np.uint8), mask.shape), 0).astype(np.uint8)).to(dev)
    assert set(np.unique(raw.cpu().numpy())) == {0, 1, 2, 255}
    a, b = _c_shift_forward(dev, hd, _u8(md), pd, case), _c_shift_forward(dev, hd, raw, pd, case)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y) and not torch.isnan(x.float()).any()
    for which in (1, 2):
        ga = _c_shift_backward(dev, hd, _u8(md), pd, a[2][which - 1].contiguous(), case, which, 1.3)
        gb = _c_shift_backward(dev, hd, raw, pd, a[2][which - 1].contiguous(), case, which, 1.3)
        assert ga[0] == 0 and gb[0] == 0 and torch.equal(ga[1], gb[1]) and not torch.isnan(ga[1]).any()
    lo = _losses(case)
    ob, of = lo.evaluate_all(hd, md, pd), lo.evaluate_all(hd, md.float(), pd)
    for k in ob:
        assert torch.equal(ob[k], of[k]), k
    assert torch.equal(ob["l1"], a[1][0]) and torch.equal(ob["arg_l2"], a[2][1])


def test_edge_and_l1msssim_raw_mask_bytes(dev):
    rng = np.random.default_rng(2)
    for case in (lc.by_id("edge-S18-b1-B3-random-random"), lc.by_id("revssim-S9-b1-B3-faint-random")):
        (hr, mask, pred), (hd, md, pd) = _dev_inputs(case, dev)
        raw = torch.as_tensor(np.where(mask, rng.choice(np.array([1, 2, 255], np.uint8), mask.shape), 0).astype(np.uint8)).to(dev)
        if case["loss"] == lc.EDGE:
            a, b = _c_edge_forward(dev, hd, _u8(md), pd, case), _c_edge_forward(dev, hd, raw, pd, case)
            assert a[0] == 0 and b[0] == 0, _L().lib().probav_last_error()
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3][:1], b[3][:1])
            ga, gb = _c_edge_backward(dev, hd, _u8(md), pd, a[2], case, 1.3), _c_edge_backward(dev, hd, raw, pd, a[2], case, 1.3)
            assert ga[0] == 0 and gb[0] == 0 and torch.equal(ga[1], gb[1]) and not torch.isnan(ga[1]).any()
        else:
            a, b = _c_revssim(dev, hd, _u8(md), pd, case, 1.3), _c_revssim(dev, hd, raw, pd, case, 1.3)
            assert a[0] == 0 and b[0] == 0, _L().lib().probav_last_error()
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
            assert not torch.isnan(a[3]).any()


# ---- sobel_l1_mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.EDGE_CASES, ids=lc.ids(lc.EDGE_CASES))
def test_sobel_l1_mix_per_sample_mean_and_gradient(dev, case):
    (hr, mask, pred), (hd, md, pd) = _dev_inputs(case, dev)
    pi = float(np.float32(case["pi"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref, aref = on.select_min(on.shift_l1edge_table(hr, mask, pred, case["border"], pi))
        gref = lc.oracle_gradients(case, hr, mask, pred)["edge"][1]
    rc, loss, arg, mean = _c_edge_forward(dev, hd, _u8(md), pd, case)
    assert rc == 0, _L().lib().probav_last_error()
    assert (arg.cpu().numpy() == aref).all()
    e = _value_err(loss.cpu().numpy(), ref)
    _fig(case, "edge", e)
    assert e <= VAL
    _mean_checks(case, "mean_edge", float(mean[0]), loss.cpu().numpy(), ref)
    up = case["upstream"]
    rc, dp = _c_edge_backward(dev, hd, _u8(md), pd, arg, case, up)
    assert rc == 0, _L().lib().probav_last_error()
    e = _grad_err(case, dp.cpu().numpy(), gref, "edge")
    _fig(case, "grad_edge", e)
    assert e <= GRAD
    # the same through Losses: the same launches, the same bits
    lo = _losses(case)
    p = pd.clone().requires_grad_(True)
    v = lo.shiftCompensatedL1EdgeLoss(hd, md, p)
    (up * v).backward()
    assert np.array_equal(v.detach().cpu().numpy(), mean[0].cpu().numpy(), equal_nan=True)
    assert np.array_equal(p.grad.cpu().numpy(), dp.cpu().numpy(), equal_nan=True)
    if case["pi"] == 1.0:                                        # a cross-kernel identity: pi = 1 is the L1 loss of the shift kernels
        l1 = lo.evaluate_all(hd, md, pd)
        e = _value_err(loss.cpu().numpy(), l1["l1"].cpu().numpy())
        _fig(case, "edge_pi1_vs_l1", e)
        assert e <= 1e-6 and torch.equal(arg, l1["arg_l1"])


# ---- l1msssim -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.REVSSIM_CASES, ids=lc.ids(lc.REVSSIM_CASES))
def test_l1msssim_value_and_gradient(dev, case):
    (hr, mask, pred), (hd, md, pd) = _dev_inputs(case, dev)
    eta = float(np.float32(case["eta"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref, aref = on.select_min(on.shift_revssim_table(hr, mask, pred, case["border"], case["bit_depth"], eta))
    rc, loss, arg, dp, _ = _c_revssim(dev, hd, _u8(md), pd, case, case["upstream"])
    assert rc == 0, _L().lib().probav_last_error()
    assert int(arg[0]) == int(aref)
    e = _value_err(loss.cpu().numpy(), [ref])
    _fig(case, "revssim", e)
    assert e <= VAL
    if lc.empty_samples(case):                                   # one scalar for the batch: a sample without a clear pixel makes it NaN
        assert np.isnan(float(loss[0])) and int(arg[0]) == 0
        return
    gref = on.shift_revssim_grad_at(hr, mask, pred, aref, case["border"], case["bit_depth"], eta, case["upstream"])
    e = _grad_err(case, dp.cpu().numpy(), gref, "revssim")
    _fig(case, "grad_revssim", e)
    assert e <= GRAD_SSIM
    lo = _losses(case)
    p = pd.clone().requires_grad_(True)
    v = lo.shiftCompensatedRevSSIM(hd, md, p)
    (case["upstream"] * v).backward()
    assert np.array_equal(v.detach().cpu().numpy(), loss[0].cpu().numpy()) and np.array_equal(p.grad.cpu().numpy(), dp.cpu().numpy())


# ---- refusals: argument checks, nothing launched ----------------------------------------------------------------------------------------
def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        if t is None:
            continue
        assert bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == -7).all())


def _tiny(loss, S, border, B=1, **kw):
    return lc._case(loss, S, border, B, 1, **kw)


def _last_error():
    return _L().lib().probav_last_error().decode()


@pytest.mark.parametrize("S,border", [(6, 3), (2, 1), (5, 3)])
def test_shift_losses_refuse_a_patch_without_a_crop(dev, S, border):
    case = _tiny(lc.SHIFT, max(S, 1), border)
    z = torch.zeros((1, 8, 8, 1), device=dev)
    m = torch.ones((1, 8, 8, 1), dtype=torch.uint8, device=dev)
    rc, f, arg, means = _c_shift_forward(dev, z, m, z, case)
    assert rc == _L().PROBAV_EINVAL
    _untouched(f, arg, means)
    rc, dp = _c_shift_backward(dev, z, m, z, torch.zeros(1, dtype=torch.int32, device=dev), case, 1, None)
    assert rc == _L().PROBAV_EINVAL
    _untouched(dp)


@pytest.mark.parametrize("which", [0, 3, -1])
def test_shift_backward_refuses_an_unknown_loss(dev, which):
    case = _tiny(lc.SHIFT, 8, 1)
    z = torch.zeros((1, 8, 8, 1), device=dev)
    m = torch.ones((1, 8, 8, 1), dtype=torch.uint8, device=dev)
    rc, dp = _c_shift_backward(dev, z, m, z, torch.zeros(1, dtype=torch.int32, device=dev), case, which, None)
    assert rc == _L().PROBAV_EINVAL and "which" in _last_error()
    _untouched(dp)


def test_edge_loss_refuses_small_and_oversized_crops_in_the_forward(dev):
    """L < 3 and L = 101 (one past the limit): PROBAV_EINVAL from the FORWARD and from the backward, the limit named, nothing launched."""
    from probav_amd.loss import L1EDGE_MAX_CROP, Losses
    assert L1EDGE_MAX_CROP == 100
    for S, border, named in ((4, 1, None), (L1EDGE_MAX_CROP + 3, 1, str(L1EDGE_MAX_CROP)), (L1EDGE_MAX_CROP + 7, 3, str(L1EDGE_MAX_CROP))):
        case = _tiny(lc.EDGE, S, border)
        z = torch.zeros((1, S, S, 1), device=dev)
        m = torch.ones((1, S, S, 1), dtype=torch.uint8, device=dev)
        rc, loss, arg, mean = _c_edge_forward(dev, z, m, z, case)
        assert rc == _L().PROBAV_EINVAL and (named is None or named in _last_error()), _last_error()
        _untouched(loss, arg, mean)
        rc, dp = _c_edge_backward(dev, z, m, z, torch.zeros(1, dtype=torch.int32, device=dev), case, None)
        assert rc == _L().PROBAV_EINVAL and (named is None or named in _last_error())
        _untouched(dp)
        with pytest.raises(ValueError, match=named or "shape"):
            Losses(targetShape=(S, S, 1), cropBorder=border).shiftCompensatedL1EdgeLoss(z, m, z.clone().requires_grad_(True))


def test_l1msssim_refuses_small_and_oversized_crops_and_a_short_scratch(dev):
    from probav_amd.loss import REVSSIM_MAX_CROP, Losses
    assert REVSSIM_MAX_CROP == 140
    for S, border, named in ((3, 1, None), (REVSSIM_MAX_CROP + 3, 1, str(REVSSIM_MAX_CROP))):
        case = _tiny(lc.REVSSIM, S, border)
        z = torch.zeros((1, S, S, 1), device=dev)
        m = torch.ones((1, S, S, 1), dtype=torch.uint8, device=dev)
        rc, loss, arg, dp, scratch = _c_revssim(dev, z, m, z, case, None)
        assert rc == _L().PROBAV_EINVAL and (named is None or named in _last_error()), _last_error()
        _untouched(loss, arg)
        assert bool((scratch == 0).all())
        dpred = torch.full_like(z, NAN32)
        L = _L()
        rc = L.lib().probav_revssim_backward(L.ptr(z), L.ptr(m), L.ptr(z), L.ptr(torch.zeros(1, dtype=torch.int32, device=dev)), L.ptr(scratch), 1, S, border,
                                             16, 0.25, None, L.ptr(dpred), L.current_stream())
        assert rc == L.PROBAV_EINVAL and (named is None or named in _last_error())
        _untouched(dpred)
        with pytest.raises(ValueError, match=named or "shape"):
            Losses(targetShape=(S, S, 1), cropBorder=border).shiftCompensatedRevSSIM(z, m, z.clone().requires_grad_(True))
    case = lc.by_id("revssim-S9-b1-B3-faint-random")
    _, (hd, md, pd) = _dev_inputs(case, dev)
    rc, loss, arg, dp, scratch = _c_revssim(dev, hd, _u8(md), pd, case, None, short=1)
    assert rc == _L().PROBAV_ENOSPACE
    _untouched(loss, arg)
    assert bool((scratch == 0).all())


def test_losses_refuse_a_prediction_of_another_size(dev):
    from probav_amd.loss import Losses
    lo = Losses(targetShape=(12, 12, 1), cropBorder=2)
    z = torch.zeros((1, 11, 11, 1), device=dev)
    with pytest.raises(ValueError):
        lo.evaluate_all(z, z > -1, z)
