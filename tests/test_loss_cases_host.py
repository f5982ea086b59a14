"""The case table of tests/loss_cases.py, proved on the host with the fp64 oracle alone: the conditions under which comparing the device
with the oracle case by case, with no pixel and no sample left out, is meaningful.

(a) every candidate of every non-empty-mask case is finite;
(b) the oracle's best candidate is ahead of the second best by at least 1e-9 relative, per sample (per batch for l1msssim): any fp64
    evaluation, whatever its summation order (error ~1e-15), decides the arg-min the same way;
(c) sobel_l1_mix: every |Gy|, |Gx| at the winning shift is exactly 0 or above 1e-2 -- the device keeps D as fp32 in LDS (absolute error
    ~1e-3 at 16-bit magnitudes, times the Sobel weights' sum 8), so no Sobel sign is undecidable; with no pixel excluded;
(d) the gradient of the winning shift is not identically zero for any sample with a clear pixel (except where the case is built to have
    none: an exact registration): the L1 sign term is mixed, so a wrong sign or bias term would show;
and what the table claims of its special cases: the ties tie bit for bit on a pair of distinct shifts, the 'unrelated' case has samples whose
L1 and L2 arg-mins differ, the 'exact' cases have l2 = 0 and the empty-mask cases are empty where they say."""
import numpy as np
import pytest

from oracle import wdsr_numpy as on
from tests import loss_cases as lc

GAP = 1e-9


def _tables(case):
    hr, mask, pred = lc.inputs(case)
    b = case["border"]
    if case["loss"] == lc.SHIFT:
        return list(on.shift_tables(hr, mask, pred, b))
    if case["loss"] == lc.EDGE:
        return [on.shift_l1edge_table(hr, mask, pred, b, float(np.float32(case["pi"])))]
    return [on.shift_revssim_table(hr, mask, pred, b, case["bit_depth"], float(np.float32(case["eta"])))[:, None]]


@pytest.mark.parametrize("case", lc.ALL_CASES, ids=lc.ids(lc.ALL_CASES))
def test_case_is_decidable(case):
    hr, mask, pred = lc.inputs(case)
    assert hr.shape == mask.shape == pred.shape == (case["B"], case["S"], case["S"], 1)
    assert hr.dtype == pred.dtype == np.float32 and mask.dtype == bool
    empty = case["mask"] in ("row0", "none1")
    for t in _tables(case):
        assert t.shape[0] == (2 * case["border"] + 1) ** 2
        if not empty:
            assert np.isfinite(t).all()                                             # (a)
        elif case["mask"] == "none1":
            dead = np.isnan(t).all(axis=0)
            if case["loss"] == lc.REVSSIM:
                assert dead.all()                                                   # one scalar per shift for the batch: NaN with any dead sample
            else:
                assert list(np.flatnonzero(dead)) == lc.empty_samples(case)
                assert np.isfinite(np.delete(t, lc.empty_samples(case), axis=1)).all()
        else:                                                                       # row0: sample 0 has candidates under i = 0 only
            ns = 2 * case["border"] + 1
            assert np.isfinite(t[:ns]).all() and np.isnan(t[ns:, 0]).all() and np.isfinite(t[:, 1:]).all()
        if lc.is_tie(case):
            continue
        gap = on.second_best_gap(t)
        alive = ~np.isnan(t).all(axis=0)
        assert (gap[alive] >= GAP).all(), gap.min()                                 # (b)


# (left out: the cases built to have a zero gradient -- an exact registration -- or an all-NaN one -- a batch-level loss with a dead sample)
GRADIENT_CASES = [c for c in lc.ALL_CASES if c["kind"] != "exact" and not (c["loss"] == lc.REVSSIM and c["mask"] == "none1")]


@pytest.mark.parametrize("case", GRADIENT_CASES, ids=lc.ids(GRADIENT_CASES))
def test_gradient_is_not_degenerate(case):
    hr, mask, pred = lc.inputs(case)
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = lc.oracle_gradients(case, hr, mask, pred)
    live = [b for b in range(case["B"]) if b not in lc.empty_samples(case)]
    for name, (_, g) in grads.items():
        assert np.isfinite(g[live]).all()
        assert (np.abs(g[live]).max(axis=(1, 2, 3)) > 0).all(), name                # (d)
        c = case["border"]
        ring = np.ones(g.shape[1:3], bool)
        ring[c:case["S"] - c, c:case["S"] - c] = False
        assert (g[:, ring] == 0).all()


@pytest.mark.parametrize("case", lc.EDGE_CASES, ids=lc.ids(lc.EDGE_CASES))
def test_sobel_signs_are_decidable(case):
    hr, mask, pred = lc.inputs(case)
    t = on.shift_l1edge_table(hr, mask, pred, case["border"], float(np.float32(case["pi"])))
    _, arg = on.select_min(t)
    keep = [b for b in range(case["B"]) if b not in lc.empty_samples(case)]
    _, gy, gx = on.shift_l1edge_sobel_at(hr[keep], mask[keep], pred[keep], arg[keep], case["border"])
    g = np.abs(np.concatenate([gy.ravel(), gx.ravel()]))
    assert ((g == 0) | (g > 1e-2)).all(), np.sort(g[g > 0])[:3]                     # (c), cap 0: no pixel excluded


@pytest.mark.parametrize("case", lc.SHIFT_TIES + lc.EDGE_TIES + lc.REVSSIM_TIES, ids=lc.ids(lc.SHIFT_TIES + lc.EDGE_TIES + lc.REVSSIM_TIES))
def test_ties_tie_bit_for_bit(case):
    """Every sample (the batch for l1msssim) has its minimum on at least two distinct shifts with identical fp64 values, and the gradients of
    the first and the second of them differ where the table says the crops are mirror images (the split gradient is then a third one)."""
    ns = 2 * case["border"] + 1
    for t in _tables(case):
        v, a = on.select_min(t)
        for b in range(t.shape[1]):
            tied = np.flatnonzero(t[:, b] == v[b])
            assert len(tied) >= 2 and tied[0] == a[b], (b, tied)
            i, j = divmod(int(tied[0]), ns)
            partner = i * ns + (ns - 1 - j) if case["kind"] == "tie_lr" else i * ns + j + 2
            assert partner in tied, (b, tied)
    if case["kind"] == "tie_lr" and case["loss"] == lc.SHIFT:
        hr, mask, pred = lc.inputs(case)
        t1, _ = on.shift_tables(hr, mask, pred, case["border"])
        _, a = on.select_min(t1)
        single = on.shift_grad_at(hr, mask, pred, a, case["border"], 1)
        split = on.shift_l1_grad(hr, mask, pred, case["border"])
        assert np.abs(single - split).max() > 1e-3 * np.abs(single).max()


def test_arg_l1_and_arg_l2_differ_somewhere():
    hr, mask, pred = lc.inputs(lc.SHIFT_ARGS_DIFFER)
    r = on.shift_per_sample(hr, mask, pred, lc.SHIFT_ARGS_DIFFER["border"])
    assert (r["arg_l1"] != r["arg_l2"]).any()


@pytest.mark.parametrize("case", lc.SHIFT_EXACT, ids=lc.ids(lc.SHIFT_EXACT))
def test_exact_shift_has_zero_error(case):
    hr, mask, pred = lc.inputs(case)
    c, ns = case["border"], 2 * case["border"] + 1
    r = on.shift_per_sample(hr, mask, pred, c)
    want = 1 * ns + 2 * c - 1 if c else 0
    assert (r["l1"] == 0).all() and (r["l2"] == 0).all() and np.isposinf(r["cpsnr"]).all()
    assert (r["arg_l1"] == want).all() and (r["arg_l2"] == want).all()
    assert (on.shift_grad_at(hr, mask, pred, r["arg_l1"], c, 1) == 0).all()


def test_table_covers_what_it_promises():
    """The shapes at which the kernels take another path are all present."""
    crops = {(c["S"], c["border"]) for c in lc.SHIFT_CASES}
    assert {(8, 1), (9, 1), (12, 1), (22, 3), (23, 3), (48, 3), (16, 0), (20, 4), (21, 5)} <= crops
    assert {1, 63, 64, 65, 128, 1024, 1025, 1100} <= {c["B"] for c in lc.SHIFT_CASES if (c["S"], c["border"]) == (8, 1)}
    assert {8, 14, 16} <= {c["bit_depth"] for c in lc.SHIFT_CASES}
    e = {(c["S"], c["border"]) for c in lc.EDGE_CASES}
    assert {(5, 1), (6, 1), (7, 1), (18, 1), (19, 1), (48, 3), (72, 3), (96, 3), (12, 0), (20, 4)} <= e
    assert {1, 65, 130} <= {c["B"] for c in lc.EDGE_CASES} and {0.0, 0.7, 1.0} <= {c["pi"] for c in lc.EDGE_CASES}
    r = {(c["S"], c["border"]) for c in lc.REVSSIM_CASES}
    assert {(4, 1), (5, 1), (9, 1), (48, 3), (72, 3), (96, 3), (12, 0), (20, 4), (21, 5)} <= r
    assert {1, 2, 5, 33} <= {c["B"] for c in lc.REVSSIM_CASES} and {0.0, 0.25, 1.0} <= {c["eta"] for c in lc.REVSSIM_CASES}
    assert {8, 14, 16} <= {c["bit_depth"] for c in lc.REVSSIM_CASES}
    assert any(c["upstream"] != 1.0 for c in lc.EDGE_CASES) and any(c["upstream"] != 1.0 for c in lc.REVSSIM_CASES)
