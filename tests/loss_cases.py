"""The case table of the shift-compensated losses: one list serves tests/test_gpu_losses.py (device against the fp64 oracle) and
tests/test_loss_cases_host.py (the oracle alone, no GPU), which proves for every case the conditions that make the device comparison
meaningful -- finite candidates, a decided arg-min, decidable Sobel signs, the ties and the disagreeing arg-mins the table claims.  A case
that does not satisfy them fails THERE; the GPU tests never skip a case and leave no pixel out.

A case is a dict: id, loss ('shift' = L1 / L2 / cPSNR, 'edge' = sobel_l1_mix, 'revssim' = l1msssim), S (patch side), border, B, seed,
kind (how hr and pred are drawn), mask (how the mask is drawn) and the loss's parameters.  inputs(case) draws (hr f32, mask bool, pred f32),
all [B, S, S, 1], from numpy's default_rng(seed) alone.

kinds
  random     hr ~ N(8000, 2000) clipped to 14 bits, pred = hr + N(0, 150) rolled by (1, -2): the true registration is not the centre shift
  faint      hr ~ N(300, 20), pred = hr + N(0, 5) rolled likewise.  l1msssim calls variances "sigma": its structure term is
             (2 cov + C3) / (sH sS + C3) with sH sS a product of VARIANCES, about 1.6e13 at 14-bit contrast against C3 = 1.9e6, so the product
             over five scales is ~1e-32 and the SSIM term is the constant 1 in fp64 (every candidate ties at eta = 1, and the SSIM half of the
             gradient is ~1e-30).  With variances of 400 the term is alive and its derivative is really compared.
  unrelated  pred drawn independently of hr: all candidates are about equally bad, the L1 and L2 arg-mins disagree for some samples
  exact      integer hr, full mask, the crop of pred IS the crop of hr under shift (1, 2 * border - 1) [or (0, 0) at border 0]: l2 = 0 there
  tie_lr     integers 0..63, hr and pred left-right symmetric, full mask, S = 14, border 3: n = 64, so the bias (a multiple of 1/64) and
             every sum are exact in fp32 and fp64 alike whatever the order, and shifts (i, j) and (i, 6 - j) tie bit for bit (the crop of hr at
             (i, 6 - j) is the mirror image of the one at (i, j), the crop of pred its own mirror image).  Sobel's |Gx| and |Gy| are mirror
             symmetric too, so the edge loss ties as well.
  tie_cols   integers 0..63, hr has period 2 along x, full mask: the crops at (i, j) and (i, j + 2) are the SAME numbers in the same places,
             so every evaluation of the two candidates runs the same operations: an exact tie for any loss.  This is the tie of l1msssim:
             its windows exp(-x / (2 sigma^2)) are not symmetric in x, so a mirrored crop does not tie there.
masks
  full, random (85 % clear), cloud (random, and the top third of sample 0 covered),
  row0 (sample 0 is clear in its first row only: under every shift with i > 0 it has no clear pixel, those shifts are no candidates),
  none1 (sample 1 has no clear pixel at all; the others are random)
  Under a covered pixel hr is dim (see inputs()).
"""
import numpy as np

from oracle import wdsr_numpy as on

SHIFT, EDGE, REVSSIM = "shift", "edge", "revssim"


def _case(loss, S, border, B, seed, kind="random", mask="random", **params):
    p = {"upstream": 1.0, "bit_depth": 16}
    if loss == EDGE:
        p["pi"] = 0.7
    if loss == REVSSIM:
        p["eta"] = 0.25
    p.update(params)
    tag = "-".join("%s%g" % (k[:2], v) for k, v in sorted(params.items()))
    cid = "%s-S%d-b%d-B%d-%s-%s%s" % (loss, S, border, B, kind, mask, "-" + tag if tag else "")
    return dict(id=cid, loss=loss, S=S, border=border, B=B, seed=seed, kind=kind, mask=mask, **p)


def inputs(case):
    rng = np.random.default_rng(case["seed"])
    B, S, c, kind = case["B"], case["S"], case["border"], case["kind"]
    shape = (B, S, S, 1)
    if kind == "faint":
        hr = np.clip(rng.normal(300.0, 20.0, shape), 0, 16383).astype(np.float32)
        pred = np.roll((hr + rng.normal(0, 5, shape)).astype(np.float32), (1, -2), axis=(1, 2))
    elif kind in ("random", "unrelated"):
        hr = np.clip(rng.normal(8000.0, 2000.0, shape), 0, 16383).astype(np.float32)
        if kind == "random":
            pred = np.roll((hr + rng.normal(0, 150, shape)).astype(np.float32), (1, -2), axis=(1, 2))
        else:
            pred = np.clip(rng.normal(8000.0, 2000.0, shape), 0, 16383).astype(np.float32)
    elif kind == "exact":
        hr = rng.integers(0, 16384, shape).astype(np.float32)
        pred = rng.integers(0, 16384, shape).astype(np.float32)
        i, j = (1, 2 * c - 1) if c else (0, 0)
        L = S - 2 * c
        pred[:, c:c + L, c:c + L] = hr[:, i:i + L, j:j + L]
    elif kind == "tie_lr":
        half = lambda: rng.integers(0, 64, (B, S, (S + 1) // 2, 1))
        sym = lambda a: np.concatenate([a, a[:, :, ::-1][:, :, S % 2:]], axis=2)
        hr, pred = sym(half()).astype(np.float32), sym(half()).astype(np.float32)
    elif kind == "tie_cols":
        two = rng.integers(0, 64, (B, S, 2, 1))
        hr = np.tile(two, (1, 1, (S + 1) // 2, 1))[:, :, :S].astype(np.float32)
        pred = rng.integers(0, 64, shape).astype(np.float32)
    else:
        raise ValueError(kind)
    mk = case["mask"]
    if mk == "full":
        mask = np.ones(shape, bool)
    else:
        mask = rng.random(shape) < 0.85
        if mk == "cloud":
            mask[0, : S // 3] = False
        elif mk == "row0":
            mask[0] = False
            mask[0, 0] = True
        elif mk == "none1":
            mask[1] = False
        elif mk != "random":
            raise ValueError(mk)
        # hr under the covered pixels is dim, not dark.  The reference does not mask hr (models/loss.py:146,151), so these pixels enter the bias as
        # sum(hr[covered]) / n: a kernel that masked hr would be far off.  At full brightness that offset is ~1400, ten times the noise of pred:
        # H - C then has ONE sign on every clear pixel and the L1 gradient -(M/n)(s - sum(s M)/n) is identically zero.  Dim keeps the signs mixed.
        dim = {"random": 600.0, "unrelated": 600.0, "faint": 30.0}[kind]
        hr[~mask] = rng.uniform(0.0, dim, int((~mask).sum())).astype(np.float32)
    return hr, mask, pred


def is_tie(case):
    return case["kind"].startswith("tie")


def empty_samples(case):
    """Samples without a clear pixel under ANY shift."""
    return [1] if case["mask"] == "none1" else []


# ---- L1 / L2 / cPSNR ------------------------------------------------------------------------------------------------------------
# crops (S, border): L^2 = 36, 49, 100 (below one 256-pixel wave round), 256 exactly, 289 (one pixel into the second round), 1764;
# one shift (three idle waves); 81 and 121 shifts (the waves take three shifts of a row each)
SHIFT_CASES = [_case(SHIFT, S, b, 3, 100 + k, mask="cloud" if S >= 12 else "random", upstream=1.7)
               for k, (S, b) in enumerate([(8, 1), (9, 1), (12, 1), (22, 3), (23, 3), (48, 3), (16, 0), (20, 4), (21, 5)])]
# batches: one wave of the select block, the 64 / 65 and 1024 / 1025 edges (above 1024 the select and the mean are two launches)
SHIFT_CASES += [_case(SHIFT, 8, 1, B, 200 + B, upstream=0.5) for B in (1, 63, 64, 65, 128, 1024, 1025, 1100)]
SHIFT_CASES += [_case(SHIFT, 12, 2, 4, 300 + d, bit_depth=d) for d in (8, 14)]
SHIFT_ARGS_DIFFER = _case(SHIFT, 12, 2, 6, 310, kind="unrelated")
SHIFT_EXACT = [_case(SHIFT, 12, 2, 2, 320, kind="exact", mask="full"), _case(SHIFT, 16, 0, 2, 321, kind="exact", mask="full")]
# (seeds: about half of them put a sample's minimum on a mirror pair; these do so for every sample, for L1 and L2 alike -- asserted on the host)
SHIFT_TIES = [_case(SHIFT, 14, 3, 2, 25, kind="tie_lr", mask="full"), _case(SHIFT, 14, 3, 2, 29, kind="tie_lr", mask="full", upstream=2.0)]
SHIFT_EMPTY = [_case(SHIFT, 12, 2, 3, 330, mask="row0"), _case(SHIFT, 12, 2, 4, 331, mask="none1"),
               _case(SHIFT, 8, 1, 1025, 332, mask="none1")]
SHIFT_CASES += [SHIFT_ARGS_DIFFER] + SHIFT_EXACT + SHIFT_TIES + SHIFT_EMPTY

# ---- sobel_l1_mix -----------------------------------------------------------------------------------------------------------------
# crops L = 3 (both mirror folds hit row 1), 4 (adjacent rows), 5, 16, 17 at border 1; the shipped patch sizes 16, 24, 32 (S = 48, 72, 96);
# one shift; 81 shifts
EDGE_CASES = [_case(EDGE, L + 2, 1, 3, 400 + L) for L in (3, 4, 5, 16, 17)]
EDGE_CASES += [_case(EDGE, 48, 3, 3, 448, mask="cloud"), _case(EDGE, 72, 3, 2, 472, mask="cloud"), _case(EDGE, 96, 3, 2, 497, mask="cloud"),
               _case(EDGE, 12, 0, 3, 412), _case(EDGE, 20, 4, 3, 420, upstream=1.7)]
EDGE_CASES += [_case(EDGE, 7, 1, B, 500 + B) for B in (1, 65, 130)]
EDGE_CASES += [_case(EDGE, 12, 2, 3, 520, pi=0.0), _case(EDGE, 12, 2, 3, 521, pi=1.0)]
EDGE_CASES += [_case(EDGE, 102, 1, 1, 540)]                      # L = 100, the limit: the backward's LDS block is 161 616 of 163 840 bytes
EDGE_TIES = [_case(EDGE, 14, 3, 2, 25, kind="tie_lr", mask="full")]
EDGE_EMPTY = [_case(EDGE, 12, 2, 3, 530, mask="none1")]
EDGE_CASES += EDGE_TIES + EDGE_EMPTY

# ---- l1msssim ---------------------------------------------------------------------------------------------------------------------
# crops L = 2, 3, 7 at border 1; S = 48, 72, 96; one shift; 81 and 121 shifts (the select kernel's 64 lanes take a second lap)
REVSSIM_CASES = [_case(REVSSIM, L + 2, 1, 3, 600 + L, kind="faint") for L in (2, 3, 7)]
REVSSIM_CASES += [_case(REVSSIM, 48, 3, 3, 648, mask="cloud"), _case(REVSSIM, 48, 3, 3, 649, kind="faint", mask="cloud"),
                  _case(REVSSIM, 72, 3, 2, 672, mask="cloud"), _case(REVSSIM, 96, 3, 2, 696, kind="faint", mask="cloud"),
                  _case(REVSSIM, 12, 0, 3, 612, kind="faint"), _case(REVSSIM, 20, 4, 3, 620, upstream=1.7),
                  _case(REVSSIM, 21, 5, 2, 621, kind="faint")]
REVSSIM_CASES += [_case(REVSSIM, 9, 1, B, 700 + B, kind="faint") for B in (1, 2, 5, 33)]
REVSSIM_CASES += [_case(REVSSIM, 12, 2, 3, 720, kind="faint", eta=0.0), _case(REVSSIM, 12, 2, 3, 721, kind="faint", eta=1.0)]
REVSSIM_CASES += [_case(REVSSIM, 12, 2, 3, 730 + d, kind="faint", bit_depth=d) for d in (8, 14)]
REVSSIM_CASES += [_case(REVSSIM, 142, 1, 1, 760, kind="faint")]   # L = 140, the limit: 162 400 bytes
REVSSIM_TIES = [_case(REVSSIM, 20, 4, 3, 740, kind="tie_cols", mask="full")]
REVSSIM_EMPTY = [_case(REVSSIM, 12, 2, 3, 750, mask="none1")]
REVSSIM_CASES += REVSSIM_TIES + REVSSIM_EMPTY

ALL_CASES = SHIFT_CASES + EDGE_CASES + REVSSIM_CASES
assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)



def ids(cases):
    return [c["id"] for c in cases]


def by_id(cid):
    return next(c for c in ALL_CASES if c["id"] == cid)


def oracle_gradients(case, hr, mask, pred):
    """{name: (arg, gradient [B,S,S,1])} of the winning shifts, closed form."""
    b, up = case["border"], case["upstream"]
    if case["loss"] == SHIFT:
        r = on.shift_per_sample(hr, mask, pred, b, case["bit_depth"])
        return {"l1": (r["arg_l1"], on.shift_grad_at(hr, mask, pred, r["arg_l1"], b, 1, up)),
                "l2": (r["arg_l2"], on.shift_grad_at(hr, mask, pred, r["arg_l2"], b, 2, up))}
    if case["loss"] == EDGE:
        pi = float(np.float32(case["pi"]))
        _, arg = on.select_min(on.shift_l1edge_table(hr, mask, pred, b, pi))
        return {"edge": (arg, on.shift_l1edge_grad_at(hr, mask, pred, arg, b, pi, up))}
    eta = float(np.float32(case["eta"]))
    _, arg = on.select_min(on.shift_revssim_table(hr, mask, pred, b, case["bit_depth"], eta))
    return {"revssim": (arg, on.shift_revssim_grad_at(hr, mask, pred, arg, b, case["bit_depth"], eta, up))}
