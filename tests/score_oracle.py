"""Exact numpy / Python-integer oracle of the ESA shift-compensated clear PSNR (proba-v_amd/scoring.py states the metric): the moments
in int64, cMSE as a Fraction, the first minimum in row-major shift order, the cPSNR from Python integers."""
import math
from fractions import Fraction

import numpy as np


def moments(sr, hr, mask, border):
    """(n, s1, s2) int64 [N, (2b+1)^2, 3] of every shift, row-major (u, v)."""
    sr, hr = np.asarray(sr, np.int64), np.asarray(hr, np.int64)
    m = (np.asarray(mask) != 0).astype(np.int64)
    N, S = sr.shape[0], sr.shape[1]
    L, ns = S - 2 * border, 2 * border + 1
    P = sr[:, border:border + L, border:border + L]
    out = np.zeros((N, ns * ns, 3), np.int64)
    for u in range(ns):
        for v in range(ns):
            d = hr[:, u:u + L, v:v + L] - P
            mm = m[:, u:u + L, v:v + L]
            out[:, u * ns + v] = np.stack([mm.sum((1, 2)), (mm * d).sum((1, 2)), (mm * d * d).sum((1, 2))], 1)
    return out


def select(mom):
    """-> list of dicts (cpsnr, shift, bias, n_clear, cmse Fraction) from exact moments [N, nshift, 3]."""
    ns = int(round(math.sqrt(mom.shape[1])))
    res = []
    for img in mom:
        best, bc = None, None
        for k, (n, s1, s2) in enumerate(img.tolist()):
            if n == 0:
                continue
            c = Fraction(n * s2 - s1 * s1, n * n)
            if bc is None or c < bc:
                best, bc = k, c
        if best is None:
            res.append({"cpsnr": math.nan, "shift": (-1, -1), "bias": math.nan, "n_clear": 0, "cmse": None})
            continue
        n, s1, _ = img[best].tolist()
        num = bc.numerator
        cp = math.inf if num == 0 else 10.0 * (math.log10(65535 ** 2 * bc.denominator) - math.log10(num))
        res.append({"cpsnr": cp, "shift": (best // ns, best % ns), "bias": s1 / n, "n_clear": n, "cmse": bc})
    return res


def shift_cpsnr(sr, hr, mask, border=3):
    return select(moments(sr, hr, mask, border))
