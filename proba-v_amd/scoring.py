"""Scoring of super-resolved images by the ESA PROBA-V measure (evaluate.py; the reference's evaluate.py:76-87 left it unfinished).

The metric, per image.  SR: uint16 prediction S x S; HR: uint16 ground truth S x S; M: clear mask of HR (nonzero = clear; SM.png, i.e.
``~mask`` of resolverDir/TRAINimgHR_<band>.npy); border b = 3.  L = S - 2b, P = SR[b:b+L, b:b+L].  For every shift (u, v) in [0, 2b]^2,
row-major::

    d = HR[u:u+L, v:v+L] - P  (integers)        m = M[u:u+L, v:v+L]
    n = sum m      s1 = sum m d      s2 = sum m d^2                       (exact integers)
    cMSE(u, v) = (n s2 - s1^2) / n^2                                      (bias s1 / n folded in; raw 16-bit units)
    cPSNR = 10 log10(65535^2 / min cMSE)                                  shift = the first (u, v) attaining the minimum

A shift with n = 0 is skipped; an image where every shift has n = 0 gets NaN (reported, never averaged); cMSE = 0 gives +inf, whose
score term is 0.  The score of a set of images is mean(N_i / cPSNR_i), N_i the baseline cPSNR of image set i from the download's
norm.csv; lower is better.  This is the ESA / HighRes-net shift_cPSNR (HR normalised by 2^16 - 1, Losses.numBytes).  It differs from
Losses.shiftCompensatedcPSNR (models/loss.py:37-53), which the reference's evaluate.py calls, only in that HR is masked too:
``formula="reference"`` computes that one instead.

Ids.  Image sets are named imgsetNNNN.  Train ids below 594 are RED, 594 .. 1159 NIR (inference.FIRST_ID); ids from 1160 are test sets and
have no HR.  The HR row of a train id is id - first id of its band: TRAINimgHR_<band>.npy holds every set of the band, the ones
dataGenerator.py removed included.  Images are matched to HR by id, never by position.

cSSIM, the shift-compensated SSIM published beside the cPSNR, is stated further down (gauss11, cssim_table_numpy, shift_cssim); it is
computed only when asked for (score_images(..., metrics=("cpsnr", "cssim")), evaluate.py --metrics cpsnr,cssim).
"""
import csv
import glob
import json
import math
import os
import re

import numpy as np
import torch

from . import _lib, ops       # noqa: F401  (ops registers torch.ops.probav.*)
from .inference import FIRST_ID

FIRST_TRAIN_ID = {b: FIRST_ID[("TRAIN", b)] for b in ("RED", "NIR")}
FIRST_TEST_ID = FIRST_ID[("TEST", "RED")]
BANDS = ("RED", "NIR")
MAX_PER_LAUNCH = 4096                                     # images per launch (the C ABI takes up to 65535)


def band_of(img_id):
    """'RED' / 'NIR' for a train id, None for a test id (>= 1160: no HR)."""
    if img_id < 0:
        raise ValueError("negative image set id %d" % img_id)
    if img_id >= FIRST_TEST_ID:
        return None
    return "NIR" if img_id >= FIRST_TRAIN_ID["NIR"] else "RED"


def hr_index(img_id):
    """Row of TRAINimgHR_<band>.npy that holds the HR of train id `img_id` (id - first id of its band)."""
    band = band_of(img_id)
    if band is None:
        raise ValueError("imgset%04d is a test set: it has no HR" % img_id)
    return img_id - FIRST_TRAIN_ID[band]


def read_removed(band, directory="."):
    """The ids dataGenerator.py removed from a band (removedTrainSets<BAND>.txt, read as test.py reads it); [] if the file is absent."""
    path = os.path.join(directory, "removedTrainSets%s.txt" % band.upper())
    if not os.path.exists(path):
        return []
    with open(path) as fh:
        return [int(float(line.split("\n")[0])) for line in fh.readlines() if line.strip()]


def read_norm(path):
    """norm.csv of the ESA download -> {id: baseline cPSNR}: one ``imgsetNNNN <value>`` per line, separated by whitespace or a comma."""
    out = {}
    with open(path) as fh:
        for k, line in enumerate(fh, 1):
            txt = line.strip()
            if not txt:
                continue
            parts = [p for p in re.split(r"[\s,]+", txt) if p]
            m = re.fullmatch(r"imgset(\d+)", parts[0]) if len(parts) == 2 else None
            if m is None:
                raise ValueError("%s:%d: expected 'imgsetNNNN <value>', got %r" % (path, k, txt))
            out[int(m.group(1))] = float(parts[1])
    return out


def score(cpsnr, norm):
    """mean(N_i / cPSNR_i) over the images of `cpsnr` ({id: cPSNR}); +inf contributes 0, NaN images are left out.  None when `norm` is
    None, when an image has no baseline, or when nothing finite is left."""
    if norm is None:
        return None
    terms = []
    for i, c in cpsnr.items():
        if c is None or math.isnan(c):
            continue
        if i not in norm:
            return None
        terms.append(0.0 if math.isinf(c) else norm[i] / c)
    return float(np.mean(terms)) if terms else None


def _to_device_u16(a, dev):
    if isinstance(a, torch.Tensor):
        if a.dtype in (torch.uint16, torch.int16):
            return a.to(dev)
        raise ValueError("image tensors must be uint16 (or int16 bits), got %s" % a.dtype)
    a = np.asarray(a)
    if a.dtype != np.uint16:
        if not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > 65535)):
            raise ValueError("images must be uint16 (or integers in 0..65535), got %s" % a.dtype)
        a = a.astype(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(torch.uint16)


def _to_device_mask(m, dev):
    if isinstance(m, torch.Tensor):
        return (m if m.dtype == torch.bool else m != 0).to(dev)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(m) != 0)).to(dev)


def shift_cpsnr(sr, hr, mask, border=3, formula="esa", device=None):
    """cPSNR of every image: sr, hr [N, S, S] (uint16 numpy arrays or tensors), mask [N, S, S] (nonzero = clear pixel of HR).

    formula="esa" (default): the metric of this module's docstring, on the device (torch.ops.probav.esa_shift_cpsnr) ->
    dict(cpsnr f64[N], shift i32[N, 2], bias f64[N], n_clear i64[N]) of numpy arrays.
    formula="reference": Losses(targetShape=(S, S, 1)).shiftCompensatedcPSNR -- HR unmasked, what the reference's evaluate.py computes
    -> dict(cpsnr f64[N]) (its float32 values), the other keys None."""
    if formula not in ("esa", "reference"):
        raise ValueError("formula must be 'esa' or 'reference', got %r" % (formula,))
    if device is None:
        if not torch.cuda.is_available():
            for t, name in ((sr, "sr"), (hr, "hr"), (mask, "mask")):
                if isinstance(t, torch.Tensor):
                    _lib.require_device(t, name)
            raise RuntimeError("shift_cpsnr needs a HIP device: the scoring kernels run only on a gfx950 device (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    for t, name in ((sr, "sr"), (hr, "hr"), (mask, "mask")):
        if isinstance(t, torch.Tensor):
            _lib.require_device(t, name)
    if tuple(sr.shape) != tuple(hr.shape) or tuple(mask.shape) != tuple(sr.shape) or len(sr.shape) != 3 or sr.shape[1] != sr.shape[2]:
        raise ValueError("sr, hr, mask must all be [N, S, S]; got %s %s %s" % (tuple(sr.shape), tuple(hr.shape), tuple(mask.shape)))
    N, S = sr.shape[0], sr.shape[1]
    if formula == "reference":
        from .loss import Losses
        losses = Losses(targetShape=(S, S, 1), cropBorder=border)
        out = []
        for i in range(0, N, MAX_PER_LAUNCH):
            as_float = lambda t: (t.view(torch.int16).to(torch.int32) & 0xFFFF).float()[..., None]      # uint16 bits -> exact fp32
            s = as_float(_to_device_u16(sr[i:i + MAX_PER_LAUNCH], device))
            h = as_float(_to_device_u16(hr[i:i + MAX_PER_LAUNCH], device))
            m = _to_device_mask(mask[i:i + MAX_PER_LAUNCH], device)[..., None]
            out.append(losses.shiftCompensatedcPSNR(h, m, s).double().cpu())
        c = torch.cat(out).numpy() if out else np.zeros(0)
        return {"cpsnr": c, "shift": None, "bias": None, "n_clear": None}
    parts = {"cpsnr": [], "shift": [], "bias": [], "n_clear": []}
    for i in range(0, N, MAX_PER_LAUNCH):
        res = torch.ops.probav.esa_shift_cpsnr(_to_device_u16(sr[i:i + MAX_PER_LAUNCH], device), _to_device_u16(hr[i:i + MAX_PER_LAUNCH], device),
                                               _to_device_mask(mask[i:i + MAX_PER_LAUNCH], device), int(border))
        for k, t in zip(("cpsnr", "shift", "bias", "n_clear"), res):
            parts[k].append(t.cpu())
    empty = {"cpsnr": np.zeros(0), "shift": np.zeros((0, 2), np.int32), "bias": np.zeros(0), "n_clear": np.zeros(0, np.int64)}
    return {k: (torch.cat(v).numpy() if v else empty[k]) for k, v in parts.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# cSSIM: the shift-compensated SSIM published beside the cPSNR (DeepSUM, HighRes-net, RAMS, ...).  Images, mask, border, L, P and the
# shift order as in the module docstring; for every shift (u, v), all in fp64::
#
#     H = HR[u:u+L, v:v+L]      m = M[u:u+L, v:v+L] as 0/1      n = sum m      s1 = sum m (H - P)      bias = s1 / n
#     x = m (P + bias)          y = m H                         (masked pixels are zero on BOTH sides, as the published implementations do)
#     F(a)[i, j] = sum_{p, q} g[p] g[q] a[i+p, j+q], g = gauss11(), "valid": K x K outputs, K = L - 10
#     mx = F(x)  my = F(y)  vx = F(x x) - mx^2  vy = F(y y) - my^2  cxy = F(x y) - mx my     C1 = (0.01 * 65535)^2   C2 = (0.03 * 65535)^2
#     ssim(u, v) = mean over the K^2 windows of ((2 mx my + C1)(2 cxy + C2)) / ((mx^2 + my^2 + C1)(vx + vy + C2))
#     cSSIM = max over the shifts with n > 0, shift_ssim = the FIRST (u, v) attaining it
#
# A shift with n = 0 has the value NaN; every shift n = 0: cSSIM = NaN, shift (-1, -1).  A window that sees only masked pixels
# contributes exactly 1 (that is what the published numbers contain).  L >= 11 is required.  Because m is 0/1 everything follows from six
# filtered maps (the folded form, what the kernel and cssim_table_numpy compute):
#     mx = F(mP) + bias F(m)     F(xx) = F(mP^2) + bias (2 F(mP) + bias F(m))     F(xy) = F(mPH) + bias F(mH)     my = F(mH)     F(yy) = F(mH^2)
# ---------------------------------------------------------------------------------------------------------------------------------
SSIM_TAPS = 11
SSIM_C1, SSIM_C2 = (0.01 * 65535.0) ** 2, (0.03 * 65535.0) ** 2
METRICS = ("cpsnr", "cssim")


def gauss11():
    """The 11 taps of the SSIM window: exp(-(j - 5)^2 / (2 * 1.5^2)), j = 0..10, divided by their sum (numpy fp64)."""
    j = np.arange(SSIM_TAPS, dtype=np.float64)
    g = np.exp(-(j - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _check_ssim_shape(shape, border, what):
    if len(shape) != 3 or shape[1] != shape[2]:
        raise ValueError("%s: sr, hr, mask must all be [N, S, S]; got %s" % (what, tuple(shape)))
    if not 0 <= border <= 3:
        raise ValueError("%s: border must be in 0..3, got %d" % (what, border))
    if shape[1] - 2 * border < SSIM_TAPS:
        raise ValueError("%s: the 11-tap SSIM window needs a crop of at least 11 rows: S >= 2 border + 11 = %d, got S = %d"
                         % (what, 2 * border + SSIM_TAPS, shape[1]))


def _filter11(a, g):
    """F of the definition on the last two axes: the row pass (along a row) first, then the column pass, taps in index order."""
    k = a.shape[-1] - SSIM_TAPS + 1
    rows = g[0] * a[..., :, 0:k]
    for q in range(1, SSIM_TAPS):
        rows = rows + g[q] * a[..., :, q:q + k]
    k = a.shape[-2] - SSIM_TAPS + 1
    out = g[0] * rows[..., 0:k, :]
    for p in range(1, SSIM_TAPS):
        out = out + g[p] * rows[..., p:p + k, :]
    return out


def cssim_table_numpy(sr, hr, mask, border):
    """The fp64 statement the kernel is held to: ssim(u, v) of every image and shift -> f64 [N, (2b+1)^2], NaN where n = 0.  The folded
    form; F(m), F(mH), F(mH^2) of a shift are read as windows at (u, v) of one filtered map of the whole image (the same arithmetic per
    element as filtering the crop, so the same bits)."""
    sr, hr = np.asarray(sr), np.asarray(hr)
    m_all = (np.asarray(mask) != 0)
    if sr.shape != hr.shape or m_all.shape != sr.shape:
        raise ValueError("cssim_table_numpy: sr, hr, mask must all be [N, S, S]; got %s %s %s" % (sr.shape, hr.shape, m_all.shape))
    _check_ssim_shape(sr.shape, border, "cssim_table_numpy")
    N, S = sr.shape[0], sr.shape[1]
    ns, L = 2 * border + 1, S - 2 * border
    K = L - SSIM_TAPS + 1
    g = gauss11()
    table = np.full((N, ns * ns), np.nan)
    for i in range(N):
        Mi = m_all[i].astype(np.int64)
        Hi = hr[i].astype(np.int64)
        P = sr[i, border:border + L, border:border + L].astype(np.int64)
        Md, Hd, Pd = Mi.astype(np.float64), Hi.astype(np.float64), P.astype(np.float64)
        full = _filter11(np.stack([Md, Md * Hd, Md * Hd * Hd]), g)                  # [3, S - 10, S - 10]
        for u in range(ns):
            for v in range(ns):
                m = Mi[u:u + L, v:v + L]
                n = int(m.sum())
                if n == 0:
                    continue
                s1 = int((m * (Hi[u:u + L, v:v + L] - P)).sum())
                bias = np.float64(s1) / np.float64(n)
                md, hd = Md[u:u + L, v:v + L], Hd[u:u + L, v:v + L]
                mP = md * Pd
                f1, f3, f5 = _filter11(np.stack([mP, mP * Pd, mP * hd]), g)
                f0, f2, f4 = full[:, u:u + K, v:v + K]
                mx, my = f1 + bias * f0, f2
                fxx = f3 + bias * (2.0 * f1 + bias * f0)
                fxy = f5 + bias * f2
                vx, vy, cxy = fxx - mx * mx, f4 - my * my, fxy - mx * my
                term = ((2.0 * mx * my + SSIM_C1) * (2.0 * cxy + SSIM_C2)) / ((mx * mx + my * my + SSIM_C1) * (vx + vy + SSIM_C2))
                table[i, u * ns + v] = term.sum() / (float(K) * float(K))
    return table


def cssim_select_numpy(table, border):
    """(cssim f64[N], shift i32[N, 2]) of a table: the largest entry that is not NaN and the FIRST shift attaining it; all NaN: NaN, (-1, -1)."""
    table = np.asarray(table, np.float64)
    ns = 2 * border + 1
    cssim = np.full(table.shape[0], np.nan)
    shift = np.full((table.shape[0], 2), -1, np.int32)
    for i, row in enumerate(table):
        ok = ~np.isnan(row)
        if ok.any():
            k = int(np.argmax(np.where(ok, row, -np.inf)))                           # argmax returns the first maximum
            cssim[i], shift[i] = row[k], (k // ns, k % ns)
    return cssim, shift


def shift_cssim(sr, hr, mask, border=3, device=None):
    """cSSIM of every image, on the device (torch.ops.probav.esa_shift_ssim_table, then the first maximum by probav_ssim_select): sr, hr,
    mask as shift_cpsnr takes them -> dict(cssim f64[N], shift i32[N, 2], table f64[N, (2b+1)^2]) of numpy arrays."""
    if device is None:
        if not torch.cuda.is_available():
            for t, name in ((sr, "sr"), (hr, "hr"), (mask, "mask")):
                if isinstance(t, torch.Tensor):
                    _lib.require_device(t, name)
            raise RuntimeError("shift_cssim needs a HIP device: the scoring kernels run only on a gfx950 device (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    for t, name in ((sr, "sr"), (hr, "hr"), (mask, "mask")):
        if isinstance(t, torch.Tensor):
            _lib.require_device(t, name)
    if tuple(sr.shape) != tuple(hr.shape) or tuple(mask.shape) != tuple(sr.shape):
        raise ValueError("sr, hr, mask must all be [N, S, S]; got %s %s %s" % (tuple(sr.shape), tuple(hr.shape), tuple(mask.shape)))
    _check_ssim_shape(tuple(sr.shape), border, "shift_cssim")
    N, ns = sr.shape[0], 2 * border + 1
    parts = {"cssim": [], "shift": [], "table": []}
    for i in range(0, N, MAX_PER_LAUNCH):
        table = torch.ops.probav.esa_shift_ssim_table(_to_device_u16(sr[i:i + MAX_PER_LAUNCH], device), _to_device_u16(hr[i:i + MAX_PER_LAUNCH], device),
                                                      _to_device_mask(mask[i:i + MAX_PER_LAUNCH], device), int(border))
        n = table.shape[0]
        cssim = torch.empty(n, dtype=torch.float64, device=table.device)
        shift = torch.empty((n, 2), dtype=torch.int32, device=table.device)
        with torch.cuda.device(table.device):
            _lib.check(_lib.lib().probav_ssim_select(_lib.ptr(table), n, int(border), _lib.ptr(cssim), _lib.ptr(shift), _lib.current_stream()),
                       "probav_ssim_select")
        for k, t in zip(("cssim", "shift", "table"), (cssim, shift, table)):
            parts[k].append(t.cpu())
    empty = {"cssim": np.zeros(0), "shift": np.zeros((0, 2), np.int32), "table": np.zeros((0, ns * ns))}
    return {k: (torch.cat(v).numpy() if v else empty[k]) for k, v in parts.items()}


def check_metrics(metrics):
    """("cpsnr",) or ("cpsnr", "cssim") as a tuple; anything else is a ValueError that names the offender."""
    metrics = tuple(metrics)
    for name in metrics:
        if name not in METRICS:
            raise ValueError("unknown metric %r (known: %s)" % (name, ", ".join(METRICS)))
    if "cpsnr" not in metrics or len(set(metrics)) != len(metrics):
        raise ValueError("metrics must be cpsnr or cpsnr,cssim; got %r" % (",".join(metrics),))
    return metrics


def load_hr(config, band):
    """resolverDir/TRAINimgHR_<band>.npy -> (hr uint16 [n, S, S], clear bool [n, S, S]); row k is train id FIRST_TRAIN_ID[band] + k."""
    path = os.path.join(config["preprocessing_out"], "resolverDir", "TRAINimgHR_%s.npy" % band.upper())
    a = np.load(path, allow_pickle=True)
    data, masked = np.ma.getdata(a), np.ma.getmaskarray(a)
    if data.ndim < 3 or any(n != 1 for n in data.shape[1:-2]):
        raise ValueError("%s: expected [sets, (1, ...,) S, S], got %s" % (path, data.shape))
    shape = (data.shape[0],) + data.shape[-2:]                 # [sets, 1, 1, S, S] as dataGenerator.py dumps it, or [sets, 1, S, S]
    data, masked = data.reshape(shape), masked.reshape(shape)
    if data.dtype != np.uint16:
        if np.any(data != np.rint(data)) or data.min() < 0 or data.max() > 65535:
            raise ValueError("%s: HR values are not 16-bit integers" % path)
        data = data.astype(np.uint16)
    return np.ascontiguousarray(data), np.ascontiguousarray(~masked)


def load_sr_dir(path):
    """Every imgsetNNNN.png of a folder -> {id: uint16 [S, S]} (by file name; other files are ignored)."""
    from .pngio import imread
    out = {}
    for p in sorted(glob.glob(os.path.join(path, "imgset*.png"))):
        m = re.fullmatch(r"imgset(\d+)\.png", os.path.basename(p))
        if m:
            a = imread(p)
            if a.ndim != 2 or a.dtype not in (np.uint16, np.uint8):
                raise ValueError("%s: greyscale 8/16-bit PNG expected" % p)
            out[int(m.group(1))] = a.astype(np.uint16)
    return out


def score_images(images, hr_by_band, border=3, formula="esa", removed=None, metrics=("cpsnr",)):
    """Score {id: SR image} against {band: (hr, clear)}.  Returns (rows, counts): rows = list of dicts (id, band, cpsnr, u, v, bias,
    n_clear) in id order; counts = scored / skipped (test ids, bands not loaded) / missing (HR sets with no image, removed ids
    excepted) / removed.  With "cssim" in `metrics` every row also has cssim, su, sv (the cSSIM and its own best shift) and
    cssim_at_cpsnr_shift (the SSIM table's entry at the row's (u, v): NaN when there is none); `formula` does not affect them."""
    removed = removed or {}
    metrics = check_metrics(metrics)
    rows, skipped = [], 0
    by_band = {b: [] for b in hr_by_band}
    for i in sorted(images):
        b = band_of(i)
        if b is None or b not in hr_by_band:
            skipped += 1
            continue
        if hr_index(i) >= len(hr_by_band[b][0]):
            raise ValueError("imgset%04d: %s HR holds only %d sets" % (i, b, len(hr_by_band[b][0])))
        by_band[b].append(i)
    missing = 0
    for b, (hr, _) in hr_by_band.items():
        have = set(by_band[b])
        gone = set(removed.get(b, ()))
        missing += sum(1 for k in range(len(hr)) if FIRST_TRAIN_ID[b] + k not in have and FIRST_TRAIN_ID[b] + k not in gone)
    for b, ids in by_band.items():
        if not ids:
            continue
        hr, clear = hr_by_band[b]
        idx = [hr_index(i) for i in ids]
        res = shift_cpsnr(np.stack([images[i] for i in ids]), hr[idx], clear[idx], border=border, formula=formula)
        for k, i in enumerate(ids):
            rows.append({"id": i, "band": b, "cpsnr": float(res["cpsnr"][k]),
                         "u": None if res["shift"] is None else int(res["shift"][k, 0]),
                         "v": None if res["shift"] is None else int(res["shift"][k, 1]),
                         "bias": None if res["bias"] is None else float(res["bias"][k]),
                         "n_clear": None if res["n_clear"] is None else int(res["n_clear"][k])})
        if "cssim" in metrics:
            ssim = shift_cssim(np.stack([images[i] for i in ids]), hr[idx], clear[idx], border=border)
            ns = 2 * border + 1
            for k, r in enumerate(rows[-len(ids):]):
                at = r["u"] is not None and r["u"] >= 0
                r.update({"cssim": float(ssim["cssim"][k]), "su": int(ssim["shift"][k, 0]), "sv": int(ssim["shift"][k, 1]),
                          "cssim_at_cpsnr_shift": float(ssim["table"][k, r["u"] * ns + r["v"]]) if at else math.nan})
    rows.sort(key=lambda r: r["id"])
    counts = {"scored": len(rows), "skipped": skipped, "missing": missing, "removed": sum(len(v) for v in removed.values())}
    return rows, counts


def _finite_mean(vals):
    f = [v for v in vals if not (math.isnan(v) or math.isinf(v))]
    return float(np.mean(f)) if f else None


def summarize(rows, counts, norm=None, bench_rows=None, metrics=("cpsnr",)):
    """The JSON summary evaluate.py prints: counts, mean cPSNR (finite values) and score per band and overall, NaN / +inf counts, and
    against a benchmark (rows of the same ids): wins / losses / ties and the mean and median of candidate - benchmark cPSNR.  With
    "cssim" in `metrics`: mean_cssim, mean_cssim_at_cpsnr_shift (finite values) and cssim_nan per band and overall, and against a
    benchmark the mean and median of candidate - benchmark cSSIM (norm.csv has no SSIM counterpart: there is no cSSIM score)."""
    metrics = check_metrics(metrics)
    out = dict(counts)
    for name, sel in [("overall", rows)] + [(b, [r for r in rows if r["band"] == b]) for b in BANDS]:
        c = [r["cpsnr"] for r in sel]
        out[name] = {"images": len(sel), "mean_cpsnr": _finite_mean(c), "nan": sum(1 for v in c if math.isnan(v)),
                     "inf": sum(1 for v in c if math.isinf(v) and v > 0),
                     "score": score({r["id"]: r["cpsnr"] for r in sel}, norm) if sel else None}
        if "cssim" in metrics:
            out[name].update({"mean_cssim": _finite_mean([r["cssim"] for r in sel]),
                              "mean_cssim_at_cpsnr_shift": _finite_mean([r["cssim_at_cpsnr_shift"] for r in sel]),
                              "cssim_nan": sum(1 for r in sel if math.isnan(r["cssim"]))})
    if bench_rows is not None:
        bench = {r["id"]: r["cpsnr"] for r in bench_rows}
        pairs = [(r["cpsnr"], bench[r["id"]]) for r in rows if r["id"] in bench and not math.isnan(r["cpsnr"]) and not math.isnan(bench[r["id"]])]
        delta = [a - b for a, b in pairs if not (math.isinf(a) or math.isinf(b))]
        out["benchmark"] = {"compared": len(pairs), "wins": sum(1 for a, b in pairs if a > b), "losses": sum(1 for a, b in pairs if a < b),
                            "ties": sum(1 for a, b in pairs if a == b), "mean_delta_cpsnr": float(np.mean(delta)) if delta else None,
                            "median_delta_cpsnr": float(np.median(delta)) if delta else None}
        if "cssim" in metrics:
            bs = {r["id"]: r["cssim"] for r in bench_rows if "cssim" in r}
            ds = [r["cssim"] - bs[r["id"]] for r in rows if r["id"] in bs and not math.isnan(r["cssim"]) and not math.isnan(bs[r["id"]])]
            out["benchmark"].update({"mean_delta_cssim": float(np.mean(ds)) if ds else None,
                                     "median_delta_cssim": float(np.median(ds)) if ds else None})
    return out


CSV_FIELDS = ("id", "band", "cpsnr", "u", "v", "bias", "n_clear", "norm", "benchmark_cpsnr")


CSV_FIELDS_SSIM = CSV_FIELDS + ("cssim", "su", "sv", "cssim_at_cpsnr_shift", "benchmark_cssim")      # only when cSSIM was computed


def write_csv(path, rows, norm=None, bench_rows=None, metrics=("cpsnr",)):
    """scores.csv: one line per scored image, CSV_FIELDS (empty where a value does not apply); cPSNR with 17 significant digits.  With
    "cssim" in `metrics` the columns are CSV_FIELDS_SSIM."""
    with_ssim = "cssim" in check_metrics(metrics)
    bench = {r["id"]: r["cpsnr"] for r in bench_rows} if bench_rows is not None else {}
    bench_ssim = {r["id"]: r.get("cssim") for r in bench_rows} if bench_rows is not None else {}
    fmt = lambda v: "" if v is None else (repr(float(v)) if isinstance(v, float) else str(v))
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(CSV_FIELDS_SSIM if with_ssim else CSV_FIELDS)
        for r in rows:
            line = ["imgset%04d" % r["id"], r["band"], fmt(r["cpsnr"]), fmt(r["u"]), fmt(r["v"]), fmt(r["bias"]), fmt(r["n_clear"]),
                    fmt(None if norm is None else norm.get(r["id"])), fmt(bench.get(r["id"]))]
            if with_ssim:
                line += [fmt(r["cssim"]), fmt(r["su"]), fmt(r["sv"]), fmt(r["cssim_at_cpsnr_shift"]), fmt(bench_ssim.get(r["id"]))]
            w.writerow(line)


def json_line(summary):
    """One JSON line; NaN / inf (not JSON) become null."""
    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, float) and (math.isnan(v) or math.isinf(v)):
            return None
        return v
    return json.dumps(clean(summary), sort_keys=False)


def plot_comparison(path, rows, bench_rows):
    """The reference's scatter (evaluate.py:53-72): candidate against benchmark cPSNR, RED and NIR panels, 20-70 dB, identity line.
    Returns False (and writes nothing) when matplotlib does not import."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    bench = {r["id"]: r["cpsnr"] for r in bench_rows}
    fig, axs = plt.subplots(1, 2, figsize=(10, 5))
    for ax, b, col in ((axs[0], "RED", "#cc0e74"), (axs[1], "NIR", "#916dd5")):
        pts = [(bench[r["id"]], r["cpsnr"]) for r in rows if r["band"] == b and r["id"] in bench]
        if pts:
            ax.scatter([p[0] for p in pts], [p[1] for p in pts], edgecolors="k", alpha=0.6, color=col, label=b)
        ax.set_title("%s images" % b)
        ax.grid(True)
        ax.set_xlim([20, 70])
        ax.set_ylim([20, 70])
        ax.plot([20, 70], [20, 70], "#08ffc8", zorder=1)
        ax.set_xlabel("cPSNR(dB) Benchmark")
        ax.set_ylabel("cPSNR(dB) Candidate")
    fig.tight_layout()
    fig.savefig(path, dpi=100)
    plt.close(fig)
    return True
