"""Dataset builder: the reference's utils/dataGenerator.py (lines 33-273 and the helpers they call) on the GPU.

Same function names, argument orders, directory layout, file names, shapes, dtypes and pickle protocols as the reference.  The clear
counts of the raw frames, the registration of every LR frame against its set's clearest frame and the pad + unfold of the patches run
as HIP kernels (csrc/kernels_prep.hip, behind include/probav_hip.h); the selections in between are numpy index bookkeeping over small
count arrays, written with the SAME numpy calls on the same dtypes and shapes as the reference (its `np.argsort` is the default,
unstable kind: tie order then depends on the numpy build exactly as the reference's does).

Deliberate differences ('From the ESA download to train.py'):
  - stage 1 writes ragged image sets as object arrays of per-set arrays (numpy >= 1.24 refuses the reference's implicit ragged arrays);
  - registration takes the argmax of the EXACT integer cross-correlation (the reference's fp64 FFT agrees except where two shifts tie
    exactly, which it breaks by rounding noise) and rolls exactly (the reference's Fourier shift leaves ~1e-12 residue);
  - masks are booleans: a nonzero QM / SM pixel is clear;
  - randomness is drawn from the `rng` that main() threads through (a numpy.random.RandomState; None = numpy's global state, as the
    reference), in the reference's call order;
  - splitPatches restates sklearn's train_test_split(test_size=split, random_state=17) without sklearn;
  - registerFrame(tech='time'), the reference's cloud-aware registration (utils/dataGenerator.py:663-666), is a masked normalised
    correlation over a bounded window of integer shifts with a shift that does not wrap: `register_masked_numpy` is its statement,
    csrc/kernels_prep_masked.hip the kernel that equals it bit for bit.  Selected by registerImages(tech='time') /
    main(register='masked'); the default ('freq') is the plain path above, unchanged;
  - registerImages(refine=RefineSpec(...)) / main(refine=...) take temporal outliers and saturated pixels of the registered frames out of
    their masks before anything is selected -- the counterpart of nothing in the reference.  `refine_masks_numpy` is the statement,
    csrc/kernels_refine.hip the kernels that equal it bit for bit.  Off by default (refine=None): the masks as the quality masks give them.
"""
import dataclasses
import glob
import logging
import math
import os

import numpy as np

from . import pngio
from .frame_windows import MAX_POOL

LR_SIZE = 128          # registration geometry (PROBA-V LR frames)
PREP_BAD_SHIFT = -2 ** 31   # PROBAV_PREP_BAD_SHIFT
MASKED_MAX_WINDOW = 32      # largest window of the masked registration (csrc/kernels_prep_masked.hip)
PREP_BAD_COUNT = -1          # PROBAV_PREP_BAD_COUNT
REFINE_MAX_K16, REFINE_MAX_DILATE = 1024, 3   # the mask refinement's ranges (csrc/kernels_refine.hip); its longest set is frame_windows.MAX_POOL
REGISTER_TECHS = ('freq', 'time')                        # registerFrame's `tech`, the reference's names
REGISTER_MODES = {'freq': 'freq', 'masked': 'time'}      # main()'s `register` / the CLI's --register -> tech


# ---- device helpers ----------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    from . import _lib
    _lib.lib()
    if not torch.cuda.is_available():
        raise RuntimeError("the dataset builder's registration and patch kernels run only as HIP kernels on a gfx950 device "
                           "(no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_count_nonzero(a, chunk_len):
    """count_nonzero of every consecutive chunk of `chunk_len` elements of a bool / uint8 array, on the device."""
    import torch
    from . import _lib
    dev = _dev()
    flat = np.ascontiguousarray(a).reshape(-1)
    if flat.dtype == np.bool_:
        flat = flat.view(np.uint8)
    flat = (flat != 0).view(np.uint8) if flat.dtype != np.uint8 else flat
    n = flat.size // chunk_len
    d = _to_dev(flat, dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        _lib.check(_lib.lib().probav_prep_count_nonzero(_lib.ptr(d), n, chunk_len, _lib.ptr(out), _lib.current_stream()),
                   "probav_prep_count_nonzero")
    return out.cpu().numpy()


def device_register(frames, masks, set_offsets, ref_frame):
    """frames [F,128,128] uint16, masks [F,128,128] (nonzero = clear), set_offsets [S+1], ref_frame [S] frame indices ->
    (shifts [F,2] int32, rolled frames uint16, rolled masks bool, rolled clear counts int32)."""
    import torch
    from . import _lib
    dev = _dev()
    F = frames.shape[0]
    S = len(set_offsets) - 1
    o, r = np.asarray(set_offsets, np.int64), np.asarray(ref_frame, np.int64)
    if S < 1 or o[0] != 0 or o[-1] != F or (np.diff(o) < 1).any() or len(r) != S or (r < o[:-1]).any() or (r >= o[1:]).any():
        raise ValueError("registration needs set_offsets[0] = 0, set_offsets[-1] = n_frames, no empty set, one reference inside each set")
    if frames.shape[1:] != (LR_SIZE, LR_SIZE) or masks.shape != frames.shape:
        raise ValueError("registration takes %d x %d frames, got %r / %r" % (LR_SIZE, LR_SIZE, frames.shape, masks.shape))
    fr = _to_dev(frames.astype(np.uint16, copy=False), dev)
    mk = _to_dev((np.asarray(masks) != 0).view(np.uint8), dev)
    off = _to_dev(np.asarray(set_offsets, np.int64), dev)
    ref = _to_dev(np.asarray(ref_frame, np.int32), dev)
    spec = torch.empty(S * LR_SIZE * LR_SIZE * 2, dtype=torch.float32, device=dev)
    shifts = torch.empty(F, 2, dtype=torch.int32, device=dev)
    rf = torch.empty_like(fr)
    rm = torch.empty_like(mk)
    rc = torch.empty(F, dtype=torch.int32, device=dev)
    L = _lib.lib()
    _lib.check(L.probav_prep_register(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(off), S, F, _lib.ptr(ref), _lib.ptr(spec), _lib.ptr(shifts),
                                      _lib.ptr(rf), _lib.ptr(rm), _lib.ptr(rc), _lib.current_stream()), "probav_prep_register")
    sh = shifts.cpu().numpy()
    if (sh == PREP_BAD_SHIFT).any():
        raise ValueError("probav_prep_register: set_offsets / ref_frame break the preconditions of include/probav_hip.h (empty set or a "
                         "reference outside its set)")
    return sh, rf.cpu().numpy(), rm.cpu().numpy().astype(bool), rc.cpu().numpy()


def _check_window(window):
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= MASKED_MAX_WINDOW:
        raise ValueError("masked registration takes a window of 1..%d shifts, got %r" % (MASKED_MAX_WINDOW, window))
    return int(window)


def _check_tech(tech):
    if tech not in REGISTER_TECHS:
        raise ValueError("tech must be one of %r, got %r" % (REGISTER_TECHS, tech))
    return tech


def shift_masked_numpy(img, img_clear, shift):
    """The masked registration's way of applying an integer shift s: out[p] = img[reflect(p - s)] with scipy.ndimage's 'reflect'
    (d c b a | a b c d), exact uint16; clear_out[p] = img_clear[p - s] inside the frame, False outside.  The reference's
    shift(img, s, mode='reflect') / shift(msk, s, mode='constant', cval=0) for integer s, without the spline's ringing on the mask."""
    img, clear = np.asarray(img), np.asarray(img_clear) != 0
    H, W = img.shape
    dy, dx = int(shift[0]), int(shift[1])
    if max(abs(dy), abs(dx)) >= min(H, W):
        raise ValueError("shift %r does not fit a %d x %d frame" % ((dy, dx), H, W))
    yy, xx = np.arange(H) - dy, np.arange(W) - dx
    fold = lambda i, n: np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    out = img[fold(yy, H)[:, None], fold(xx, W)[None, :]]
    inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
    return out, clear[fold(yy, H)[:, None], fold(xx, W)[None, :]] & inside


def register_masked_numpy(ref, img, ref_clear, img_clear, window):
    """THE statement of the masked registration (csrc/kernels_prep_masked.hip equals it bit for bit).  ref, img uint16 [128,128], their
    clear masks, window R in 1..32 -> ((dy, dx), registered, shifted frame uint16, shifted clear mask bool).

    For every shift s = (dy, dx) in [-R, R]^2, dy outer, both ascending: over m = ref_clear & clear_s (clear_s[p] = img_clear[p - s]
    inside the frame, False outside: nothing wraps), with a = ref and b[p] = img[p - s], the exact integer moments n, Sa, Sb, Saa, Sbb, Sab
    (int64: a, b < 2^16 and n <= 2^14 keep every moment, product and difference below 2^61);
        num = n Sab - Sa Sb,  da = n Saa - Sa^2,  db = n Sbb - Sb^2,    v = float64(num) / sqrt(float64(da) * float64(db)).
    A shift is a candidate when 10 n >= 3 max n (skimage's overlap_ratio = 3/10, over the window) and da > 0 and db > 0.  The largest v
    wins, ties to the first shift visited; without a candidate the shift is (0, 0) and registered is 0.  The frame is then shifted by
    `shift_masked_numpy`."""
    R = _check_window(window)
    ref, img = np.asarray(ref), np.asarray(img)
    if ref.shape != (LR_SIZE, LR_SIZE) or img.shape != ref.shape or np.shape(ref_clear) != ref.shape or np.shape(img_clear) != ref.shape:
        raise ValueError("masked registration takes %d x %d frames and masks" % (LR_SIZE, LR_SIZE))
    rc, ic = np.asarray(ref_clear) != 0, np.asarray(img_clear) != 0
    a, b = ref.astype(np.int64) * rc, img.astype(np.int64) * ic          # zero where their own mask is: Sab needs no mask
    aa, bb = a * a, b * b
    rc8, ic8 = rc.astype(np.int64), ic.astype(np.int64)
    N, Wd = LR_SIZE, 2 * R + 1
    mom = np.zeros((6, Wd * Wd), np.int64)
    for i in range(Wd * Wd):
        dy, dx = i // Wd - R, i % Wd - R
        P = (slice(max(0, dy), min(N, N + dy)), slice(max(0, dx), min(N, N + dx)))          # p with p - s inside the frame
        Q = (slice(max(0, -dy), min(N, N - dy)), slice(max(0, -dx), min(N, N - dx)))        # p - s
        mr, ms = rc8[P], ic8[Q]
        mom[:, i] = ((mr * ms).sum(), (a[P] * ms).sum(), (b[Q] * mr).sum(), (aa[P] * ms).sum(), (bb[Q] * mr).sum(), (a[P] * b[Q]).sum())
    n, Sa, Sb, Saa, Sbb, Sab = mom
    num, da, db = n * Sab - Sa * Sb, n * Saa - Sa * Sa, n * Sbb - Sb * Sb
    cand = (10 * n >= 3 * n.max()) & (da > 0) & (db > 0)
    if cand.any():
        v = np.full(Wd * Wd, -np.inf)
        v[cand] = num[cand].astype(np.float64) / np.sqrt(da[cand].astype(np.float64) * db[cand].astype(np.float64))
        i = int(np.argmax(v))                              # the first of the largest
        shift, registered = (i // Wd - R, i % Wd - R), 1
    else:
        shift, registered = (0, 0), 0
    out, clear = shift_masked_numpy(img, ic, shift)
    return shift, registered, out, clear


def register_masked_sets_numpy(frames, masks, set_offsets, ref_frame, window):
    """`register_masked_numpy` over sets, what `device_register_masked` returns: every frame against ref_frame[its set]; the reference
    frames themselves are copied through with shift (0, 0) and registered = 1."""
    frames, clear = np.asarray(frames), np.asarray(masks) != 0
    F = len(frames)
    shifts, reg = np.zeros((F, 2), np.int32), np.ones(F, np.uint8)
    of, om = frames.astype(np.uint16), clear.copy()
    for s in range(len(set_offsets) - 1):
        r = int(ref_frame[s])
        for f in range(int(set_offsets[s]), int(set_offsets[s + 1])):
            if f != r:
                shifts[f], reg[f], of[f], om[f] = register_masked_numpy(frames[r], frames[f], clear[r], clear[f], window)
    return shifts, reg, of, om, om.reshape(F, -1).sum(1).astype(np.int32)


def device_register_masked(frames, masks, set_offsets, ref_frame, window):
    """The masked registration on the device (csrc/kernels_prep_masked.hip): frames [F,128,128] uint16, masks [F,128,128] (nonzero = clear),
    set_offsets [S+1], ref_frame [S] frame indices, window 1..32 -> (shifts [F,2] int32 (dy, dx), registered [F] uint8, shifted frames
    uint16, shifted masks bool, their clear counts int32).  Equal to `register_masked_sets_numpy` bit for bit."""
    R = _check_window(window)
    frames, masks = np.asarray(frames), np.asarray(masks)
    F = frames.shape[0]
    S = len(set_offsets) - 1
    o, r = np.asarray(set_offsets, np.int64), np.asarray(ref_frame, np.int64)
    if S < 1 or o[0] != 0 or o[-1] != F or (np.diff(o) < 1).any() or len(r) != S or (r < o[:-1]).any() or (r >= o[1:]).any():
        raise ValueError("registration needs set_offsets[0] = 0, set_offsets[-1] = n_frames, no empty set, one reference inside each set")
    if frames.shape[1:] != (LR_SIZE, LR_SIZE) or masks.shape != frames.shape:
        raise ValueError("registration takes %d x %d frames, got %r / %r" % (LR_SIZE, LR_SIZE, frames.shape, masks.shape))
    import torch
    from . import _lib
    dev = _dev()
    fr = _to_dev(frames.astype(np.uint16, copy=False), dev)
    mk = _to_dev((masks != 0).view(np.uint8), dev)
    off, ref = _to_dev(o, dev), _to_dev(r.astype(np.int32), dev)
    shifts = torch.empty(F, 2, dtype=torch.int32, device=dev)
    reg = torch.empty(F, dtype=torch.uint8, device=dev)
    rf, rm = torch.empty_like(fr), torch.empty_like(mk)
    rc = torch.empty(F, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().probav_prep_register_masked(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(off), S, F, _lib.ptr(ref), R, _lib.ptr(shifts),
                                                      _lib.ptr(reg), _lib.ptr(rf), _lib.ptr(rm), _lib.ptr(rc), _lib.current_stream()),
               "probav_prep_register_masked")
    sh = shifts.cpu().numpy()
    if (sh == PREP_BAD_SHIFT).any():
        raise ValueError("probav_prep_register_masked: set_offsets / ref_frame break the preconditions of include/probav_hip.h (empty set or "
                         "a reference outside its set)")
    return sh, reg.cpu().numpy(), rf.cpu().numpy(), rm.cpu().numpy().astype(bool), rc.cpu().numpy()


# ---- refined quality masks (csrc/kernels_refine.hip) --------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class RefineSpec:
    """What `refine_masks_numpy` / `device_refine_masks` flag.  k: outlier threshold in MADs, a multiple of 1/16 with k16 = 16 k in 0..1024;
    floor: smallest scale in DN, 0..65535; min_clear: clear looks a pixel needs before it is judged, 3..64; dilate: radius in pixels by
    which the flags grow, 0..3; saturation: None, or the value 0..65535 above which a clear pixel is flagged whatever the set says.
    Anything else is a ValueError, here and wherever a spec is used."""
    k: float = 5.0
    floor: int = 32
    min_clear: int = 5
    dilate: int = 1
    saturation: object = None

    def __post_init__(self):
        _check_refine(self)

    @property
    def k16(self):
        return int(round(16 * self.k))


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_refine(spec):
    if not isinstance(spec, RefineSpec):
        raise ValueError("refine takes a prep.RefineSpec, got %r" % (spec,))
    k = spec.k
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not math.isfinite(k) or 16 * k != round(16 * k) \
            or not 0 <= round(16 * k) <= REFINE_MAX_K16:
        raise ValueError("refine k must be a multiple of 1/16 in 0..%d, got %r" % (REFINE_MAX_K16 // 16, k))
    for name, lo, hi in (("floor", 0, 65535), ("min_clear", 3, MAX_POOL), ("dilate", 0, REFINE_MAX_DILATE)):
        v = getattr(spec, name)
        if not _is_int(v) or not lo <= v <= hi:
            raise ValueError("refine %s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
    if spec.saturation is not None and (not _is_int(spec.saturation) or not 0 <= spec.saturation <= 65535):
        raise ValueError("refine saturation must be None or an integer in 0..65535, got %r" % (spec.saturation,))
    return spec


def _check_refine_sets(frames, masks, set_offsets):
    frames, masks = np.asarray(frames), np.asarray(masks)
    o = np.asarray(set_offsets, np.int64)
    if frames.ndim != 3 or masks.shape != frames.shape or min(frames.shape) < 1:
        raise ValueError("mask refinement takes frames and masks [F, H, W] with F, H, W >= 1, got %r / %r" % (frames.shape, masks.shape))
    if o.ndim != 1 or len(o) < 2 or o[0] != 0 or o[-1] != len(frames) or (np.diff(o) < 1).any():
        raise ValueError("mask refinement needs set_offsets[0] = 0, set_offsets[-1] = n_frames and no empty set")
    if np.diff(o).max() > MAX_POOL:
        raise ValueError("mask refinement takes sets of at most %d frames, got one of %d" % (MAX_POOL, np.diff(o).max()))
    return frames.astype(np.uint16, copy=False), masks != 0, o


def refine_set_numpy(x, c, spec):
    """One set of `refine_masks_numpy`, steps 1 to 5: x uint16 [T, H, W], c bool [T, H, W] -> (sat, o, med, mad, n); med and mad are int64
    [H, W] (0 where n = 0) whatever min_clear says."""
    T = len(x)
    x = x.astype(np.int64)
    sat = c & (x > spec.saturation) if spec.saturation is not None else np.zeros_like(c)
    cc = c & ~sat
    n = cc.sum(0)
    r = np.maximum(n - 1, 0) // 2
    BIG = 1 << 20                                           # above every value and every distance: unclear looks sort last
    pick = lambda v: np.take_along_axis(np.sort(np.where(cc, v, BIG), axis=0), r[None], 0)[0]
    med = np.where(n > 0, pick(x), 0)
    d = np.abs(x - med[None])
    mad = np.where(n > 0, pick(d), 0)
    s = np.maximum(mad, spec.floor)
    o = cc & (n >= spec.min_clear)[None] & (16 * d > spec.k16 * s[None])
    return sat, o, med, mad, n


def refine_masks_numpy(frames, clear, set_offsets, spec=None):
    """THE statement of the mask refinement (csrc/kernels_refine.hip equals it bit for bit).  frames uint16 [F, H, W] of one band AFTER
    registration, clear [F, H, W] (nonzero = clear), set_offsets [S+1] (the ragged convention of `device_register`), a RefineSpec ->
    (clear_out bool [F, H, W], counts int32 [F], flagged int32 [F, 2]).

    Per set with frames x[t], clear flags c[t], t < T <= 64, and per pixel p, all in integers:
      1. sat[t] = c[t] and saturation is not None and x[t] > saturation;  c'[t] = c[t] and not sat[t]
      2. n = #{t : c'[t]};  med = the element (n - 1) // 2 of {x[t] : c'[t]} in ascending order (the lower median)
      3. d[t] = |x[t] - med|;  mad = the element (n - 1) // 2 of {d[t] : c'[t]} in ascending order
      4. s = max(mad, floor)
      5. o[t] = c'[t] and n >= min_clear and 16 d[t] > k16 s      (strict; everything fits int32)
      6. f[t] = sat[t] or o[t]
      7. g[t][p] = any f[t][q] over |q - p|_inf <= dilate, q inside the frame (nothing wraps or reflects)
      8. clear_out[t] = c[t] and not g[t]
    counts = the ones of clear_out per frame, flagged = {sum sat, sum o} per frame (before the dilation).  Only values are selected, so
    ties need no rule; a set with T < min_clear gets the saturation flags alone; the frames are never changed."""
    spec = _check_refine(RefineSpec() if spec is None else spec)
    frames, c, off = _check_refine_sets(frames, clear, set_offsets)
    F, H, W = frames.shape
    f = np.zeros((F, H, W), bool)
    flagged = np.zeros((F, 2), np.int32)
    for i in range(len(off) - 1):
        sl = slice(off[i], off[i + 1])
        sat, o = refine_set_numpy(frames[sl], c[sl], spec)[:2]
        f[sl] = sat | o
        flagged[sl, 0], flagged[sl, 1] = sat.sum((1, 2)), o.sum((1, 2))
    r = spec.dilate
    g = np.zeros_like(f)
    pad = np.pad(f, ((0, 0), (r, r), (r, r)))              # zeros outside the frame
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            g |= pad[:, dy:dy + H, dx:dx + W]
    out = c & ~g
    return out, out.sum((1, 2)).astype(np.int32), flagged


def device_refine_masks(frames, masks, set_offsets, spec=None):
    """The mask refinement on the device (csrc/kernels_refine.hip): frames [F, H, W] uint16 (any H, W >= 1), masks [F, H, W] (nonzero =
    clear), set_offsets [S+1], a RefineSpec -> (clear_out bool [F, H, W], counts int32 [F], flagged int32 [F, 2] = {saturated, outliers}
    per frame before the dilation).  Equal to `refine_masks_numpy` bit for bit."""
    spec = _check_refine(RefineSpec() if spec is None else spec)
    frames, clear, o = _check_refine_sets(frames, masks, set_offsets)
    import torch
    from . import _lib
    dev = _dev()
    F, H, W = frames.shape
    fr, mk, off = _to_dev(frames, dev), _to_dev(clear.view(np.uint8), dev), _to_dev(o, dev)
    out = torch.empty_like(mk)
    planes = torch.empty((len(o) - 1) * 3 * H * W, dtype=torch.int64, device=dev)      # pixel_masks: per set and pixel, one bit per frame
    counts = torch.empty(F, dtype=torch.int32, device=dev)
    flagged = torch.empty(F, 2, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().probav_prep_refine_masks(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(off), len(o) - 1, F, H, W, int(np.diff(o).max()), spec.k16,
                                                   spec.floor, spec.min_clear, spec.dilate, -1 if spec.saturation is None else spec.saturation,
                                                   _lib.ptr(planes), _lib.ptr(out), _lib.ptr(counts), _lib.ptr(flagged), _lib.current_stream()),
               "probav_prep_refine_masks")
    cn = counts.cpu().numpy()
    if (cn == PREP_BAD_COUNT).any():
        raise ValueError("probav_prep_refine_masks: set_offsets break the preconditions of include/probav_hip.h (an empty or over-long set)")
    return out.cpu().numpy().astype(bool), cn, flagged.cpu().numpy()


def _refine_registered(rf, rm, offsets, spec, log):
    """registerImages' refinement of one band's registered flat arrays: the refined masks, with what they changed logged."""
    out, counts, flagged = device_refine_masks(rf, rm, offsets, spec)
    before = rm.reshape(len(rm), -1).sum(1).astype(np.int64)
    lost = before - counts
    log.info('[ INFO ] Refined masks (k %g, floor %d, min_clear %d, dilate %d, saturation %s): %d pixels newly masked of %d clear '
             '(%d saturated, %d temporal outliers, the rest by dilation); %d of %d frames lost more than 10 %% of their clear pixels',
             spec.k, spec.floor, spec.min_clear, spec.dilate, spec.saturation, int(lost.sum()), int(before.sum()), int(flagged[:, 0].sum()),
             int(flagged[:, 1].sum()), int((10 * lost > before).sum()), len(rm))
    # the number a user needs to choose `floor`: the median MAD of judged pixels, from the statement on the host over at most 8 sets
    pick = np.linspace(0, len(offsets) - 2, min(8, len(offsets) - 1)).astype(int)
    mads = []
    for i in np.unique(pick):
        sl = slice(offsets[i], offsets[i + 1])
        _, _, _, mad, n = refine_set_numpy(rf[sl].astype(np.uint16, copy=False), rm[sl] != 0, spec)
        mads.append(mad[n >= spec.min_clear])
    mads = np.concatenate(mads)
    if len(mads):
        log.info('[ INFO ] Refined masks: median over pixels of the temporal MAD is %d DN on %d sets (floor = %d DN)',
                 int(np.median(mads)), len(np.unique(pick)), spec.floor)
    return out


def device_xcorr_surface(ref, img):
    """Diagnostic: (fp32 surface [128,128], {B, c_ref, c_img, max}) the registration kernel ranks shifts by."""
    import torch
    from . import _lib
    dev = _dev()
    pair = _to_dev(np.stack([ref, img]).astype(np.uint16), dev)
    spec = torch.empty(LR_SIZE * LR_SIZE * 2, dtype=torch.float32, device=dev)
    surf = torch.empty(LR_SIZE, LR_SIZE, dtype=torch.float32, device=dev)
    info = torch.empty(4, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().probav_prep_xcorr_surface(_lib.ptr(pair), _lib.ptr(spec), _lib.ptr(surf), _lib.ptr(info), _lib.current_stream()),
               "probav_prep_xcorr_surface")
    i = info.cpu().numpy()
    return surf.cpu().numpy(), {"B": float(i[0]), "c_ref": int(i[1]), "c_img": int(i[2]), "max": float(i[3])}


def _device_patches(frames, masks, pad, win, stride):
    """`device_patches` without the copy to the host: (patches [S,P,T,win,win] fp32, masks uint8, counts [S,P,T] int32) as device tensors
    (tiles.build_tiles keeps the patches where they are and brings only the counts back)."""
    import torch
    from . import _lib
    dev = _dev()
    S, T, H, W = frames.shape
    nh, nw = (H + 2 * pad - win) // stride + 1, (W + 2 * pad - win) // stride + 1
    fr = _to_dev(np.asarray(frames, np.float32), dev)
    mk = _to_dev((np.asarray(masks) != 0).view(np.uint8), dev)
    P = nh * nw
    pt = torch.empty(S, P, T, win, win, dtype=torch.float32, device=dev)
    pm = torch.empty(S, P, T, win, win, dtype=torch.uint8, device=dev)
    pc = torch.empty(S, P, T, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().probav_prep_patches(_lib.ptr(fr), _lib.ptr(mk), S, T, H, W, pad, win, stride, _lib.ptr(pt), _lib.ptr(pm),
                                              _lib.ptr(pc), _lib.current_stream()), "probav_prep_patches")
    return pt, pm, pc


def device_patches(frames, masks, pad, win, stride):
    """frames [S,T,H,W] (cast to fp32), masks [S,T,H,W] -> patches [S,P,T,win,win] fp32, masks bool, counts [S,P,T] int32."""
    pt, pm, pc = _device_patches(frames, masks, pad, win, stride)
    return pt.cpu().numpy(), pm.cpu().numpy().astype(bool), pc.cpu().numpy()


def _objects(items):
    out = np.empty(len(items), dtype=object)
    for i, a in enumerate(items):
        out[i] = a
    return out


# ---- checkpoint 1 (utils/dataGenerator.py:844-941) --------------------------------------------------------------------------------
def loadAndSaveRawData(rawDataDir, arrayDir, band, isGrayScale=True, isTrainData=True):
    if not isGrayScale:
        raise ValueError("PROBA-V frames are greyscale (isGrayScale=True)")
    os.makedirs(arrayDir, exist_ok=True)
    key = 'TRAIN' if isTrainData else 'TEST'
    dirList = sorted(glob.glob(os.path.join(rawDataDir, key.lower(), band, 'imgset*')))
    read = lambda f: np.expand_dims(pngio.imread(f), axis=0)
    for name, pat in (('imgLR', 'LR*.png'), ('mskLR', 'QM*.png')):
        sets = _objects([np.array([read(f) for f in sorted(glob.glob(os.path.join(d, pat)))]) for d in dirList])
        sets.dump(os.path.join(arrayDir, f'{key}{name}_{band}.npy'))
    if isTrainData:
        for name, fname in (('imgHR', 'HR.png'), ('mskHR', 'SM.png')):
            a = np.expand_dims(np.array([read(os.path.join(d, fname)) for d in dirList]), axis=1)
            a.dump(os.path.join(arrayDir, f'{key}{name}_{band}.npy'))


def loadData(arrayDir, band):
    if not os.path.exists(arrayDir):
        raise Exception("[ ERROR ] Folder path does not exists...")
    if not os.listdir(arrayDir):
        raise Exception("[ ERROR ] No files in the provided directory...")
    load = lambda n: np.load(os.path.join(arrayDir, f'{n}_{band}.npy'), allow_pickle=True)
    TRAIN = (load('TRAINimgLR'), load('TRAINmskLR'), load('TRAINimgHR'), load('TRAINmskHR'))
    TEST = (load('TESTimgLR'), load('TESTmskLR'))
    return TRAIN, TEST


# ---- checkpoint 2 (utils/dataGenerator.py:599-841) --------------------------------------------------------------------------------
def registerFrame(img, msk, referenceImg, referenceMsk, tech='freq', window=8):
    """The reference's registerFrame (utils/dataGenerator.py:649-678) for one pair of [1, 128, 128] (or [128, 128]) frames and masks, on
    the device: tech='freq' is the plain circular registration (csrc/kernels_prep.hip), tech='time' the masked one over `window`
    (csrc/kernels_prep_masked.hip).  Returns (regImg float64, regMsk bool) in the shape of `img`."""
    _check_tech(tech)
    R = _check_window(window)
    shape = np.shape(img)
    pair = np.stack([np.asarray(referenceImg).reshape(LR_SIZE, LR_SIZE), np.asarray(img).reshape(LR_SIZE, LR_SIZE)]).astype(np.uint16)
    clear = np.stack([np.asarray(referenceMsk).reshape(LR_SIZE, LR_SIZE), np.asarray(msk).reshape(LR_SIZE, LR_SIZE)]) != 0
    if tech == 'time':
        _, _, rf, rm, _ = device_register_masked(pair, clear, [0, 2], [0], R)
    else:
        _, rf, rm, _ = device_register(pair, clear, [0, 2], [0])
    return rf[1].astype(np.float64).reshape(shape), rm[1].reshape(shape)


def registerImages(allImgLR, allMskLR, tech='freq', window=8, refine=None):
    """Per set: frames reordered by np.argsort(-clear count), the first is the reference, every other one registered against it
    (device; tech / window as registerFrame).  Returns an object array of float64 masked arrays [T, 1, 128, 128] (mask = ~clear).
    refine: None, or a RefineSpec: the registered frames' masks go through `device_refine_masks` (whichever `tech`) before the masked
    arrays are built; the data are the same either way."""
    _check_tech(tech)
    window = _check_window(window)
    if refine is not None:
        _check_refine(refine)
    sets_img = [np.asarray(allImgLR[i]) for i in range(len(allImgLR))]
    sets_msk = [np.asarray(allMskLR[i]) for i in range(len(allMskLR))]
    for a, m in zip(sets_img, sets_msk):
        assert a.shape == m.shape, 'Input shape does not match!'
    sizes = [len(a) for a in sets_img]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hw = sets_img[0].shape[-2:]
    frames = np.concatenate([a.reshape(-1, *a.shape[-2:]) for a in sets_img]).astype(np.uint16)
    masks = np.concatenate([(m != 0).reshape(-1, *m.shape[-2:]) for m in sets_msk])
    counts = device_count_nonzero(masks, hw[0] * hw[1]).astype(np.int64)
    order = np.concatenate([offsets[i] + np.argsort(-counts[offsets[i]:offsets[i + 1]]) for i in range(len(sizes))])
    if tech == 'time':
        _, reg, rf, rm, _ = device_register_masked(frames[order], masks[order], offsets, offsets[:-1], window)
        logging.getLogger("dataGenerator").info('[ INFO ] Masked registration (window %d): %d of %d frames had no candidate shift and '
                                                'stay where they are', window, int((reg == 0).sum()), len(reg))
    else:
        _, rf, rm, _ = device_register(frames[order], masks[order], offsets, offsets[:-1])
    if refine is not None:
        rm = _refine_registered(rf, rm, offsets, refine, logging.getLogger("dataGenerator"))
    out = []
    for i in range(len(sizes)):
        sl = slice(offsets[i], offsets[i + 1])
        data = rf[sl].astype(np.float64)[:, None]
        out.append(np.ma.masked_array(data, mask=~rm[sl][:, None]))
    return _objects(out)


def convertToMaskedArray(imgSets, mskSets):
    imgSets = np.squeeze(imgSets, axis=1)
    mskSets = np.squeeze(mskSets, axis=1)
    imgMskSets = np.ma.array([np.ma.masked_array(img, mask=~(msk != 0)) for img, msk in zip(imgSets, mskSets)])
    imgMskSets = np.expand_dims(imgMskSets, axis=1)
    assert (imgMskSets.shape == imgMskSets.mask.shape), 'Mask and Array shapes do not match!'
    return imgMskSets


def isImageSetNotCorrupted(imgSet, clarityThreshold):
    isImageClearEnough = np.array([np.count_nonzero(img.mask) / (img.shape[1] * img.shape[2]) < (1 - clarityThreshold) for img in imgSet])
    return np.sum(isImageClearEnough) != 0


def removeCorruptedTrainImageSets(imgMskLR, imgMskHR, clarityThreshold):
    booleanMask = np.array([isImageSetNotCorrupted(imgSet, clarityThreshold) for imgSet in imgMskLR])
    imgSetRemoved = np.arange(len(imgMskLR))[~booleanMask]
    return imgMskLR[booleanMask], imgMskHR[booleanMask], imgSetRemoved


def removeCorruptedTestImageSets(imgMskLR, clarityThreshold):
    booleanMask = np.array([isImageSetNotCorrupted(imgSet, clarityThreshold) for imgSet in imgMskLR])
    return imgMskLR[booleanMask]


def filterImgMskSet(imgSet, clarityThreshold):
    isImageClearEnough = np.array([np.count_nonzero(img.mask) / (img.shape[1] * img.shape[2]) < (1 - clarityThreshold) for img in imgSet])
    return imgSet[isImageClearEnough]


def pickClearImg(imgMsk, numImgToPick, rng=None):
    rng = np.random if rng is None else rng
    sortedIndices = np.argsort(np.sum(imgMsk.mask, axis=(1, 2, 3)))
    sortedImgMskArray = imgMsk[sortedIndices]
    count = 0
    if numImgToPick < len(imgMsk):
        trimmedImgMsk = sortedImgMskArray[:numImgToPick]
    else:
        trimmedImgMsk = np.ma.copy(sortedImgMskArray)
        count += (numImgToPick - len(trimmedImgMsk))
        while len(trimmedImgMsk) < numImgToPick:
            shuffledIndices = rng.choice(sortedIndices, size=len(sortedIndices), replace=False)
            trimmedImgMsk = np.ma.concatenate((trimmedImgMsk, imgMsk[shuffledIndices]))
        trimmedImgMsk = trimmedImgMsk[:numImgToPick]
    return trimmedImgMsk, count


def pickClearLRImgsPerImgSet(imgMskLR, numImgToPick, clarityThreshold, rng=None):
    cache = []
    for imgMsk in imgMskLR:
        clearData, _ = pickClearImg(filterImgMskSet(imgMsk, clarityThreshold), numImgToPick=numImgToPick, rng=rng)
        cache.append(np.expand_dims(clearData, axis=0))
    return np.ma.concatenate(cache)


# ---- checkpoint 3 (utils/dataGenerator.py:99-174, 553-596) ------------------------------------------------------------------------
def _patches(imgSets, patchSize, stride, pad=0):
    """Device pad + unfold of [S, T, C=1, H, W] masked frames -> ([S, P, T, 1, k, k] float32 masked array, masked-pixel counts [S, P, T])."""
    S, T, C, H, W = imgSets.shape
    if C != 1:
        raise ValueError("greyscale frames expected (C = 1), got C = %d" % C)
    data = np.ma.getdata(imgSets).reshape(S, T, H, W)
    mask = np.ma.getmaskarray(imgSets).reshape(S, T, H, W)
    p, m, c = device_patches(data, mask, pad, patchSize, stride)
    return np.ma.masked_array(p[:, :, :, None], mask=m[:, :, :, None]), c


def generatePatches(imgSets, patchSize, stride):
    """[S, T, C, H, W] -> [S, P * T, C, k, k] in the reference's (patch, frame) order (utils/dataGenerator.py:553-596)."""
    p, _ = _patches(imgSets, patchSize, stride)
    S, P, T = p.shape[:3]
    return p.reshape(S, P * T, *p.shape[3:])


# ---- checkpoint 4 (utils/dataGenerator.py:326-551) --------------------------------------------------------------------------------
def _mask_counts(patches):
    m = np.ma.getmaskarray(patches)
    return m.reshape(*m.shape[:-3], -1).sum(-1)


def clearFrameSelection(counts, pixels, k, clarityThreshold):
    """The index half of removeAndReplaceDirtyFrames: counts [P, T] masked pixels of every frame of every patch (`pixels` each) ->
    (sel [P, k] frame indices, count, countNotReplaced).  tiles.build_tiles applies `sel` to patches that stay on the device."""
    P, T = np.shape(counts)
    sel = np.empty((P, k), np.int64)
    count = countNotReplaced = 0
    for i in range(P):
        cnt = np.asarray(counts[i], np.int64)
        idx = np.nonzero(cnt / pixels < (1 - clarityThreshold))[0]
        if len(idx) == 0:
            idx = np.arange(T)
            count += T
            countNotReplaced += T
        else:
            count += T - len(idx)
        tiled = np.tile(idx, math.ceil(k / len(idx)))
        sel[i] = tiled[np.argsort(cnt[tiled])][:k]
    return sel, count, countNotReplaced


def removeAndReplaceDirtyFrames(imgSet, k, clarityThreshold, counts=None):
    """imgSet [P, T, C, H, W]: per patch, the frames that pass the threshold (all of them if none does), tiled to at least k, sorted by
    masked-pixel count (np.argsort of the tiled counts, as the reference), first k."""
    P, T, C, H, W = imgSet.shape
    counts = _mask_counts(imgSet) if counts is None else counts
    sel, count, countNotReplaced = clearFrameSelection(counts, H * W, k, clarityThreshold)
    out = imgSet[np.arange(P)[:, None], sel]
    return np.ma.masked_array(np.ma.getdata(out), mask=np.ma.getmaskarray(out)), count, countNotReplaced


def pickClearPatchesLR(patchesLR, k, clarityThreshold):
    counts = _mask_counts(patchesLR)
    sets = [removeAndReplaceDirtyFrames(s, k, clarityThreshold, c)[0] for s, c in zip(patchesLR, counts)]
    return np.ma.concatenate([np.expand_dims(s, 0) for s in sets])


def isPatchSetNotCorrupted(patchSet, clarityThreshold):
    return np.sum(np.array([np.count_nonzero(p.mask) / (p.shape[-1] * p.shape[-2]) < (1 - clarityThreshold) for p in patchSet])) != 0


def removeCorruptedTrainPatchSets(patchesLR, patchesHR, clarityThreshold):
    booleanMask = np.array([isPatchSetNotCorrupted(s, clarityThreshold) for s in patchesHR])
    return patchesLR[booleanMask], patchesHR[booleanMask]


def pickClearPatches(patchesLR, patchesHR, clarityThreshold):
    _, _, T, C, HLR, WLR = patchesLR.shape
    reshapeLR = patchesLR.reshape((-1, T, C, HLR, WLR))
    _, _, THR, C, HHR, WHR = patchesHR.shape
    reshapeHR = patchesHR.reshape((-1, THR, C, HHR, WHR))
    booleanMask = _mask_counts(reshapeHR)[:, 0] / (HHR * WHR) < (1 - clarityThreshold)
    return reshapeLR[booleanMask], reshapeHR[booleanMask]


# ---- checkpoint 5 (utils/dataGenerator.py:276-323) --------------------------------------------------------------------------------
def splitPatches(patchesLR, patchesHR, config):
    """sklearn train_test_split(LR, LR.mask, HR, HR.mask, test_size=split, random_state=17), restated: ShuffleSplit draws
    RandomState(17).permutation(n); the first ceil(split * n) are the test part, the rest (in permutation order) the train part."""
    n = len(patchesLR)
    perm = np.random.RandomState(17).permutation(n)
    n_test = math.ceil(config['split'] * n)
    test, train = perm[:n_test], perm[n_test:]
    return patchesLR[train], patchesLR[test], patchesHR[train], patchesHR[test]


def augmentByShufflingLRImgs(patchLR, numPermute=9, rng=None):
    rng = np.random if rng is None else rng
    if numPermute == 0:
        return patchLR
    numLRImg = patchLR.shape[3]
    cacheLR = [patchLR]
    for _ in range(numPermute):
        cacheLR.append(patchLR[:, :, :, rng.permutation(np.arange(numLRImg)), :])
    return np.ma.concatenate(cacheLR)


def augmentByFlipping(patches):
    return np.ma.concatenate((patches, np.flip(patches, axis=1), np.flip(patches, axis=2), np.flip(patches, axis=(1, 2))))


def augmentByRotating(patches):
    return np.ma.concatenate((patches, np.rot90(patches, k=1, axes=(1, 2)), np.rot90(patches, k=2, axes=(1, 2)),
                              np.rot90(patches, k=3, axes=(1, 2))))


def gridPatches(imgLR, imgHR, config):
    """Stages 3 and 4 for the training arrays of whole scenes (trimmedArrayDir's TRAINimgLR [S, T_pre, 1, H, H], TRAINimgHR [S, 1, 1, rH, rH]) in
    one go, through the functions those stages call: unfold on the patch grid, frame choice per threshold, the HR clarity filter, the
    transposes -> (LR [N, win, win, k, 1], HR [N, rP, rP, 1]) as trimmedPatchesDir holds them."""
    pad = config['max_shift'] // 2 if config['max_shift'] > 0 else 0
    lr = _patches(imgLR, config['patch_size'] + config['max_shift'], config['patch_stride'], pad)[0]
    khr = config['patch_size'] * (imgHR.shape[3] // imgLR.shape[3])
    hr = _patches(imgHR, khr, khr, 0)[0]
    for thr in config['low_res_patch_thresholds']:
        lr = pickClearPatchesLR(lr, k=config['num_low_res_imgs'], clarityThreshold=thr)
    lr, hr = removeCorruptedTrainPatchSets(lr, hr, config['high_res_threshold'])
    lr, hr = pickClearPatches(lr, hr, config['high_res_threshold'])
    return lr.transpose((0, 3, 4, 1, 2)), hr.transpose((0, 3, 4, 1, 2)).squeeze(4)


# ---- driver (utils/dataGenerator.py:33-273) ---------------------------------------------------------------------------------------
def main(config, band, rng=None, online_aug=False, register='freq', register_window=8, scene_split=False, refine=None):
    """register: 'freq' (the default: the plain circular registration, as the reference's registerFrame default) or 'masked' (the
    cloud-aware one over [-register_window, register_window]^2, the reference's tech='time'); stage 2 only.
    refine: None (the default: the masks as the ESA quality masks give them) or a RefineSpec: stage 2 takes temporal outliers and saturated
    pixels of the registered TRAIN and TEST frames out of their masks (`refine_masks_numpy`) before anything is selected; stage 2 only.
    online_aug: stage 5 draws the frame permutations as ever (same rng, same order) but SAVES them beside the un-augmented training
    arrays instead of applying them -- TRAINbasepatches{LR,HR}_<band>.npy and TRAINaugperms_<band>.npy, what `train.py --online-aug` reads
    (probav_amd.augment).  The TRAINVAL dumps do not depend on it.
    scene_split: stage 5 holds out whole SCENES of trimmedArrayDir instead of patches (crops.scene_split: RandomState(17).permutation(S), the
    first ceil(split S) scenes) -- random crops of the training scenes would overlap validation patches of the same scenes.  It writes
    the TRAINVAL dumps from the held-out scenes' grid patches (gridPatches) and TRAINscenes_<band>.npy, the training scenes' indices into
    trimmedArrayDir: what `train.py --random-crops` reads (probav_amd.crops).  Nothing else of stage 5 runs."""
    log = logging.getLogger("dataGenerator")
    if band not in ('NIR', 'RED'):
        raise ValueError("band must be NIR or RED, got %r" % band)
    if register not in REGISTER_MODES:
        raise ValueError("register must be one of %r, got %r" % (tuple(REGISTER_MODES), register))
    tech, register_window = REGISTER_MODES[register], _check_window(register_window)
    if refine is not None:
        _check_refine(refine)
    rawDataDir, cleanDataDir = config['raw_data'], config['preprocessing_out']
    d = {k: os.path.join(cleanDataDir, k) for k in ('arrayDir', 'trimmedArrayDir', 'patchesDir', 'trimmedPatchesDir', 'resolverDir',
                                                     'augmentedPatchesDir')}
    for p in d.values():
        os.makedirs(p, exist_ok=True)
    path = lambda k, n: os.path.join(d[k], f'{n}_{band}.npy')
    load = lambda k, n: np.load(path(k, n), allow_pickle=True)
    ckpt = config['ckpt']

    if 1 in ckpt:
        log.info('Loading and dumping raw data...')
        for b in ('NIR', 'RED'):
            for isTrain in (True, False):
                loadAndSaveRawData(rawDataDir, d['arrayDir'], b, isGrayScale=True, isTrainData=isTrain)

    if 2 in ckpt:
        TRAIN, TEST = loadData(d['arrayDir'], band)
        allImgLR, allMskLR, allImgHR, allMskHR = TRAIN
        allImgMskLR = registerImages(allImgLR, allMskLR, tech, register_window, refine)
        allImgMskHR = convertToMaskedArray(allImgHR, allMskHR)
        allImgMskHR.dump(path('resolverDir', 'TRAINimgHR'))
        trmImgMskLR, trmImgMskHR, imgSetRemoved = removeCorruptedTrainImageSets(allImgMskLR, allImgMskHR, config['low_res_threshold'])
        start = 0 if band == 'RED' else 594
        np.savetxt(f'removedTrainSets{band}.txt', imgSetRemoved + start)
        if len(imgSetRemoved):
            print(f'[ WARNING ] Imgsets {imgSetRemoved} were removed')
        trmImgMskLR = pickClearLRImgsPerImgSet(trmImgMskLR, config['num_low_res_imgs_pre'], config['low_res_threshold'], rng)
        allImgLRTest, allMskLRTest = TEST
        allImgMskLRTest = registerImages(allImgLRTest, allMskLRTest, tech, register_window, refine)
        trmImgMskLRTest = removeCorruptedTestImageSets(allImgMskLRTest, config['low_res_threshold'])
        trmImgMskLRTest = pickClearLRImgsPerImgSet(trmImgMskLRTest, config['num_low_res_imgs_pre'], config['low_res_threshold'], rng)
        trmImgMskLR.dump(path('trimmedArrayDir', 'TRAINimgLR'))
        trmImgMskHR.dump(path('trimmedArrayDir', 'TRAINimgHR'))
        trmImgMskLRTest.dump(path('trimmedArrayDir', 'TESTimgLR'))

    if 3 in ckpt:
        pad = config['max_shift'] // 2 if config['max_shift'] > 0 else 0
        k = config['patch_size'] + config['max_shift']
        test = load('trimmedArrayDir', 'TESTimgLR')
        _patches(test, k, config['patch_size'], pad)[0].dump(path('patchesDir', 'TESTpatchesLR'), protocol=4)
        train = load('trimmedArrayDir', 'TRAINimgLR')
        H = train.shape[3]
        _patches(train, k, config['patch_stride'], pad)[0].dump(path('patchesDir', 'TRAINpatchesLR'), protocol=4)
        hr = load('trimmedArrayDir', 'TRAINimgHR')
        khr = config['patch_size'] * (hr.shape[3] // H)
        _patches(hr, khr, khr, 0)[0].dump(path('patchesDir', 'TRAINpatchesHR'), protocol=4)

    if 4 in ckpt:
        test, train = load('patchesDir', 'TESTpatchesLR'), load('patchesDir', 'TRAINpatchesLR')
        for thr in config['low_res_patch_thresholds']:
            test = pickClearPatchesLR(test, k=config['num_low_res_imgs'], clarityThreshold=thr)
        for thr in config['low_res_patch_thresholds']:
            train = pickClearPatchesLR(train, k=config['num_low_res_imgs'], clarityThreshold=thr)
        test.dump(path('resolverDir', 'TESTpatchesLR'), protocol=4)
        train.dump(path('resolverDir', 'TRAINpatchesLR'), protocol=4)
        hr = load('patchesDir', 'TRAINpatchesHR')
        train, hr = removeCorruptedTrainPatchSets(train, hr, config['high_res_threshold'])
        train, hr = pickClearPatches(train, hr, config['high_res_threshold'])
        train = train.transpose((0, 3, 4, 1, 2))
        hr = hr.transpose((0, 3, 4, 1, 2)).squeeze(4)
        test.dump(path('trimmedPatchesDir', 'TESTpatchesLR'), protocol=4)
        train.dump(path('trimmedPatchesDir', 'TRAINpatchesLR'), protocol=4)
        hr.dump(path('trimmedPatchesDir', 'TRAINpatchesHR'), protocol=4)

    if 5 in ckpt and scene_split:
        from .crops import scene_split as split_scenes
        imgLR, imgHR = load('trimmedArrayDir', 'TRAINimgLR'), load('trimmedArrayDir', 'TRAINimgHR')
        val, train = split_scenes(len(imgLR), config['split'])
        lrVal, hrVal = gridPatches(imgLR[val], imgHR[val], config)
        lrVal.dump(path('augmentedPatchesDir', 'TRAINVALpatchesLR'), protocol=4)
        hrVal.dump(path('augmentedPatchesDir', 'TRAINVALpatchesHR'), protocol=4)
        np.save(path('augmentedPatchesDir', 'TRAINscenes'), np.sort(train).astype(np.int64))
        log.info('[ INFO ] Scene split: %d validation scenes (%d grid patches), %d training scenes', len(val), len(lrVal), len(train))
        return

    if 5 in ckpt:
        lr, hr = load('trimmedPatchesDir', 'TRAINpatchesLR'), load('trimmedPatchesDir', 'TRAINpatchesHR')
        lr, lrVal, hr, hrVal = splitPatches(lr, hr, config)
        lrVal.dump(path('augmentedPatchesDir', 'TRAINVALpatchesLR'), protocol=4)
        hrVal.dump(path('augmentedPatchesDir', 'TRAINVALpatchesHR'), protocol=4)
        if online_aug:
            from .augment import draw_perms
            perms = draw_perms(config['num_low_res_permute'], lr.shape[3], rng)      # the draws augmentByShufflingLRImgs would make
            lr.dump(path('augmentedPatchesDir', 'TRAINbasepatchesLR'), protocol=4)
            hr.dump(path('augmentedPatchesDir', 'TRAINbasepatchesHR'), protocol=4)
            np.save(path('augmentedPatchesDir', 'TRAINaugperms'), perms)
            return
        lr = augmentByShufflingLRImgs(lr, numPermute=config['num_low_res_permute'], rng=rng)
        if config['to_flip']:
            lr = augmentByFlipping(lr)
        if config['to_rotate']:
            lr = augmentByRotating(lr)
        lr.dump(path('augmentedPatchesDir', 'TRAINpatchesLR'), protocol=4)
        hr = np.tile(hr, (config['num_low_res_permute'] + 1, 1, 1, 1))
        if config['to_flip']:
            hr = augmentByFlipping(hr)
        if config['to_rotate']:
            hr = augmentByRotating(hr)
        hr.dump(path('augmentedPatchesDir', 'TRAINpatchesHR'), protocol=4)
