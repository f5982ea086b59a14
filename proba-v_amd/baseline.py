"""The bicubic-mean baseline of the PROBA-V competition on the device (test.py --method baseline, evaluate.py --baseline): every LR frame of an
image set upscaled 3 x by the Keys cubic, the frames of highest clearance averaged.  It needs no weights; it replaces the reference's unfinished
bicubicMean / padding (evaluate.py:142-197) and the baseline upscaling of utils/utils.py:534-586.

The statement (`baseline_numpy`, int64, no floats; csrc/kernels_baseline.hip equals it bit for bit).  frames uint16 [F, H, W], clear uint8
[F, H, W] (nonzero = clear pixel), set_offsets int64 [S + 1] (ragged sets, the layout of probav_prep_register), scale 3.

Upscale of one frame p: Keys cubic, a = -1/2, half-pixel centres, clamped indices.  HR index Y sits at the LR coordinate (Y - 1) / 3; with
i0 = floor((Y - 1) / 3) and t = ((Y - 1) mod 3) / 3 the four taps are the rows clamp(i0 - 1 .. i0 + 2, 0, H - 1) with the integer weights over 27

    t = 0: (0, 27, 0, 0)        t = 1/3: (-2, 21, 9, -1)        t = 2/3: (-1, 9, 21, -2)                      (WEIGHTS27, from `keys_cubic`)

and columns likewise: U_f[Y, X] = sum_ij wy_i wx_j p[row_i, col_j], an integer with the implied denominator 729.

Modes.  "esa": with c_f = count_nonzero(clear[f]), exactly the frames of the set with c_f == max c, all ties included; K is the same for every
pixel of the set (ESA's "frames of maximum clearance").  "clear": frame f contributes to HR pixel (Y, X) iff clear[f, Y // 3, X // 3]; where no
frame of the set is clear, all of them contribute; K = K(Y, X).

Mean.  N = sum_f U_f, D = 729 K, q = N / D rounded half to even in integers (floor division, 2 (N mod D) against D, ties to even q; N may be
negative: the cubic overshoots), out = clip(q, 0, 65535).  Nothing is clipped before the mean.  The result is fp32 [S, 3H, 3W] holding integers,
like testClass.resolve_images, with K_used int32 [S] (in "clear" mode the set's frame count).  An empty set, or one of more than MAX_FRAMES
frames, is a ValueError.

Two deviations from ESA's own baseline ('Bicubic-mean baseline'): ESA upscales with skimage's order-3 spline, not the Keys
kernel, and averages in floating point; here the mean is rounded once, in integers.  Numbers made with this module are a stand-in for norm.csv,
not a reproduction of it.
"""
import os
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from .inference import FIRST_ID, numbered
from .intmath import round_half_even_div

SCALE = 3
MAX_FRAMES = 4096                 # frames per set (csrc/kernels_baseline.hip)
MODES = ("esa", "clear")          # index = PROBAV_BASELINE_ESA / PROBAV_BASELINE_CLEAR
FRAMES = ("raw", "registered")
BAD_SET = -1                      # PROBAV_BASELINE_BAD_SET
SETS_PER_LAUNCH = 256             # baseline_images: image sets per call (a band's 600 sets of 128 x 128 frames need no more than ~0.5 GB at once)


def keys_cubic(x, a=Fraction(-1, 2)):
    """The Keys cubic convolution kernel W(x) (Keys 1981; a = -1/2), exact for a Fraction argument."""
    x = abs(Fraction(x))
    if x <= 1:
        return (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1
    if x < 2:
        return a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a
    return Fraction(0)


def _weights27():
    rows = []
    for ph in range(SCALE):
        t = Fraction(ph, SCALE)
        w = [keys_cubic(t - k) * 27 for k in (-1, 0, 1, 2)]           # taps i0 - 1 .. i0 + 2 lie at t + 1, t, 1 - t, 2 - t
        assert all(v.denominator == 1 for v in w)
        rows.append(tuple(int(v) for v in w))
    return tuple(rows)


WEIGHTS27 = _weights27()          # [phase][tap]: ((0, 27, 0, 0), (-2, 21, 9, -1), (-1, 9, 21, -2))


def _taps(n_lr):
    """(index [3 n, 4], weight [3 n, 4]) of every HR position along an axis of n_lr LR samples."""
    Y = np.arange(SCALE * n_lr, dtype=np.int64)
    i0, ph = (Y - 1) // SCALE, (Y - 1) % SCALE                        # numpy's floor division / non-negative modulo
    idx = np.clip(i0[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], 0, n_lr - 1)
    return idx, np.asarray(WEIGHTS27, np.int64)[ph]


def upscale_numpy(frames):
    """U of every frame: [F, H, W] integers -> int64 [F, 3H, 3W], each value over 729."""
    p = np.asarray(frames).astype(np.int64)
    if p.ndim != 3 or p.shape[1] < 1 or p.shape[2] < 1:
        raise ValueError("frames must be [F, H, W] with H, W >= 1, got %r" % (p.shape,))
    ri, rw = _taps(p.shape[1])
    ci, cw = _taps(p.shape[2])
    v = sum(rw[None, :, k, None] * p[:, ri[:, k], :] for k in range(4))
    return sum(cw[None, None, :, k] * v[:, :, ci[:, k]] for k in range(4))


def check_sets(set_offsets, n_frames):
    """set_offsets as int64 [S + 1] after the checks of the statement: starts at 0, ends at n_frames, every set of 1 .. MAX_FRAMES frames."""
    o = np.asarray(set_offsets, np.int64).reshape(-1)
    if len(o) < 2 or o[0] != 0 or o[-1] != n_frames:
        raise ValueError("baseline: set_offsets must be [S + 1] with set_offsets[0] = 0 and set_offsets[-1] = n_frames = %d, got %r" % (n_frames, o.tolist()[:8]))
    sizes = np.diff(o)
    if (sizes < 1).any():
        raise ValueError("baseline: empty image set (set %d)" % int(np.argmax(sizes < 1)))
    if (sizes > MAX_FRAMES).any():
        raise ValueError("baseline: an image set of %d frames; at most %d" % (int(sizes.max()), MAX_FRAMES))
    return o


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError("baseline mode must be one of %r, got %r" % (MODES, mode))
    return mode


def selected_frames_numpy(clear, set_offsets):
    """bool [F]: the frames "esa" mode averages -- those whose clear count equals their set's largest."""
    c = np.count_nonzero(np.asarray(clear).reshape(len(clear), -1), axis=1)
    o = check_sets(set_offsets, len(c))
    sel = np.zeros(len(c), bool)
    for s in range(len(o) - 1):
        sel[o[s]:o[s + 1]] = c[o[s]:o[s + 1]] == c[o[s]:o[s + 1]].max()
    return sel


def baseline_numpy(frames, clear, set_offsets, mode="esa", scale=SCALE):
    """The statement of this module's docstring -> (out float32 [S, 3H, 3W] holding integers, K_used int32 [S])."""
    if scale != SCALE:
        raise ValueError("baseline: scale must be %d (the integer weights over 27 are those of scale 3), got %r" % (SCALE, scale))
    _check_mode(mode)
    frames, clear = np.asarray(frames), np.asarray(clear)
    if frames.ndim != 3 or clear.shape != frames.shape or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("baseline: frames and clear must both be [F, H, W] with H, W >= 1; got %r %r" % (frames.shape, clear.shape))
    o = check_sets(set_offsets, frames.shape[0])
    S, H, W = len(o) - 1, frames.shape[1], frames.shape[2]
    out = np.empty((S, SCALE * H, SCALE * W), np.float32)
    k_used = np.empty(S, np.int32)
    sel = selected_frames_numpy(clear, o) if mode == "esa" else None
    for s in range(S):
        sl = slice(o[s], o[s + 1])
        U = upscale_numpy(frames[sl])
        if mode == "esa":
            K = np.int64(sel[sl].sum())
            N = U[sel[sl]].sum(axis=0)
            k_used[s] = K
        else:
            m = np.repeat(np.repeat(clear[sl] != 0, SCALE, axis=1), SCALE, axis=2).astype(np.int64)      # clear[f, Y // 3, X // 3]
            K = m.sum(axis=0)
            N = np.where(K > 0, (U * m).sum(axis=0), U.sum(axis=0))
            K = np.where(K > 0, K, U.shape[0])
            k_used[s] = U.shape[0]
        out[s] = np.clip(round_half_even_div(N, 729 * K), 0, 65535)
    return out, k_used


@dataclass(frozen=True)
class BaselineSpec:
    """Which baseline: mode "esa" (frames of maximum clearance) or "clear" (per-pixel clear frames); frames "raw" (the stage-1 dumps: ESA's
    definition, unregistered, all sets) or "registered" (trimmedArrayDir: what the network's patches are cut from)."""
    mode: str = "esa"
    frames: str = "raw"

    def __post_init__(self):
        _check_mode(self.mode)
        if self.frames not in FRAMES:
            raise ValueError("baseline frames must be one of %r, got %r" % (FRAMES, self.frames))


def baseline_device(frames, clear, set_offsets, spec=BaselineSpec()):
    """The statement on the device (torch.ops.probav.baseline_upscale_mean): frames / clear numpy arrays or tensors [F, H, W], set_offsets
    [S + 1] -> (out float32 [S, 3H, 3W], K_used int32 [S]), device tensors.  The sets are checked on the host first."""
    import torch
    from . import _lib, ops                                # noqa: F401  (ops registers torch.ops.probav.*)
    for t, name in ((frames, "frames"), (clear, "clear")):
        if isinstance(t, torch.Tensor):
            _lib.require_device(t, name)
    if not torch.cuda.is_available():
        raise RuntimeError("baseline_device needs a HIP device: the baseline kernel runs only on a gfx950 device (no CPU fallback)")
    dev = next((t.device for t in (frames, clear) if isinstance(t, torch.Tensor)), torch.device("cuda", torch.cuda.current_device()))
    o = check_sets(set_offsets.cpu().numpy() if isinstance(set_offsets, torch.Tensor) else set_offsets, int(frames.shape[0]))
    if not isinstance(frames, torch.Tensor):
        a = np.asarray(frames)
        if a.dtype != np.uint16:
            if a.size and (np.any(a != np.rint(a)) or a.min() < 0 or a.max() > 65535):
                raise ValueError("baseline: frames must hold 16-bit integers, got %s" % a.dtype)
            a = a.astype(np.uint16)
        frames = torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(torch.uint16)
    if not isinstance(clear, torch.Tensor):
        clear = torch.from_numpy(np.ascontiguousarray(np.asarray(clear) != 0)).to(dev)
    return torch.ops.probav.baseline_upscale_mean(frames, clear, torch.from_numpy(o).to(dev), spec.mode)


def _ragged(img_sets, msk_sets):
    """Object arrays of per-set [T, 1, H, W] frames and quality masks (stage 1) -> (frames uint16 [F, H, W], clear bool, sizes)."""
    fr = [np.asarray(img_sets[i]) for i in range(len(img_sets))]
    mk = [np.asarray(msk_sets[i]) for i in range(len(msk_sets))]
    if len(fr) != len(mk) or any(a.shape != m.shape for a, m in zip(fr, mk)):
        raise ValueError("baseline: LR frames and their masks do not match")
    return [a.reshape(-1, *a.shape[-2:]).astype(np.uint16) for a in fr], [(m != 0).reshape(-1, *m.shape[-2:]) for m in mk]


def load_sets(config, band, split, frames):
    """-> (list of per-set uint16 [T, H, W], list of per-set clear bool [T, H, W], image-set ids).  split: "TRAIN" or "TEST"."""
    band, split = band.upper(), "TEST" if split == "TEST" else "TRAIN"
    if band not in ("NIR", "RED"):
        raise ValueError("band must be NIR or RED, got %r" % band)
    first = FIRST_ID[(split, band)]
    if frames == "raw":
        from . import prep
        TRAIN, TEST = prep.loadData(os.path.join(config["preprocessing_out"], "arrayDir"), band)
        img, msk = (TRAIN[0], TRAIN[1]) if split == "TRAIN" else TEST
        fr, cl = _ragged(img, msk)
        return fr, cl, [first + k for k in range(len(fr))]              # every set of the band, as ESA scores them
    if frames != "registered":
        raise ValueError("baseline frames must be one of %r, got %r" % (FRAMES, frames))
    a = np.load(os.path.join(config["preprocessing_out"], "trimmedArrayDir", "%simgLR_%s.npy" % (split, band)), allow_pickle=True)
    data, masked = np.ma.getdata(a), np.ma.getmaskarray(a)              # [sets, T, 1, H, W], mask = obscured
    if data.ndim != 5 or data.shape[2] != 1:
        raise ValueError("trimmedArrayDir/%simgLR_%s.npy: expected [sets, T, 1, H, W], got %r" % (split, band, data.shape))
    if np.any(data != np.rint(data)) or (data.size and (data.min() < 0 or data.max() > 65535)):
        raise ValueError("trimmedArrayDir/%simgLR_%s.npy: the frames are not 16-bit integers" % (split, band))
    ids = [i for i, _ in numbered(data, split, band)]                   # test.py's rule: the removed ids are skipped, whatever the split
    return [d[:, 0].astype(np.uint16) for d in data], [~m[:, 0] for m in masked], ids


def baseline_images(config, band, split="TRAIN", spec=BaselineSpec()):
    """The baseline image of every image set of a band -> (uint16 [n, 3H, 3W], ids): with spec.frames == "raw" from the stage-1 dumps
    (<preprocessing_out>/arrayDir through prep.loadData: unregistered, every set, ids consecutive from the band's first), with "registered"
    from trimmedArrayDir/<TEST|TRAIN>imgLR_<band>.npy (the removed sets absent, ids as test.py names them)."""
    fr, cl, ids = load_sets(config, band, split, spec.frames)
    outs = []
    for i in range(0, len(fr), SETS_PER_LAUNCH):
        f, c = fr[i:i + SETS_PER_LAUNCH], cl[i:i + SETS_PER_LAUNCH]
        offsets = np.concatenate([[0], np.cumsum([len(a) for a in f])]).astype(np.int64)
        out, _ = baseline_device(np.concatenate(f), np.concatenate(c), offsets, spec)
        outs.append(out.cpu().numpy().astype(np.uint16))                # integers in [0, 65535]: exact
    if not outs:
        return np.zeros((0, 0, 0), np.uint16), ids
    return np.concatenate(outs), ids


def add_cli_args(p):
    """--baseline-mode / --baseline-frames, shared by test.py and evaluate.py."""
    p.add_argument("--baseline-mode", type=str, default=None, choices=MODES, help="which frames the baseline averages: esa (default) = the frames of "
                   "maximum clearance of every set; clear = per pixel, the frames that are clear there")
    p.add_argument("--baseline-frames", type=str, default=None, choices=FRAMES, help="what the baseline reads: raw (default) = the unregistered "
                   "stage-1 dumps, every set (ESA's definition); registered = trimmedArrayDir, what the network's patches are cut from")


def cli_spec(p, opt, active, flag):
    """The BaselineSpec of the two sub-flags (defaults esa / raw), or a parser error when they are given without `flag`."""
    if not active:
        if opt.baseline_mode is not None or opt.baseline_frames is not None:
            p.error("--baseline-mode / --baseline-frames need %s" % flag)
        return None
    opt.baseline_mode = opt.baseline_mode or "esa"
    opt.baseline_frames = opt.baseline_frames or "raw"
    return BaselineSpec(opt.baseline_mode, opt.baseline_frames)
