"""Frame-window ensemble: the numpy statement of the two kernels of csrc/kernels_windows.hip (testClass.resolve_windowed /
resolve_windowed_frames drive them; INTEGRATION.md, 'Frame windows').

Inference shows the network only k = num_low_res_imgs of the T_pre = num_low_res_imgs_pre registered frames of an image set: per patch, the
dataset builder keeps the k clearest.  Here a window of k frames slides over the frames of every tile sorted from clearest to dirtiest, the
network predicts one image per window, and the predictions are averaged with integer weights.  With P = patch_size, win = P + max_shift,
pixels = win**2, counts[t] the masked pixels of frame t of the tile (what the builder's unfold returns):

  limit     L = max_masked(pixels, threshold): the number of integers c in [0, pixels] with c / pixels < (1 - threshold), evaluated in fp64
            exactly as prep.clearFrameSelection writes it; they are a prefix, so "frame t is eligible" is the integer test counts[t] < L.
  order     the eligible frames of a tile -- all T_pre frames when none is eligible -- by (count ascending, frame index ascending): r[0 .. E).
            The index tie-break is deliberate: the frames of trimmedArrayDir are already sorted clearest-first per image by pickClearImg, and
            the tie order of np.argsort in the builder is unspecified.
  list      m = ceil(k / E), Q[i] = r[i // m] for i < E m: the builder's tiled, sorted list (removeAndReplaceDirtyFrames).
  window j  takes Q[(j step + i) % (E m)], i = 0 .. k - 1, for j < W.  FrameWindowSpec.validate requires (W - 1) step + k <= T_pre, so a tile
            whose frames are all eligible never wraps (W = 1 is exempt: one window is the builder's own choice, which tiles a pool
            shorter than k).  Window 0 is the builder's choice: its count sequence equals that of
            tiles.select_frames on every tile whatever the tie order, and where the eligible counts of a tile are pairwise distinct the
            frames themselves are equal.
  weight    "clear": weight[j] = the sum over the window's k frames of (pixels - count), the clear pixels it shows the network; "uniform": 1.
            A tile whose weights are all 0 gets all 1.
  member    p_j = rint(clip(net(x_j), lo, hi)), an integer (with an EnsembleSpec: resolve_ensemble(..., final="round") of the window).
  mean      out = (sum_j w_j p_j) / (sum_j w_j) rounded half to even in exact 64-bit integer arithmetic (q = N div D; 2 (N mod D) against D;
            ties to the even q), float32 holding integers.  W = 1 with uniform weights is the identity on rounded members.

Nothing is floating point after each member's own rint, so the result does not depend on summation order, launch sets or device and the
numpy functions below equal the kernels bit for bit.  Bound: w <= k pixels < 2**16 at the shipped sizes (the kernel admits any int32),
W <= 64 and p <= 2**24 give sums below 2**46.
"""
import math

import numpy as np

from .intmath import clip_rint_numpy, round_half_even_div

WEIGHTS = ("clear", "uniform")          # index = PROBAV_WINDOWS_CLEAR / PROBAV_WINDOWS_UNIFORM
MAX_WINDOWS = 64
MAX_POOL = 64                           # T_pre: one lane of a wave per frame in the ranking


def max_masked(pixels, threshold):
    """L: frame t of a tile is eligible iff counts[t] < L.  The fp64 test of prep.clearFrameSelection on every possible count."""
    pixels = int(pixels)
    if pixels < 1:
        raise ValueError("pixels = %d" % pixels)
    ok = np.arange(pixels + 1, dtype=np.int64) / pixels < (1 - threshold)
    L = int(ok.sum())
    assert ok[:L].all() and not ok[L:].any(), "the eligible counts are not a prefix of 0 .. %d" % pixels
    return L


def single_threshold(config):
    """The one entry of low_res_patch_thresholds; ValueError when the cfg has several (the builder chains them: the windows are defined for one)."""
    thr = list(config["low_res_patch_thresholds"])
    if len(thr) != 1:
        raise ValueError("frame windows are defined for one patch threshold; low_res_patch_thresholds has %d entries: %s" % (len(thr), thr))
    return float(thr[0])


class FrameWindowSpec:
    """W windows of k frames, `step` positions of the sorted frame list apart, averaged with "clear" (clear-pixel) or "uniform" weights."""

    def __init__(self, windows, step=1, weights="clear", threshold=None):
        if weights not in WEIGHTS:
            raise ValueError("weights must be one of %s, got %r" % (WEIGHTS, weights))
        self.windows, self.step, self.weights = int(windows), int(step), weights
        self.threshold = None if threshold is None else float(threshold)    # the cfg's patch threshold (bind): it decides which frames are eligible
        if not 1 <= self.windows <= MAX_WINDOWS:
            raise ValueError("frame windows W = %d; 1 <= W <= %d" % (self.windows, MAX_WINDOWS))
        if self.step < 1:
            raise ValueError("frame window step = %d; step >= 1" % self.step)

    @property
    def mode(self):
        return WEIGHTS.index(self.weights)

    def bind(self, config):
        """The spec with the cfg's one patch threshold (ValueError when the cfg has several)."""
        return FrameWindowSpec(self.windows, self.step, self.weights, single_threshold(config))

    def limit(self, pixels):
        """L = max_masked(pixels, threshold) of the bound threshold."""
        if self.threshold is None:
            raise ValueError("the FrameWindowSpec has no patch threshold: FrameWindowSpec(..., threshold=t) or spec.bind(config)")
        return max_masked(pixels, self.threshold)

    @staticmethod
    def largest(T_pre, k, step=1):
        """The largest valid W for a pool of T_pre frames (a pool shorter than k admits the one window of the builder's own choice)."""
        return 1 if T_pre < k else min(MAX_WINDOWS, (int(T_pre) - int(k)) // int(step) + 1)

    def validate(self, T_pre, k, config=None):
        T_pre, k = int(T_pre), int(k)
        if not 1 <= k <= MAX_POOL or not 1 <= T_pre <= MAX_POOL:
            raise ValueError("k = %d, a pool of T_pre = %d frames; 1 <= k, T_pre <= %d" % (k, T_pre, MAX_POOL))
        need = (self.windows - 1) * self.step + k
        if self.windows > 1 and need > T_pre:
            raise ValueError("%d windows at step %d over num_low_res_imgs = %d frames need (W - 1) * step + k = %d frames, the pool "
                             "(num_low_res_imgs_pre) has %d: the largest valid W at this step is %d"
                             % (self.windows, self.step, k, need, T_pre, self.largest(T_pre, k, self.step)))
        if config is not None:
            single_threshold(config)
        return self


def frame_windows_select_numpy(counts, pixels, k, L, W, step, weights="clear"):
    """counts [N, T_pre] -> (sel int32 [N, W, k], weight int32 [N, W]): the frames of every window of every tile and the window weights."""
    counts = np.asarray(counts, np.int64)
    if counts.ndim != 2 or weights not in WEIGHTS:
        raise ValueError("counts [N, T_pre], weights one of %s; got %s %r" % (WEIGHTS, counts.shape, weights))
    N, T_pre = counts.shape
    pixels, k, L, W, step = int(pixels), int(k), int(L), int(W), int(step)
    sel, weight = np.empty((N, W, k), np.int32), np.empty((N, W), np.int32)
    for n in range(N):
        c = counts[n]
        idx = np.nonzero(c < L)[0]
        if len(idx) == 0:
            idx = np.arange(T_pre)
        r = idx[np.lexsort((idx, c[idx]))]                          # by (count, index)
        m = math.ceil(k / len(r))
        Q = np.repeat(r, m)
        for j in range(W):
            sel[n, j] = Q[(j * step + np.arange(k)) % len(Q)]
        weight[n] = (pixels - c[sel[n]]).sum(-1) if weights == "clear" else 1
        if not weight[n].any():
            weight[n] = 1
    return sel, weight


def frame_windows_gather_numpy(patches, sel):
    """patches [N, T_pre, win, win], sel [N, W, k] -> x float32 [N, W, win, win, k, 1]: test.py's transpose per window; frame i of window j
    of tile n is patches[n, sel[n, j, i]], copied bit for bit."""
    p = np.asarray(patches, np.float32)
    sel = np.asarray(sel)
    if p.ndim != 4 or sel.ndim != 3 or sel.shape[0] != p.shape[0]:
        raise ValueError("patches [N, T_pre, win, win], sel [N, W, k]; got %s %s" % (p.shape, sel.shape))
    g = p[np.arange(p.shape[0])[:, None, None], sel]               # [N, W, k, win, win]
    return np.ascontiguousarray(g.transpose(0, 1, 3, 4, 2))[..., None]


def frame_windows_reduce_numpy(sr, weight, lo=0.0, hi=float(2 ** 16)):
    """sr [N W, S, S] (or [..., S, S, 1]; raw predictions or rounded ones), weight [N, W] non-negative integers with a positive sum per tile
    -> float32 [N, S, S]: the weighted mean of the W members of every tile in int64, rounded half to even."""
    m = np.asarray(sr, dtype=np.float32)
    if m.ndim == 4 and m.shape[3] == 1:
        m = m[..., 0]
    w = np.asarray(weight)
    if m.ndim != 3 or w.ndim != 2 or not np.issubdtype(w.dtype, np.integer) or m.shape[0] != w.shape[0] * w.shape[1] or not m.shape[0]:
        raise ValueError("sr [N W, S, S], weight [N, W] integers; got %s %s %s" % (m.shape, w.shape, w.dtype))
    w = w.astype(np.int64)
    if w.shape[1] > MAX_WINDOWS or w.min() < 0 or w.max() >= 2 ** 31 or (w.sum(1) <= 0).any():
        raise ValueError("at most %d windows; weights in [0, 2**31) with a positive sum per tile (they are multiplied by members up to 2**24 and "
                         "summed in 64-bit integers)" % MAX_WINDOWS)
    N, W = w.shape
    p = clip_rint_numpy(m, lo, hi).astype(np.int64).reshape(N, W, m.shape[1], m.shape[2])
    return round_half_even_div((w[:, :, None, None] * p).sum(1), w.sum(1)[:, None, None]).astype(np.float32)


def images_per_chunk(wspec, tspec, config, H, T_pre, budget=None):
    """Whole images per chunk so that the unfolded tiles (fp32 [n n, T_pre, win, win] per image), the W-fold network inputs
    ([n n, W, win, win, k]: the tiles' share times W k / T_pre) and the predictions ([n n W, S, S]) each stay under `budget` bytes; at
    least one.  tiles.images_per_chunk's rule, extended by the windows."""
    from . import tiles
    P, _, win, r, k, _ = tiles.geometry(config)
    n = tspec.n(P, H)
    W = wspec.windows
    per_image = 4 * n * n * max(T_pre * win * win, W * k * win * win, W * (r * P) ** 2)
    return max(1, int(tiles.CHUNK_BYTES if budget is None else budget) // per_image)

