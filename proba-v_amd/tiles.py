"""Overlapped-tile inference: the tile grid, the blend windows, the numpy statement of the blend the device computes (csrc/kernels_tile.hip)
and the device-resident tile builder (testClass.resolve_tiled / resolve_tiled_frames drive them; INTEGRATION.md, 'Overlapped tiles').

test.py predicts a 384 x 384 image as an 8 x 8 grid of disjoint 48 x 48 predictions placed side by side, so every 48th row and column is a
seam.  Here the tiles overlap and are blended.  With P = patch_size, b = max_shift // 2, win = P + 2 b, r = scale, S = r P, H the LR frame
size and G = r H:

  stride  s is valid when 1 <= s <= P and (H - P) % s == 0; there are n = (H - P) / s + 1 tiles per axis; tile (a, c), row-major, has its
          LR core at (a s, c s) and its HR origin at (o_a, o_c) = (r a s, r c s).
  inputs  the dataset builder's own steps at stride s instead of P (build_tiles): reflect pad by b, win x win windows at stride s, then
          pickClearPatchesLR(k = num_low_res_imgs) per tile for every threshold of low_res_patch_thresholds, ties included, and test.py's
          transpose.  With s = P this is resolverDir/<...>patchesLR_<band>.npy element for element.
  tile    p_t = rint(clip(net(x_t), 0, 2**16)), an integer: what resolve_device returns (with an EnsembleSpec: resolve_ensemble(...,
          final="round") of the tile, one documented second rounding).
  window  a vector of S positive integers w[i], W2[i, j] = w[i] w[j];  "hat": w[i] = min(i, S - 1 - i) + 1,  "box": w[i] = 1.
  blend   for HR pixel (y, x), over the tiles t that cover it:  N = sum_t W2[y - o_a, x - o_c] p_t[y - o_a, x - o_c],
          D = sum_t W2[y - o_a, x - o_c],  out[y, x] = N / D rounded half to even in exact 64-bit integer arithmetic
          (q = N div D; compare 2 (N mod D) with D; ties to the even q).  fp32 [images, G, G] holding integers in [0, 65536].

Nothing is floating point after the tile's own rint, so the image does not depend on summation order, launch sets, kernel scheduling or
device; `tile_blend_numpy` equals the kernel bit for bit; with s = P every pixel has one tile and out = p_t, the plain path.
Every w[i] must lie in [1, 1024]: at most ceil(S / (r s))**2 <= S**2 tiles cover a pixel, so with S <= 90 and p <= 2**16,
N < 2**13 * 2**20 * 2**16 = 2**49.
"""
import numpy as np

from .intmath import clip_rint_numpy, round_half_even_div

WINDOWS = ("hat", "box")
MAX_WEIGHT = 1024
LR_SIZE = 128                  # PROBA-V LR frames
CHUNK_BYTES = 1 << 30          # budget of one chunk of whole images: its unfolded tiles and its predictions stay below this, each


def valid_strides(P, H):
    return [s for s in range(1, int(P) + 1) if (int(H) - int(P)) % s == 0]


def validate_window(w, S):
    """int32 [S] from any integer sequence; ValueError unless every entry lies in [1, 1024] (the bound that keeps the blend's 64-bit sums exact)."""
    a = np.asarray(w)
    if a.ndim != 1 or a.shape[0] != int(S) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("a window is a vector of S = %d integers, got shape %s dtype %s" % (S, a.shape, a.dtype))
    if a.min() < 1 or a.max() > MAX_WEIGHT:
        raise ValueError("window weights must lie in [1, %d] (they are multiplied pairwise and summed in 64-bit integers); got [%d, %d]"
                         % (MAX_WEIGHT, a.min(), a.max()))
    return np.ascontiguousarray(a, dtype=np.int32)


class TileSpec:
    """Which tiles of an image are predicted and how they are blended: LR `stride` between tile cores, `window` "hat" or "box" (or a vector
    of S integers in [1, 1024])."""

    def __init__(self, stride, window="hat"):
        if isinstance(window, str) and window not in WINDOWS:
            raise ValueError("window must be one of %s or a vector of integers, got %r" % (WINDOWS, window))
        self.stride, self.window = int(stride), window

    def validate(self, P, H):
        ok = valid_strides(P, H)
        if self.stride not in ok:
            raise ValueError("tile stride %d does not tile %d-pixel frames with %d-pixel cores: 1 <= s <= %d and (%d - %d) %% s == 0; valid strides: %s"
                             % (self.stride, H, P, P, H, P, ok))
        return self

    def n(self, P, H):
        """Tiles per axis."""
        self.validate(P, H)
        return (int(H) - int(P)) // self.stride + 1

    def weights(self, S):
        """The window as int32 [S]."""
        S = int(S)
        if isinstance(self.window, str):
            i = np.arange(S)
            w = np.minimum(i, S - 1 - i) + 1 if self.window == "hat" else np.ones(S, np.int64)
        else:
            w = self.window
        return validate_window(w, S)

    def origins(self, P, H, scale=1):
        """int64 [n n, 2]: the (row, column) origin of every tile in row-major order, in pixels of the `scale`-times enlarged image."""
        n = self.n(P, H)
        o = np.arange(n, dtype=np.int64) * (self.stride * int(scale))
        return np.stack(np.meshgrid(o, o, indexing="ij"), -1).reshape(n * n, 2)


def tile_blend_numpy(members, w, n, hr_stride, lo=0.0, hi=float(2 ** 16)):
    """The definition in numpy int64: members [images n n, S, S] (or [..., S, S, 1]; raw predictions or rounded ones), w [S] integers,
    tile (a, c) of an image at (a hr_stride, c hr_stride) -> float32 [images, G, G], G = (n - 1) hr_stride + S."""
    m = np.asarray(members, dtype=np.float32)
    if m.ndim == 4 and m.shape[3] == 1:
        m = m[..., 0]
    n, hs = int(n), int(hr_stride)
    if m.ndim != 3 or m.shape[1] != m.shape[2] or n < 1 or not m.shape[0] or m.shape[0] % (n * n):
        raise ValueError("members must be [images n n, S, S] with n = %d; got %s" % (n, m.shape))
    S, images = m.shape[1], m.shape[0] // (n * n)
    if not 1 <= hs <= S:
        raise ValueError("hr_stride = %d; 1 <= hr_stride <= S = %d (a gap between tiles would leave pixels without a weight)" % (hs, S))
    w = validate_window(w, S).astype(np.int64)
    W2 = w[:, None] * w[None, :]
    p = clip_rint_numpy(m, lo, hi).astype(np.int64).reshape(images, n, n, S, S)
    G = (n - 1) * hs + S
    N, D = np.zeros((images, G, G), np.int64), np.zeros((G, G), np.int64)
    for a in range(n):
        for c in range(n):
            N[:, a * hs:a * hs + S, c * hs:c * hs + S] += W2 * p[:, a, c]
            D[a * hs:a * hs + S, c * hs:c * hs + S] += W2
    return round_half_even_div(N, D).astype(np.float32)


# ---- the tile builder ---------------------------------------------------------------------------------------------------------------
def _device_unfold(frames, masks, pad, win, stride):
    from . import prep
    pt, _, pc = prep._device_patches(frames, masks, pad, win, stride)
    return pt, pc


def geometry(config):
    """(P, b, win, r, k, thresholds) of a parsed cfg."""
    P, b = int(config["patch_size"]), int(config["max_shift"]) // 2 if config["max_shift"] > 0 else 0
    return P, b, P + int(config["max_shift"]), int(config["scale"]), int(config["num_low_res_imgs"]), list(config["low_res_patch_thresholds"])


def select_frames(counts, pixels, k, thresholds):
    """counts [images, tiles, T_pre] masked pixels -> int64 [images, tiles, k]: the frames pickClearPatchesLR(k) keeps, applied once per
    threshold as stage 4 of the dataset builder chains it (the counts of the second and later thresholds are those of the selected frames).
    The selection itself is prep.clearFrameSelection, the index half of removeAndReplaceDirtyFrames."""
    from . import prep
    counts = np.asarray(counts, np.int64)
    images, tiles = counts.shape[:2]
    rows = np.arange(tiles)[:, None]
    idx = np.tile(np.arange(counts.shape[2], dtype=np.int64), (images, tiles, 1))
    for thr in thresholds:
        nxt_idx, nxt_cnt = [], []
        for i in range(images):
            sel = prep.clearFrameSelection(counts[i], pixels, k, thr)[0]
            nxt_idx.append(idx[i][rows, sel])
            nxt_cnt.append(counts[i][rows, sel])
        idx, counts = np.stack(nxt_idx), np.stack(nxt_cnt)
    return idx


def build_tiles(imgsLR_masked, spec, config, device=None, unfold=None):
    """Registered, trimmed LR frames (trimmedArrayDir/<TEST|TRAIN>imgLR_<band>.npy: masked [images, T_pre, 1, H, H]) -> the network inputs of
    every tile, fp32 [images, n n, win, win, T, 1] on `device`.  The pad + unfold is the builder's kernel (probav_prep_patches) at stride
    s; only its counts [images, n n, T_pre] come to the host, where the frames of every tile are chosen (select_frames); the frame gather
    and the change of layout are torch indexing on the device.  `unfold` (frames, masks, pad, win, stride) -> (patches [images, tiles,
    T_pre, win, win], counts) replaces the device unfold (the tests put numpy's there).  Callers bound the number of images per call
    (images_per_chunk)."""
    import torch
    S_, T_pre, C, H, W = imgsLR_masked.shape
    if C != 1 or H != W:
        raise ValueError("square greyscale frames [images, T, 1, H, H] expected, got %s" % (imgsLR_masked.shape,))
    P, b, win, _, k, thresholds = geometry(config)
    n = spec.n(P, H)
    data = np.ma.getdata(imgsLR_masked).reshape(S_, T_pre, H, W)
    mask = np.ma.getmaskarray(imgsLR_masked).reshape(S_, T_pre, H, W)
    pt, pc = (_device_unfold if unfold is None else unfold)(data, mask, b, win, spec.stride)
    if tuple(pt.shape) != (S_, n * n, T_pre, win, win):
        raise RuntimeError("the unfold returned %s, expected %s" % (tuple(pt.shape), (S_, n * n, T_pre, win, win)))
    idx = select_frames(pc.cpu().numpy(), win * win, k, thresholds)
    if device is not None:
        pt = pt.to(device)
    gi = torch.from_numpy(idx).to(pt.device)                                                   # [images, tiles, T]
    sel = torch.gather(pt, 2, gi[:, :, :, None, None].expand(-1, -1, -1, win, win))            # [images, tiles, T, win, win]
    return sel.permute(0, 1, 3, 4, 2).contiguous().unsqueeze(-1)                               # test.py:67's transpose


def images_per_chunk(spec, config, H, T_pre, budget=CHUNK_BYTES):
    """Whole images per chunk so that neither the unfolded tiles (fp32 [n n, T_pre, win, win] per image) nor the predictions of a chunk
    ([n n, S, S] fp32 per image) exceed `budget` bytes; at least one."""
    P, _, win, r, _, _ = geometry(config)
    n = spec.n(P, H)
    per_image = 4 * n * n * max(T_pre * win * win, (r * P) ** 2)
    return max(1, int(budget) // per_image)

