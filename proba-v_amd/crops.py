"""Training on random crops of the registered scenes, cut on the device (csrc/kernels_crops.hip; INTEGRATION.md, 'Random crops').

The dataset builder cuts training patches on a fixed grid (stage 3: `patch_stride`), picks their frames (stage 4) and dumps them (stage 5):
with patch_size = patch_stride = 16 that is 64 of the 113 x 113 = 12 769 origins a 16-pixel patch can take in a 128 x 128 scene.  Here the
scenes of trimmedArrayDir stay on the device and every training sample is cut out of them when it is needed, at any origin.  From the cfg:

    P = patch_size, pad = max_shift // 2, win = P + max_shift, r = scale, k = num_low_res_imgs, T_pre = num_low_res_imgs_pre,
    one patch threshold (frame_windows.single_threshold; several are a ValueError, as there).

The scenes: LR [S, T_pre, H, H] with masks (1 = masked), HR [S, r H, r H] with masks.

  position  (s, y, x), 0 <= y, x <= H - P.  The LR window is rows y .. y + win - 1, columns x .. x + win - 1 of the scene padded by `pad` with
            np.pad(..., 'reflect'), data and mask alike (stage 3); the HR window is rows r y .. r y + r P - 1, columns likewise.
  valid     iff the HR window's masked-pixel count c < L_hr = max_masked((r P)**2, high_res_threshold): the net effect of
            removeCorruptedTrainPatchSets and pickClearPatches.  LR never invalidates a patch, as in the builder.
  frames    counts[t] = the masked pixels of frame t of the LR window; Q = window 0 of frame_windows_select_numpy(counts, win**2, k,
            L = max_masked(win**2, threshold), W = 1): the builder's k frames (removeAndReplaceDirtyFrames), ties broken by the frame index.
  sample    lr[:, :, i] = frame Q[perm[i]], then flip f, then q quarter turns, exactly as augment.apply_recipe_numpy does; HR and its
            clear-mask get the same flip and turns.  A recipe row is int32 [3 + k] = {j, f, q, perm[0..k)}, j an index into the position list.
  outputs   what augment.DeviceDataset.batch returns -- LR [B, win, win, k, 1] fp32, HR [B, rP, rP, 1] fp32, clear-mask [B, rP, rP, 1] in
            its own dtype (1 = clear) -- and sel [B, k] int32, the chosen frames Q[0 .. k) (before the recipe's frame order).

Bits are moved, never computed with.  `window_counts_numpy` and `crop_batch_numpy` are the statements the two kernels are tested against
(bit for bit); crop_batch_numpy is a composition of statements the repository already has: pad and slice, frame_windows_select_numpy,
apply_recipe_numpy.

`CropSpec("grid")` keeps the valid positions with y, x multiples of patch_stride in the builder's (scene, row, column) order and walks
them through augment.virtual_index_batches exactly as --online-aug walks its base set: the tensors are those of --online-aug on the
builder's patches of the same scenes (where the eligible counts of a window are pairwise distinct; ties: frame_windows.py).
`CropSpec("all")` draws j, f, q and perm independently and uniformly per sample.
"""
import numpy as np

from . import augment
from .frame_windows import MAX_POOL, frame_windows_select_numpy, max_masked, single_threshold

POSITIONS = ("all", "grid")


class CropGeometry:
    """The integers of the definition for one parsed cfg."""

    def __init__(self, config):
        self.P, self.max_shift = int(config["patch_size"]), int(config["max_shift"])
        if self.P < 1 or self.max_shift < 0 or self.max_shift % 2:
            raise ValueError("random crops need patch_size >= 1 and an even max_shift >= 0 (the window P + max_shift is the core plus a reflect pad of "
                             "max_shift // 2 on either side); got patch_size = %d, max_shift = %d" % (self.P, self.max_shift))
        self.pad, self.win = self.max_shift // 2, self.P + self.max_shift
        self.r, self.k, self.T_pre = int(config["scale"]), int(config["num_low_res_imgs"]), int(config["num_low_res_imgs_pre"])
        self.stride = int(config.get("patch_stride", self.P))
        if not 1 <= self.k <= MAX_POOL or not 1 <= self.T_pre <= MAX_POOL or self.r < 1 or self.stride < 1:
            raise ValueError("k = %d, T_pre = %d, scale = %d, patch_stride = %d; 1 <= k, T_pre <= %d, scale, patch_stride >= 1"
                             % (self.k, self.T_pre, self.r, self.stride, MAX_POOL))
        self.threshold = single_threshold(config)
        self.L = max_masked(self.win ** 2, self.threshold)
        self.L_hr = max_masked((self.r * self.P) ** 2, float(config["high_res_threshold"]))

    @property
    def side(self):
        return self.r * self.P


class CropSpec:
    """Which positions a trainer draws from and how: "grid" (the builder's patch grid, walked like --online-aug's base set) or "all" (every valid
    origin, drawn uniformly from np.random.default_rng([seed, rank]))."""

    def __init__(self, positions="all", seed=0):
        if positions not in POSITIONS:
            raise ValueError("positions must be one of %s, got %r" % (POSITIONS, positions))
        self.positions, self.seed = positions, int(seed)


# ---- numpy statements -------------------------------------------------------------------------------------------------------------------
def window_counts_numpy(masks, pad, win, stride):
    """masks [M, H, W] (nonzero = masked) -> int32 [M, ny, nx]: the masked pixels of every win x win window at `stride` of the masks padded by
    `pad` with np.pad 'reflect'; ny = (H + 2 pad - win) // stride + 1.  An integral image, exact."""
    m = np.asarray(masks) != 0
    pad, win, stride = int(pad), int(win), int(stride)
    if m.ndim != 3 or not 0 <= pad < min(m.shape[1:]) or stride < 1 or not 1 <= win <= min(m.shape[1:]) + 2 * pad:
        raise ValueError("masks [M, H, W], 0 <= pad < min(H, W), 1 <= win <= min(H, W) + 2 pad, stride >= 1; got %s pad %d win %d stride %d"
                         % (m.shape, pad, win, stride))
    p = np.pad(m, ((0, 0), (pad, pad), (pad, pad)), "reflect").astype(np.int64)
    I = np.zeros((p.shape[0], p.shape[1] + 1, p.shape[2] + 1), np.int64)
    I[:, 1:, 1:] = p.cumsum(1).cumsum(2)
    ys, xs = np.arange(0, p.shape[1] - win + 1, stride), np.arange(0, p.shape[2] - win + 1, stride)
    a, b = np.ix_(ys, xs)
    return (I[:, a + win, b + win] - I[:, a, b + win] - I[:, a + win, b] + I[:, a, b]).astype(np.int32)


def valid_table_numpy(hr_mask, geom):
    """HR masks [S, r H, r H] (nonzero = masked) -> bool [S, H - P + 1, H - P + 1]: position (s, y, x) is valid."""
    return window_counts_numpy(hr_mask, 0, geom.side, geom.r) < geom.L_hr


def positions_from_table(valid, stride=1):
    """bool [S, n, n] -> int32 [V, 3] rows {scene, y, x} in (scene, row, column) order; stride > 1 keeps the origins that are multiples of it."""
    v = np.asarray(valid)[:, ::stride, ::stride]
    return (np.argwhere(v) * np.array([1, stride, stride])).astype(np.int32)


def lr_window_counts_numpy(lr_mask, positions, geom):
    """int64 [n, T_pre]: the masked pixels of every frame of the LR window of every position (what the kernel ranks)."""
    out = np.empty((len(positions), np.shape(lr_mask)[1]), np.int64)
    for n, (s, y, x) in enumerate(np.asarray(positions)):
        mp = np.pad(np.asarray(lr_mask[s]) != 0, ((0, 0), (geom.pad, geom.pad), (geom.pad, geom.pad)), "reflect")
        out[n] = mp[:, y:y + geom.win, x:x + geom.win].reshape(mp.shape[0], -1).sum(-1)
    return out


def crop_batch_numpy(lr, lr_mask, hr, hr_clear, positions, recipe, geom):
    """The recipe's meaning in numpy, sample by sample -> (lr_b [B, win, win, k, 1] float32, hr_b [B, rP, rP, 1] float32, mask_b [B, rP, rP, 1],
    sel int32 [B, k]).  lr / lr_mask [S, T_pre, H, H], hr / hr_clear [S, r H, r H], positions [V, 3]; nothing on the training path calls it."""
    g, pw = geom, ((0, 0), (geom.pad, geom.pad), (geom.pad, geom.pad))
    lr, hr, hr_clear = np.asarray(lr, np.float32), np.asarray(hr, np.float32), np.asarray(hr_clear)
    outs, sels = ([], [], []), []
    for row in np.asarray(recipe):
        s, y, x = (int(v) for v in np.asarray(positions)[int(row[0])])
        data = np.pad(lr[s], pw, "reflect")[:, y:y + g.win, x:x + g.win]
        mask = np.pad(np.asarray(lr_mask[s]) != 0, pw, "reflect")[:, y:y + g.win, x:x + g.win]
        counts = mask.reshape(mask.shape[0], -1).sum(-1)
        Q = frame_windows_select_numpy(counts[None], g.win ** 2, g.k, g.L, 1, 1)[0][0, 0]
        sels.append(Q)
        hs = (slice(g.r * y, g.r * y + g.side), slice(g.r * x, g.r * x + g.side))
        base = (data[Q].transpose(1, 2, 0)[None, ..., None], hr[s][hs][None, ..., None], hr_clear[s][hs][None, ..., None])
        one = np.concatenate([[0], row[1:]])[None]                                  # the same row over a base set of this one window
        for o, a in zip(outs, augment.apply_recipe_numpy(*base, one)):
            o.append(a[0])
    return tuple(np.stack(o) for o in outs) + (np.stack(sels).astype(np.int32),)


# ---- recipes ----------------------------------------------------------------------------------------------------------------------------
def validate_recipe(recipe, V, k):
    """ValueError unless every row {j, f, q, perm[0..k)} can be applied to a list of V positions and k frames."""
    augment.validate_recipe(recipe, V, k)


def random_recipes(V, k, aug, spec, rank, batchSize, steps):
    """The "all" sampler: `steps` recipes [batchSize, 3 + k] with j, f, q and perm drawn independently and uniformly per sample from
    np.random.default_rng([seed, rank]); the codes only where the cfg enables them, the permutation only when num_low_res_permute > 0."""
    rng = np.random.default_rng([spec.seed, int(rank)])
    ident = np.broadcast_to(np.arange(k), (batchSize, k))
    for _ in range(int(steps)):
        r = np.zeros((batchSize, 3 + k), np.int32)
        r[:, 0] = rng.integers(0, V, batchSize)
        if aug.flip:
            r[:, 1] = rng.integers(0, 4, batchSize)
        if aug.rotate:
            r[:, 2] = rng.integers(0, 4, batchSize)
        r[:, 3:] = rng.permuted(ident, axis=1) if aug.numPermute > 0 else ident
        yield r


def steps_per_epoch(n_grid, aug, batchSize, world=1, crops_per_epoch=None):
    """len(grid positions) x multiplicity // batch in both modes (an epoch means what it meant), per rank; or crops_per_epoch // batch."""
    n = n_grid * aug.multiplicity if crops_per_epoch is None else int(crops_per_epoch)
    return (n // world) // batchSize


# ---- the scenes on the device -------------------------------------------------------------------------------------------------------------
class CropDataset:
    """The scenes on the device, uploaded once, the validity table of every origin (probav::window_counts on the HR masks) and the two
    device-resident position lists made from it (torch.nonzero; only their lengths come to the host): `positions` (every valid origin,
    __len__ = V) and `grid_positions` (those on the builder's grid).  A batch is one kernel launch (probav::crop_batch).  There is no host path:
    a device that is not a HIP device is refused, and a scene set that does not fit raises with the number of bytes asked for.

    lr [S, T_pre, H, H], hr [S, r H, r H]; lr_mask, hr_mask: True / nonzero = masked, as the builder's masked arrays have it."""

    def __init__(self, lr, lr_mask, hr, hr_mask, config, device):
        import torch
        from . import ops                                 # noqa: F401  (registers torch.ops.probav.window_counts / crop_batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CropDataset lives on %s: samples are cut by a HIP kernel on a gfx950 device (no CPU fallback)" % self.device)
        self.geom = g = CropGeometry(config)
        lr, lr_mask, hr, hr_mask = np.asarray(lr), np.asarray(lr_mask), np.asarray(hr), np.asarray(hr_mask)
        if lr.ndim != 4 or lr.shape[2] != lr.shape[3] or lr_mask.shape != lr.shape or hr.ndim != 3 or hr_mask.shape != hr.shape or not len(lr) == len(hr) >= 1:
            raise ValueError("expected LR and its mask [S, T_pre, H, H], HR and its mask [S, r H, r H] with S >= 1; got %s %s %s %s"
                             % (lr.shape, lr_mask.shape, hr.shape, hr_mask.shape))
        self.S, self.T_pre, self.H = lr.shape[0], lr.shape[1], lr.shape[2]
        if hr.shape[1:] != (g.r * self.H, g.r * self.H) or self.T_pre != g.T_pre or not g.P <= self.H or g.pad >= self.H:
            raise ValueError("the scenes do not match the cfg: LR %s, HR %s; scale %d, num_low_res_imgs_pre %d, patch_size %d, max_shift %d (square scenes only)"
                             % (lr.shape, hr.shape, g.r, g.T_pre, g.P, g.max_shift))
        host = (np.ascontiguousarray(lr, dtype=np.float32), np.ascontiguousarray(lr_mask != 0).view(np.uint8),
                np.ascontiguousarray(hr, dtype=np.float32), np.ascontiguousarray(hr_mask == 0))              # the last: the CLEAR mask, bool
        self.nbytes = sum(a.nbytes for a in host)
        try:
            self.lr, self.lr_mask, self.hr, self.hr_clear = (torch.from_numpy(a).to(self.device) for a in host)
            with torch.cuda.device(self.device):
                counts = torch.ops.probav.window_counts((~self.hr_clear).view(torch.uint8), 0, g.side, g.r)
            self.valid = counts < g.L_hr                                                                        # bool [S, n, n]
            self.positions = torch.nonzero(self.valid).to(torch.int32).contiguous()
            scale = torch.tensor([1, g.stride, g.stride], dtype=torch.int32, device=self.device)
            self.grid_positions = (torch.nonzero(self.valid[:, ::g.stride, ::g.stride]).to(torch.int32) * scale).contiguous()
        except torch.OutOfMemoryError as exc:
            raise MemoryError("the scenes do not fit on %s: %d bytes were asked for (%d scenes; LR %d, LR masks %d, HR %d, HR masks %d bytes). "
                              "There is no host-memory fallback: train from the builder's patches, or on fewer scenes."
                              % (self.device, self.nbytes, self.S, host[0].nbytes, host[1].nbytes, host[2].nbytes, host[3].nbytes)) from exc
        self.V, self.n_grid = int(self.positions.shape[0]), int(self.grid_positions.shape[0])
        self._upload = augment.RecipeUploader(self.device)

    def __len__(self):
        return self.V

    def count(self, spec):
        return self.n_grid if spec.positions == "grid" else self.V

    def batch_from_recipe(self, recipe, positions="all", with_sel=False):
        """(lr_b, hr_b, mask_b[, sel]) device tensors of a host recipe [B, 3 + k] over the "all" or the "grid" list; validated here, before anything is launched."""
        import torch
        g = self.geom
        if positions not in POSITIONS:
            raise ValueError("positions must be one of %s, got %r" % (POSITIONS, positions))
        table = self.grid_positions if positions == "grid" else self.positions
        if not len(table):
            raise ValueError("no valid %s position in %d scenes: every HR window misses high_res_threshold" % (positions, self.S))
        validate_recipe(recipe, len(table), g.k)
        with torch.cuda.device(self.device):
            out = torch.ops.probav.crop_batch(self.lr, self.lr_mask, self.hr, self.hr_clear, table, self._upload(np.asarray(recipe, dtype=np.int32)),
                                              g.P, g.pad, g.win, g.r, g.L)
        return out if with_sel else out[:3]

    def batches(self, spec, aug, batchSize, steps=None, rank=0, world=1, epochs=1, bufferSize=256, rng=None):
        """Training batches.  "grid": the virtual set of len(grid) x multiplicity elements walked by augment.virtual_index_batches (rank's shard,
        shuffle, repeat, batch), as --online-aug walks its base set.  "all": `steps` batches of the uniform sampler."""
        if spec.positions == "grid":
            _, virtual = augment.virtual_index_batches(self.n_grid * aug.multiplicity, rank, world, epochs, batchSize, bufferSize,
                                                       np.random.default_rng(0) if rng is None else rng)
            for n, v in enumerate(virtual):
                if steps is not None and n >= steps:
                    return
                yield self.batch_from_recipe(augment.make_recipe(v, self.n_grid, self.geom.k, aug), "grid")
        else:
            if steps is None:
                steps = steps_per_epoch(self.n_grid, aug, batchSize, world) * epochs
            for r in random_recipes(self.V, self.geom.k, aug, spec, rank, batchSize, steps):
                yield self.batch_from_recipe(r, "all")


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
def load_scenes(config, band, indices=None):
    """trimmedArrayDir's training scenes as test.py --tile-stride reads them -> (lr [S, T_pre, H, H], lr_mask, hr [S, r H, r H], hr_mask), masks
    True = masked; `indices`: the scenes to keep (TRAINscenes_<band>.npy of `utils/dataGenerator.py --scene-split`)."""
    import os
    d = os.path.join(config["preprocessing_out"], "trimmedArrayDir")
    lr = np.load(os.path.join(d, "TRAINimgLR_%s.npy" % band), allow_pickle=True)
    hr = np.load(os.path.join(d, "TRAINimgHR_%s.npy" % band), allow_pickle=True)
    if lr.ndim != 5 or lr.shape[2] != 1 or hr.ndim != 5 or hr.shape[1:3] != (1, 1) or len(lr) != len(hr):
        raise ValueError("expected TRAINimgLR [S, T_pre, 1, H, H] and TRAINimgHR [S, 1, 1, r H, r H]; got %s %s" % (lr.shape, hr.shape))
    if indices is not None:
        lr, hr = lr[np.asarray(indices)], hr[np.asarray(indices)]
    return (np.ma.getdata(lr)[:, :, 0], np.ma.getmaskarray(lr)[:, :, 0], np.ma.getdata(hr)[:, 0, 0], np.ma.getmaskarray(hr)[:, 0, 0])


def scene_split(S, split):
    """(validation scenes, training scenes): RandomState(17).permutation(S), the first ceil(split S) are validation (the patch split's rule,
    prep.splitPatches, on whole scenes)."""
    import math
    perm = np.random.RandomState(17).permutation(int(S))
    n_val = math.ceil(split * S)
    return perm[:n_val], perm[n_val:]
