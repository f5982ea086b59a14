"""Shared pieces of the random-crop tests: the small scene set of the issue (H = 10, P = 4, max_shift = 2, r = 3, T_pre = 5, k = 3) whose eligible
frame counts are pairwise distinct in every grid patch, scene sets with the frame-choice edge cases built in, and the builder's own patches
of a scene set (stages 3 and 4 as prep.main runs them)."""
import numpy as np

from probav_amd import crops, prep

SMALL_CFG = {"patch_size": 4, "patch_stride": 4, "max_shift": 2, "scale": 3, "num_low_res_imgs": 3, "num_low_res_imgs_pre": 5,
             "low_res_patch_thresholds": [0.5], "high_res_threshold": 0.6, "num_low_res_permute": 2, "to_flip": True, "to_rotate": True,
             "split": 0.25}
SHIPPED_CFG = {"patch_size": 16, "patch_stride": 16, "max_shift": 6, "scale": 3, "num_low_res_imgs": 9, "num_low_res_imgs_pre": 9,
               "low_res_patch_thresholds": [0.85], "high_res_threshold": 0.85, "num_low_res_permute": 2, "to_flip": True, "to_rotate": True,
               "split": 0.2}


def bits(rng, shape):
    """float32 with arbitrary bit patterns (NaN payloads, denormals, infinities included): the kernels move bits."""
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def scenes(config, S, H, seed, lr_density=None, hr_density=0.2, integers=False):
    """(lr [S, T_pre, H, H] float32, lr_mask bool, hr [S, rH, rH] float32, hr_mask bool), masks True = masked.  Frame t of every scene is masked
    with its own density (default 0.04 + 0.11 t: the frames differ in clarity, as registered frames do)."""
    rng = np.random.default_rng(seed)
    T, r = config["num_low_res_imgs_pre"], config["scale"]
    dens = 0.04 + 0.11 * np.arange(T) if lr_density is None else np.broadcast_to(lr_density, (T,))
    if integers:
        lr, hr = rng.integers(0, 2 ** 14, (S, T, H, H)).astype(np.float32), rng.integers(0, 2 ** 14, (S, r * H, r * H)).astype(np.float32)
    else:
        lr, hr = bits(rng, (S, T, H, H)), bits(rng, (S, r * H, r * H))
    lr_mask = rng.random((S, T, H, H)) < dens[None, :, None, None]
    hr_mask = rng.random((S, r * H, r * H)) < hr_density
    return lr, lr_mask, hr, hr_mask


def distinct_scenes(config, S, H, first_seed=0):
    """S scenes (`scenes(..., integers=True)`, each of the first seed at which it holds) whose eligible counts are pairwise distinct in every grid
    patch: where they are not, np.argsort in the builder is unspecified (frame_windows.py) and the builder's choice is not a function of the
    counts.  The frame densities put every frame's expected count below the limit, a step apart.  -> (seeds, (lr, lr_mask, hr, hr_mask))."""
    g = crops.CropGeometry(config)
    n = (H - g.P) // g.stride + 1
    grid = np.array([(0, a * g.stride, c * g.stride) for a in range(n) for c in range(n)], np.int32)
    T = config["num_low_res_imgs_pre"]
    dens = (0.5 + np.arange(T)) * (g.L / (T + 1.0)) / g.win ** 2
    seeds, parts = [], []
    for s in range(S):
        for seed in range(first_seed + 1000 * s, first_seed + 1000 * (s + 1)):
            sc = scenes(config, 1, H, seed, lr_density=dens, integers=True)
            if eligible_counts_distinct(crops.lr_window_counts_numpy(sc[1], grid, g), g.L):
                break
        else:
            raise AssertionError("scene %d: no seed gives pairwise distinct eligible counts" % s)
        seeds.append(seed)
        parts.append(sc)
    return seeds, tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def eligible_counts_distinct(counts, L):
    for c in np.asarray(counts):
        e = c[c < L] if (c < L).any() else c
        if len(np.unique(e)) != len(e):
            return False
    return True


def edge_scenes(config, H, seed, integers=False):
    """Four scenes for the frame-choice edge cases: scene 0 clear in every frame (all counts equal: the index tie-break), scene 1 masked in every
    frame (no eligible frame), scene 2 clear in frames 0 and 1 only (E = 2 < k: the list is tiled), scene 3 random."""
    lr, lr_mask, hr, hr_mask = scenes(config, 4, H, seed, integers=integers)
    lr_mask[0] = False
    lr_mask[1] = True
    lr_mask[2, :2] = False
    lr_mask[2, 2:] = True
    return lr, lr_mask, hr, hr_mask


def masked_scene_arrays(lr, lr_mask, hr, hr_mask):
    """The masked arrays of trimmedArrayDir: TRAINimgLR [S, T_pre, 1, H, H] float64, TRAINimgHR [S, 1, 1, rH, rH]."""
    return (np.ma.masked_array(np.asarray(lr, np.float64)[:, :, None], mask=np.asarray(lr_mask)[:, :, None]),
            np.ma.masked_array(np.asarray(hr, np.float64)[:, None, None], mask=np.asarray(hr_mask)[:, None, None]))


def builder_patches(lr_m, hr_m, config):
    """Stages 3 and 4 of prep.main on masked scenes, as written there -> (LR [N, win, win, k, 1] masked, HR [N, rP, rP, 1] masked): the content of
    trimmedPatchesDir/TRAINpatches{LR,HR}.  The unfold is prep._patches (the device's, unless the caller has put numpy's in its place)."""
    pad = config["max_shift"] // 2 if config["max_shift"] > 0 else 0
    win = config["patch_size"] + config["max_shift"]
    H = lr_m.shape[3]
    train = prep._patches(lr_m, win, config["patch_stride"], pad)[0]
    khr = config["patch_size"] * (hr_m.shape[3] // H)
    hr = prep._patches(hr_m, khr, khr, 0)[0]
    for thr in config["low_res_patch_thresholds"]:
        train = prep.pickClearPatchesLR(train, k=config["num_low_res_imgs"], clarityThreshold=thr)
    train, hr = prep.removeCorruptedTrainPatchSets(train, hr, config["high_res_threshold"])
    train, hr = prep.pickClearPatches(train, hr, config["high_res_threshold"])
    return train.transpose((0, 3, 4, 1, 2)), hr.transpose((0, 3, 4, 1, 2)).squeeze(4)


def numpy_device_patches(frames, masks, pad, win, stride):
    """prep.device_patches in numpy (tests/tiles_helpers.numpy_unfold): the stub the host tests put in its place."""
    from tests.tiles_helpers import numpy_unfold
    return numpy_unfold(frames, masks, pad, win, stride)
