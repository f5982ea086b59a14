"""Shared pieces of the overlapped-tile tests: seeded registered frames with cloud blobs, the numpy pad + unfold, and the tile inputs stated
with the dataset builder's own functions on the host."""
import numpy as np

from probav_amd import prep

CONFIG = {"patch_size": 16, "max_shift": 6, "scale": 3, "num_low_res_imgs": 9, "num_low_res_imgs_pre": 9, "low_res_patch_thresholds": [0.85]}
HI = float(2 ** 16)


def cloudy_frames(images=3, T=9, H=128, seed=41):
    """Masked float64 [images, T, 1, H, H] in the form of trimmedArrayDir/<...>imgLR_<band>.npy (mask True = obscured): per image one corner that
    every frame has under cloud, one that none has, and two or three random discs per frame in between."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2 ** 14, (images, T, 1, H, H)).astype(np.float64)
    mask = np.zeros((images, T, 1, H, H), bool)
    yy, xx = np.mgrid[:H, :H]
    for i in range(images):
        for t in range(T):
            for _ in range(int(rng.integers(2, 4))):
                cy, cx, rad = rng.integers(30, H), rng.integers(30, H), rng.integers(8, 26)
                mask[i, t, 0] |= (yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2
            mask[i, t, 0, :30, :30] = False                         # clear in every frame
            mask[i, t, 0, H - 44:, H - 44:] = True                  # under cloud in every frame
    return np.ma.masked_array(data, mask=mask)


def numpy_unfold(frames, masks, pad, win, stride):
    """frames, masks [S, T, H, W] -> (patches float32 [S, P, T, win, win], masks bool, masked-pixel counts int32 [S, P, T]): np.pad 'reflect' and
    row-major windows, what probav_prep_patches computes."""
    fp = np.pad(np.asarray(frames, np.float32), ((0, 0), (0, 0), (pad, pad), (pad, pad)), "reflect")
    mp = np.pad(np.asarray(masks) != 0, ((0, 0), (0, 0), (pad, pad), (pad, pad)), "reflect")
    n = (fp.shape[2] - win) // stride + 1
    pt = np.stack([fp[:, :, a * stride:a * stride + win, c * stride:c * stride + win] for a in range(n) for c in range(n)], 1)
    pm = np.stack([mp[:, :, a * stride:a * stride + win, c * stride:c * stride + win] for a in range(n) for c in range(n)], 1)
    return pt, pm, pm.reshape(pm.shape[:3] + (-1,)).sum(-1).astype(np.int32)


def torch_unfold_seam(frames, masks, pad, win, stride):
    """`numpy_unfold` in the form tiles.build_tiles takes for its `unfold` seam (CPU tensors)."""
    import torch
    pt, _, pc = numpy_unfold(frames, masks, pad, win, stride)
    return torch.from_numpy(pt), torch.from_numpy(pc)


def masked_patches(unfolded):
    """(patches, masks, counts) of an unfold -> the masked array [S, P, T, 1, win, win] prep._patches returns (patchesDir's layout)."""
    pt, pm, _ = unfolded
    return np.ma.masked_array(pt[:, :, :, None], mask=pm[:, :, :, None])


def tile_inputs_by_the_builder(patches, config):
    """Stage 4 of the dataset builder and test.py's transpose, as written there: pickClearPatchesLR once per threshold, then
    np.array(...).transpose((0, 1, 4, 5, 2, 3)) -> float32 [S, P, win, win, T, 1]."""
    for thr in config["low_res_patch_thresholds"]:
        patches = prep.pickClearPatchesLR(patches, k=config["num_low_res_imgs"], clarityThreshold=thr)
    return np.array(patches).transpose((0, 1, 4, 5, 2, 3))


def synthetic_members(rng, rows, S):
    """Raw 'network output' for the blend: integers, exact halves before the rint, values below lo and above hi, a block of 65536."""
    sr = rng.integers(-3000, 2 ** 16 + 3000, (rows, S, S)).astype(np.float32)
    sr += rng.integers(0, 2, (rows, S, S)).astype(np.float32) * np.float32(0.5)
    sr[:, 1, :4] = np.array([0.5, 1.5, 2.5, -0.5], np.float32)
    sr[:, 2, :4] = np.array([65535.5, 65536.5, 1e9, -1e9], np.float32)
    sr[:, S // 2:S // 2 + 6, 3:S - 3] = HI
    sr[::3, 5:9] = rng.integers(0, 2 ** 16, (len(sr[::3]), 4, S)).astype(np.float32)          # plain integers
    return sr
