"""Shared by tests/test_refine_host.py and tests/test_gpu_refine.py: an independent restatement of probav_amd.prep.refine_masks_numpy as a
plain per-pixel loop, and the random ragged corpora both files draw."""
import numpy as np


def refine_plain(frames, clear, offsets, k16, floor, min_clear, dilate, saturation):
    """Steps 1 to 8 of the issue's statement, pixel by pixel, with `sorted` and Python integers only."""
    frames, clear = np.asarray(frames), np.asarray(clear) != 0
    F, H, W = frames.shape
    flag = [[[0] * W for _ in range(H)] for _ in range(F)]
    nsat, nout = [0] * F, [0] * F
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        for y in range(H):
            for x in range(W):
                xs = [int(frames[t, y, x]) for t in range(a, b)]
                cs = [bool(clear[t, y, x]) for t in range(a, b)]
                sat = [c and saturation is not None and v > saturation for v, c in zip(xs, cs)]
                c2 = [c and not st for c, st in zip(cs, sat)]
                vals = sorted(v for v, c in zip(xs, c2) if c)
                n = len(vals)
                out = [False] * (b - a)
                if n >= min_clear:
                    med = vals[(n - 1) // 2]
                    d = [abs(v - med) for v in xs]
                    mad = sorted(dd for dd, c in zip(d, c2) if c)[(n - 1) // 2]
                    scale = max(mad, floor)
                    out = [c and 16 * dd > k16 * scale for dd, c in zip(d, c2)]
                for i in range(b - a):
                    nsat[a + i] += bool(sat[i])
                    nout[a + i] += bool(out[i])
                    flag[a + i][y][x] = 1 if (sat[i] or out[i]) else 0
    res = np.zeros((F, H, W), bool)
    for f in range(F):
        for y in range(H):
            for x in range(W):
                g = any(flag[f][yy][xx] for yy in range(max(0, y - dilate), min(H, y + dilate + 1))
                        for xx in range(max(0, x - dilate), min(W, x + dilate + 1)))
                res[f, y, x] = bool(clear[f, y, x]) and not g
    return res, np.array([int(res[f].sum()) for f in range(F)], np.int32), np.array(list(zip(nsat, nout)), np.int32).reshape(F, 2)


def ragged(rng, sizes, H, W, alphabet=None, p_clear=0.5):
    """Sets of the given sizes: values from `alphabet` (a few symbols force ties) or the whole uint16 range, clear with probability p_clear."""
    F = int(sum(sizes))
    if alphabet is None:
        frames = rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    else:
        frames = np.asarray(alphabet, np.uint16)[rng.integers(0, len(alphabet), (F, H, W))]
    clear = rng.random((F, H, W)) < p_clear
    return frames, clear, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def scene_set(rng, T, H, W, noise=40, base=None):
    """T looks at one smooth scene plus uniform noise in [-noise, noise]: what a registered set looks like, all clear."""
    if base is None:
        yy, xx = np.mgrid[0:H, 0:W]
        base = 6000 + 37 * yy + 23 * xx + 500 * ((yy // 5 + xx // 7) % 3)
    return (base[None] + rng.integers(-noise, noise + 1, (T, H, W))).astype(np.uint16), base
