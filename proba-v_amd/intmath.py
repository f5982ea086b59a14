"""The integer image arithmetic of the numpy statements, once: csrc/image_math.h is the device's form (tiles.tile_blend_numpy,
frame_windows.frame_windows_reduce_numpy, ensemble.ensemble_reduce_numpy and baseline.baseline_numpy use these)."""
import numpy as np


def clip_rint_numpy(m, lo, hi):
    """probav_clip_round's arithmetic on float32: clip to [lo, hi], round half to even.  fmax drops a NaN as the device's fmaxf does, so NaN
    goes to lo ('Non-finite values')."""
    return np.rint(np.fmin(np.fmax(np.asarray(m, np.float32), np.float32(lo)), np.float32(hi)))


def round_half_even_div(N, D):
    """N / D rounded half to even, in integers (D > 0, any sign of N): floor division, then 2 (N mod D) against D."""
    N, D = np.asarray(N, np.int64), np.asarray(D, np.int64)
    if (D <= 0).any():
        raise ValueError("round_half_even_div: D must be positive")
    q = N // D                                                         # floor
    r = N - q * D                                                      # 0 <= r < D
    up = (2 * r > D) | ((2 * r == D) & (q % 2 != 0))
    return q + up
