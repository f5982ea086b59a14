"""Shared by tests/test_ssim_host.py and tests/test_gpu_ssim.py: the literal direct form of the cSSIM definition (x = m (P + bias), y = m H
built, then filtered), and the test scenes."""
import numpy as np


def _corr_valid(a, g, axis):
    """'valid' correlation with the 11 taps along one axis: scipy.ndimage.correlate1d when scipy imports, plain loops otherwise."""
    try:
        from scipy.ndimage import correlate1d
        full = correlate1d(a, g, axis=axis, mode="constant", cval=0.0)           # output i is centred on i: taps a[i - 5 .. i + 5]
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(5, a.shape[axis] - 5)
        return full[tuple(sl)]
    except ImportError:
        k = a.shape[axis] - 10
        a = np.moveaxis(a, axis, -1)
        out = np.zeros(a.shape[:-1] + (k,))
        for j in range(k):
            for q in range(11):
                out[..., j] += g[q] * a[..., j + q]
        return np.moveaxis(out, -1, axis)


def direct_table(sr, hr, mask, border):
    """The definition, literally: per shift build x and y, filter x, y, xx, yy, xy (rows first, then columns), average the SSIM map."""
    from probav_amd.scoring import gauss11
    g = gauss11()
    C1, C2 = (0.01 * 65535) ** 2, (0.03 * 65535) ** 2
    N, S = sr.shape[0], sr.shape[1]
    ns, L = 2 * border + 1, S - 2 * border
    F = lambda a: _corr_valid(_corr_valid(a, g, 1), g, 0)
    out = np.full((N, ns * ns), np.nan)
    for i in range(N):
        P = sr[i, border:border + L, border:border + L].astype(np.int64)
        for u in range(ns):
            for v in range(ns):
                H = hr[i, u:u + L, v:v + L].astype(np.int64)
                m = (mask[i, u:u + L, v:v + L] != 0).astype(np.int64)
                n, s1 = int(m.sum()), int((m * (H - P)).sum())
                if n == 0:
                    continue
                bias = np.float64(s1) / np.float64(n)
                x, y = m * (P + bias), (m * H).astype(np.float64)
                mx, my = F(x), F(y)
                vx, vy, cxy = F(x * x) - mx * mx, F(y * y) - my * my, F(x * y) - mx * my
                out[i, u * ns + v] = np.mean(((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2)))
    return out


def noise_case(N, S, bits, seed, p_clear=0.85):
    """16-bit noise images, a third of them uncorrelated (tests/test_gpu_score.py::_case)."""
    rng = np.random.default_rng(seed)
    top = 1 << bits
    hr = rng.integers(0, top, (N, S, S)).astype(np.uint16)
    sr = np.clip(hr.astype(np.int64) + rng.integers(-top // 8, top // 8, (N, S, S)), 0, 65535).astype(np.uint16)
    sr[::3] = rng.integers(0, top, sr[::3].shape)
    return sr, hr, rng.random((N, S, S)) < p_clear


def smooth_field(S, seed, pad=8):
    """Low-passed noise scaled to 2 000 .. 14 000, (S + 2 pad)^2 floats."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((S + 2 * pad + 4, S + 2 * pad + 4))
    k = np.ones(5) / 5.0                                     # a 5 x 5 box: smooth, yet a one-pixel shift still costs ~0.1 of SSIM
    a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="valid"), 1, a)
    a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="valid"), 0, a)
    return 2000.0 + 12000.0 * (a - a.min()) / (a.max() - a.min())


def planted_scene(S, seed, dy=1, dx=2, noise=100.0, bias=300.0, p_clear=1.0, pad=8):
    """(sr, hr, mask) [1, S, S]: HR a smooth field, SR the same field displaced by (dy, dx) plus N(0, noise) plus a bias, so that
    SR[i, j] = HR[i + dy, j + dx] + ...: with border b the crop P matches HR[u:, v:] at (u, v) = (b + dy, b + dx)."""
    f = smooth_field(S, seed, pad)
    rng = np.random.default_rng(seed + 1000)
    hr = np.rint(f[pad:pad + S, pad:pad + S])
    sr = np.rint(f[pad + dy:pad + dy + S, pad + dx:pad + dx + S] + rng.normal(0.0, noise, (S, S)) + bias)
    mask = rng.random((S, S)) < p_clear
    return sr.astype(np.uint16)[None], hr.astype(np.uint16)[None], mask[None]
