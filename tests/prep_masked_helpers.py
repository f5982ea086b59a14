"""Shared inputs of the masked registration's tests: seeded smooth scenes, frames cut from them at planted shifts (so nothing wraps
and the overlap of two frames is identical pixel for pixel), and saturated 'cloud' blocks flagged unclear in the mask."""
import numpy as np

N = 128
PAD = 40            # margin of the scene around the reference crop: planted shifts up to +-PAD


def scene(rng, lo=2000, hi=20000):
    """Smooth (1/f^1.5) texture on a (N + 2 PAD)^2 canvas."""
    n = N + 2 * PAD
    k = np.fft.fftfreq(n)
    t = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) / (1e-3 + np.hypot(k[:, None], k[None, :]) ** 1.5)).real
    t = (t - t.min()) / (t.max() - t.min())
    return (lo + t * (hi - lo)).astype(np.uint16)


def cut(sc, s=(0, 0)):
    """The frame whose registration shift against cut(sc) is s: frame[q] = reference[q + s], so frame[p - s] = reference[p]."""
    return sc[PAD + s[0]:PAD + s[0] + N, PAD + s[1]:PAD + s[1] + N].copy()


def cloud(frame, clear, y, x, h, w):
    """A saturated block, flagged unclear."""
    frame[y:y + h, x:x + w] = 65535
    clear[y:y + h, x:x + w] = False


def plain_circular_argmax(ref, img):
    """What the plain path ranks by (numpy fp64 FFT of the raw pixels): the argmax shift, indices > 64 wrapped to negative."""
    cc = np.fft.ifft2(np.fft.fft2(ref.astype(np.float64)) * np.conj(np.fft.fft2(img.astype(np.float64)))).real
    y, x = np.unravel_index(int(np.argmax(cc)), cc.shape)
    return (int(y) - N if y > N // 2 else int(y), int(x) - N if x > N // 2 else int(x))


def clouded_pair(seed, s):
    """The issue's construction: a smooth scene, the frame at planted shift s with one 50 x 60 flagged saturated block, the reference
    with one 30 x 40 flagged saturated block."""
    sc = scene(np.random.default_rng(seed))
    ref, img = cut(sc), cut(sc, s)
    rc, ic = np.ones((N, N), bool), np.ones((N, N), bool)
    cloud(img, ic, 20, 30, 50, 60)
    cloud(ref, rc, 60, 70, 30, 40)
    return ref, img, rc, ic


def random_clouds(rng, frame, clear, lo=0.10, hi=0.40):
    """Random flagged saturated blocks until between lo and hi of the frame is covered."""
    target = rng.uniform(lo + 0.02, hi - 0.05)
    while 1.0 - clear.mean() < target:
        h, w = int(rng.integers(16, 48)), int(rng.integers(16, 48))
        y, x = int(rng.integers(0, N - h)), int(rng.integers(0, N - w))
        if 1.0 - (clear.sum() - clear[y:y + h, x:x + w].sum()) / (N * N) > hi:
            continue
        cloud(frame, clear, y, x, h, w)
    assert lo <= 1.0 - clear.mean() <= hi
