"""FuseNet, stated in fp64 numpy: what csrc/kernels_fusenet.hip is held to (tests/test_gpu_fusenet.py).

The network is what the reference's ``FuseNetConv2D.build()`` builds (models/modelsTF.py:391-474, FuseNetv3), for x [B, H, W] in raw DN:

    y[b,c,r,s] = bias[c] + sum_{i,j in 0..47} x[b, r+i-23, s+j-23] K[i,j,0,c]      zero outside the image; TF 'SAME' with a filter of 48 pads
                                                                                    47 in total, 23 BEFORE and 24 AFTER, on both axes
    mu, var    = mean and biased variance of y[b,c,:,:]
    xhat       = (y - mu) / sqrt(var + 1e-3)         tensorflow_addons InstanceNormalization's default epsilon, restated from memory of TFA:
                                                     neither TFA nor TensorFlow is installed where this was written
    a          = gamma[c] xhat + beta[c];   l = a if a >= 0 else 0.3 a
    m[b,r,s]   = (1/64) sum_c l                      the branch
    out        = x + m

Backward for g = d loss / d out (no d loss / d x: the input is data):

    dl = g / 64;  da = dl (1 if a >= 0 else 0.3);  dbeta = sum_{b,p} da;  dgamma = sum_{b,p} da xhat;  dxhat = da gamma
    S1 = sum_p dxhat;  S2 = sum_p dxhat xhat;  dy = (dxhat - S1/N - xhat S2/N) / sqrt(var + 1e-3),  N = H W
    dK[i,j,0,c] = sum_b sum_{r,s} dy[b,c,r,s] x[b, r+i-23, s+j-23];   dbias = 0 exactly (the bias cancels in y - mu)

Two evaluations of the convolution and of dK: ``direct`` (a window view and one tensordot; memory H W 2304 doubles per sample) and ``fft``
(size-independent cost: the shipped 384 x 384 in seconds).  ``method=None`` takes fft from 96 pixels a side up.
"""
import numpy as np

KSIZE, FILTERS, PAD_BEFORE, EPS, LEAK = 48, 64, 23, 1e-3, 0.3
N_KERNEL = KSIZE * KSIZE * FILTERS
N_FLAT = N_KERNEL + 3 * FILTERS
NAMES = ("conv2d/kernel", "conv2d/bias", "instance_normalization/gamma", "instance_normalization/beta")
SHAPES = ((KSIZE, KSIZE, 1, FILTERS), (FILTERS,), (FILTERS,), (FILTERS,))


def split_flat(flat):
    """flat [147648] -> (K [48,48,1,64], bias, gamma, beta), views."""
    flat = np.asarray(flat).reshape(-1)
    if flat.size != N_FLAT:
        raise ValueError("flat buffer of %d values, expected %d" % (flat.size, N_FLAT))
    out, off = [], 0
    for shp in SHAPES:
        n = int(np.prod(shp))
        out.append(flat[off:off + n].reshape(shp))
        off += n
    return tuple(out)


def join_flat(K, bias, gamma, beta):
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in (K, bias, gamma, beta)])


def _method(H, W, method):
    if method is None:
        return "fft" if min(H, W) >= 96 else "direct"
    if method not in ("direct", "fft"):
        raise ValueError("method must be 'direct', 'fft' or None, got %r" % (method,))
    return method


def _padded(x):
    return np.pad(x, ((0, 0), (PAD_BEFORE, KSIZE - 1 - PAD_BEFORE), (PAD_BEFORE, KSIZE - 1 - PAD_BEFORE)))


def conv(x, K, method=None):
    """x [B,H,W], K [48,48,1,64] -> [B,64,H,W] fp64, without the bias."""
    x = np.asarray(x, dtype=np.float64)
    K2 = np.asarray(K, dtype=np.float64).reshape(KSIZE, KSIZE, FILTERS)
    B, H, W = x.shape
    xp = _padded(x)
    if _method(H, W, method) == "direct":
        win = np.lib.stride_tricks.sliding_window_view(xp, (KSIZE, KSIZE), axis=(1, 2))      # [B,H,W,48,48]
        return np.stack([np.tensordot(win[b], K2, axes=([2, 3], [0, 1])) for b in range(B)]).transpose(0, 3, 1, 2)
    fh, fw = H + KSIZE - 1, W + KSIZE - 1
    FX = np.fft.rfft2(xp, s=(fh, fw))                                                       # [B, fh, fw/2+1]
    FKc = np.conj(np.fft.rfft2(K2.transpose(2, 0, 1), s=(fh, fw)))                          # correlation: conj of the filter's transform
    out = np.empty((B, FILTERS, H, W))
    for b in range(B):
        out[b] = np.fft.irfft2(FX[b][None] * FKc, s=(fh, fw))[:, :H, :W]
    return out


def _filter_grad(dy, x, method=None):
    """dK[i,j,0,c] = sum_{b,r,s} dy[b,c,r,s] xpad[b,r+i,s+j]."""
    B, H, W = x.shape
    xp = _padded(np.asarray(x, dtype=np.float64))
    if _method(H, W, method) == "direct":
        win = np.lib.stride_tricks.sliding_window_view(xp, (KSIZE, KSIZE), axis=(1, 2))      # [B,H,W,48,48]
        dK = np.zeros((KSIZE, KSIZE, FILTERS))
        for b in range(B):
            dK += np.tensordot(win[b], dy[b], axes=([0, 1], [1, 2]))
        return dK.reshape(KSIZE, KSIZE, 1, FILTERS)
    fh, fw = H + KSIZE - 1, W + KSIZE - 1
    acc = np.zeros((FILTERS, fh, fw // 2 + 1), dtype=np.complex128)
    for b in range(B):
        acc += np.fft.rfft2(xp[b], s=(fh, fw))[None] * np.conj(np.fft.rfft2(dy[b], s=(fh, fw)))
    full = np.fft.irfft2(acc, s=(fh, fw))[:, :KSIZE, :KSIZE]                                # [c, i, j]
    return full.transpose(1, 2, 0).reshape(KSIZE, KSIZE, 1, FILTERS)


def forward(x, K, bias, gamma, beta, method=None):
    """-> dict: y [B,64,H,W] (with the bias), mu, var, rstd [B,64], xhat, a [B,64,H,W], m, out [B,H,W]."""
    x = np.asarray(x, dtype=np.float64)
    bias, gamma, beta = (np.asarray(v, dtype=np.float64).reshape(1, FILTERS, 1, 1) for v in (bias, gamma, beta))
    y = conv(x, K, method) + bias
    mu = y.mean(axis=(2, 3), keepdims=True)
    var = ((y - mu) ** 2).mean(axis=(2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (y - mu) * rstd
    a = gamma * xhat + beta
    m = np.where(a >= 0, a, LEAK * a).mean(axis=1)
    return dict(y=y, mu=mu[:, :, 0, 0], var=var[:, :, 0, 0], rstd=rstd[:, :, 0, 0], xhat=xhat, a=a, m=m, out=x + m)


def backward(g, x, K, bias, gamma, beta, gates=None, method=None, fwd=None):
    """g [B,H,W] = d loss / d out -> dict dK [48,48,1,64], dbias, dgamma, dbeta [64].
    gates (optional) [B,64,H,W]: the sign of `a` per element (True / non-zero where a >= 0) to evaluate the LeakyReLU's slope at, instead of this
    evaluation's own -- the gates of the leg being judged, as tests/input_grad_helpers.py does for the ReLU."""
    g = np.asarray(g, dtype=np.float64)
    f = fwd if fwd is not None else forward(x, K, bias, gamma, beta, method)
    pos = (f["a"] >= 0) if gates is None else (np.asarray(gates) != 0)
    N = g.shape[1] * g.shape[2]
    gam = np.asarray(gamma, dtype=np.float64).reshape(1, FILTERS, 1, 1)
    da = (g[:, None] / FILTERS) * np.where(pos, 1.0, LEAK)
    dbeta = da.sum(axis=(0, 2, 3))
    dgamma = (da * f["xhat"]).sum(axis=(0, 2, 3))
    dxhat = da * gam
    S1 = dxhat.sum(axis=(2, 3), keepdims=True)
    S2 = (dxhat * f["xhat"]).sum(axis=(2, 3), keepdims=True)
    dy = (dxhat - S1 / N - f["xhat"] * S2 / N) * f["rstd"][:, :, None, None]
    return dict(dK=_filter_grad(dy, np.asarray(x, dtype=np.float64), method), dbias=np.zeros(FILTERS), dgamma=dgamma, dbeta=dbeta, dy=dy)


def init_params(seed):
    """Keras's initial values as float32: kernel glorot_uniform (fan_in 2304, fan_out 147456), bias zeros, gamma and beta random_uniform
    (-0.05, 0.05) -- what the reference's layer arguments ask for (models/modelsTF.py:455-465)."""
    rng = np.random.default_rng(seed)
    limit = (6.0 / (KSIZE * KSIZE * 1 + KSIZE * KSIZE * FILTERS)) ** 0.5
    K = rng.uniform(-limit, limit, SHAPES[0]).astype(np.float32)
    gamma = rng.uniform(-0.05, 0.05, FILTERS).astype(np.float32)
    beta = rng.uniform(-0.05, 0.05, FILTERS).astype(np.float32)
    return K, np.zeros(FILTERS, np.float32), gamma, beta
