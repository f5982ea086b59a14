"""fp64 numpy restatement of the reference's WDSR-B Conv3D network and shift-compensated losses.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py) -- PARITY UNPINNED: TensorFlow / TFA cannot be
run here, so this follows the reference source line by line instead of its outputs.

Every function cites the reference lines it restates (paths relative to /root/reference).
Tensor layout is the reference's: activations [N, H, W, T, C], kernels [kh, kw, kt, Cin, Cout]
(2-D: [kh, kw, Cin, Cout]); the three Conv3D "spatial" axes are (H, W, T).

Written with explicit tap loops + einsum so that it shares no code path with the torch
restatement (oracle/wdsr_torch.py) it is cross-checked against.
"""
import numpy as np

F64 = np.float64


# ----------------------------------------------------------------------------------------------
# architecture tables
# ----------------------------------------------------------------------------------------------
def reducer_plan(numImgLR):
    """(k, pad_hw, pad_t) of the valid k*k*k `convReducer_i` layers, per temporal depth; every pad is a
    tf.pad(mode='reflect').

    models/modelsTF.py:62-69 selects the reducer by numImgLR:
      9  -> ConvReduceAndUpscale   (:152-164)  numImgLR//scale = 3 reducers, reflect pad H,W only before the first
      13 -> ConvReduceAndUpscalev3 (:123-150)  5 reducers, reflect pad before the first three
      7  -> ConvReduceAndUpscalev2 (:166-175)  2 reducers, no pad
      19 -> ConvReduceAndUpscaleEx (:76-121, EXPERIMENTAL there)  10 reducers; the first is 5x5x5 on a reflect pad of 2 on
            H, W and T, the second pads (2,2,1), the third and fourth (2,2,0), the fifth (1,1,0), the rest none
    """
    a, b = (3, 1, 0), (3, 0, 0)
    if numImgLR == 9:
        return [a, b, b]
    if numImgLR == 13:
        return [a, a, a, b, b]
    if numImgLR == 7:
        return [b, b]
    if numImgLR == 19:
        return [(5, 2, 2), (3, 2, 1), (3, 2, 0), (3, 2, 0), a, b, b, b, b, b]
    raise ValueError("reference defines reducers only for numImgLR in {7, 9, 13, 19}; got %r" % numImgLR)


def layer_specs(numFilters=32, numResBlocks=12, expRate=8, decayRate=0.8, numImgLR=9, scale=3, inChannels=1):
    """[(keras_name, v_shape)] in Keras topological order = checkpoint order
    `model/layer_with_weights-K` (modelInfo/ckpt_p16t9c85r12/NIR/ckpt-124.index).
    Per layer the variables are g [Cout], v (= kernel), bias [Cout]  (TFA WeightNormalization)."""
    f = numFilters
    dec = int(f * decayRate)                                   # models/modelsTF.py:182
    specs = [("mainConv1", (3, 3, 3, inChannels, f))]           # :58; Input(..., 1) or (..., 3): :19-20
    for i in range(numResBlocks):                               # :59-60, :177-189
        specs.append(("expConv_%d" % i, (1, 1, 1, f, f * expRate)))
        specs.append(("decConv_%d" % i, (1, 1, 1, f * expRate, dec)))
        specs.append(("normConv_%d" % i, (3, 3, 3, dec, f)))
    for i, (k, _, _) in enumerate(reducer_plan(numImgLR)):      # :159-160, :80
        specs.append(("convReducer_%d" % (i + 1), (k, k, k, f, f)))
    s2 = scale * scale
    specs.append(("residConv1", (3, 3, inChannels, s2)))        # :45-50 (depth-interleaved with main path)
    specs.append(("upscaleConv1", (3, 3, 3, f, s2)))            # :162-163
    specs.append(("residConv2", (3, 3, s2, s2)))
    specs.append(("residConv3", (3, 3, s2, s2)))
    return specs


# ----------------------------------------------------------------------------------------------
# primitive ops
# ----------------------------------------------------------------------------------------------
def weight_norm(v, g):
    """TFA WeightNormalization kernel:  tf.nn.l2_normalize(v, axis=all-but-last) * g
    = v * rsqrt(max(sum v^2, 1e-12)) * g      (models/modelsTF.py:191-197)."""
    v = np.asarray(v, F64)
    ss = (v * v).reshape(-1, v.shape[-1]).sum(axis=0)
    return v * (1.0 / np.sqrt(np.maximum(ss, 1e-12))) * np.asarray(g, F64)


def conv_valid(x, w):
    """Cross-correlation, stride 1, no padding.  x [N,H,W,T,Cin] (or [N,H,W,Cin]),
    w [kh,kw,kt,Cin,Cout] (or [kh,kw,Cin,Cout]).  Keras Conv3D/Conv2D never flips the kernel."""
    x = np.asarray(x, F64)
    w = np.asarray(w, F64)
    if w.ndim == 4:                                             # 2-D conv: add a unit T axis
        return conv_valid(x[:, :, :, None, :], w[:, :, None, :, :])[:, :, :, 0, :]
    kh, kw, kt = w.shape[:3]
    N, H, W, T, _ = x.shape
    Ho, Wo, To = H - kh + 1, W - kw + 1, T - kt + 1
    y = np.zeros((N, Ho, Wo, To, w.shape[-1]), F64)
    for a in range(kh):
        for b in range(kw):
            for c in range(kt):
                y += np.einsum("nhwti,io->nhwto", x[:, a:a + Ho, b:b + Wo, c:c + To, :], w[a, b, c])
    return y


def pad_zero_same(x, w):
    """Keras padding='same' for stride 1: (k-1)//2 zeros before, k//2 after, on every kernel axis
    (H, W and T for Conv3D)."""
    ks = w.shape[:-2]
    pads = [(0, 0)] + [((k - 1) // 2, k // 2) for k in ks] + [(0, 0)]
    return np.pad(x, pads, mode="constant")


def wn_conv(x, p, padding, relu):
    """WeightNormalization(Conv(outChannels, k, padding, activation)) (models/modelsTF.py:191-197)."""
    w = weight_norm(p["v"], p["g"])
    if padding == "same":
        x = pad_zero_same(x, w)
    y = conv_valid(x, w) + np.asarray(p["bias"], F64)
    return np.maximum(y, 0.0) if relu else y


def reflect_pad_hw(x, n=1, nt=0):
    """tf.pad(x, [[0,0],[n,n],[n,n],[nt,nt],[0,0]], mode='reflect') (models/modelsTF.py:157-158, :78-79)."""
    return np.pad(x, [(0, 0), (n, n), (n, n), (nt, nt), (0, 0)], mode="reflect")


def depth_to_space(x, s):
    """tf.nn.depth_to_space NHWC: out[n, s*h+i, s*w+j, c] = x[n, h, w, (i*s+j)*Co + c]."""
    N, H, W, C = x.shape
    co = C // (s * s)
    y = x.reshape(N, H, W, s, s, co).transpose(0, 1, 3, 2, 4, 5)
    return y.reshape(N, H * s, W * s, co)


# ----------------------------------------------------------------------------------------------
# network
# ----------------------------------------------------------------------------------------------
def wdsr_forward(x, params, mean, std, numResBlocks=12, numImgLR=9, scale=3, taps=None):
    """WDSRConv3D.build graph (models/modelsTF.py:15-43), x [N, P+6, P+6, T, 1] -> [N, 3P, 3P, 1].
    `params[name] = {"v","g","bias"}`.  `taps` (optional dict) collects intermediates."""
    x = np.asarray(x, F64)
    meanLR = x.mean(axis=3)                                     # :23  reduce_mean over T -> [N,H,W,1]
    xn = (x - mean) / std                                       # :26, :199-200
    mn = (meanLR - mean) / std                                  # :27

    # main / high-frequency path (:55-74)
    h = wn_conv(xn, params["mainConv1"], "same", True)          # :58
    if taps is not None:
        taps["mainConv1"] = h
    for i in range(numResBlocks):                               # :177-189
        e = wn_conv(h, params["expConv_%d" % i], "same", True)
        d = wn_conv(e, params["decConv_%d" % i], "same", False)
        n = wn_conv(d, params["normConv_%d" % i], "same", False)
        h = n + h
        if taps is not None:
            taps["dec_%d" % i] = d
            taps["block_%d" % i] = h
    for i, (_, pad, pad_t) in enumerate(reducer_plan(numImgLR)):  # :152-164 / :123-150 / :166-175 / :76-121
        if pad or pad_t:
            h = reflect_pad_hw(h, pad, pad_t)
        h = wn_conv(h, params["convReducer_%d" % (i + 1)], "valid", True)
        if taps is not None:
            taps["reducer_%d" % (i + 1)] = h
    h = wn_conv(h, params["upscaleConv1"], "valid", False)      # :162-163  -> [N,P,P,1,s*s]
    assert h.shape[3] == 1, "temporal axis must collapse to 1 before Reshape (models/modelsTF.py:71)"
    main = depth_to_space(h[:, :, :, 0, :], scale)              # :71-73

    # low-frequency residual path on the T-mean image (:45-53)
    r = wn_conv(mn, params["residConv1"], "valid", True)
    r = wn_conv(r, params["residConv2"], "valid", False)
    r = wn_conv(r, params["residConv3"], "valid", False)
    resid = depth_to_space(r, scale)
    if taps is not None:
        taps["main"] = main
        taps["resid"] = resid
    return (main + resid) * std + mean                          # :38, :41, :202-203


# ----------------------------------------------------------------------------------------------
# shift-compensated losses (models/loss.py)
# ----------------------------------------------------------------------------------------------
def _shift_terms(hr, mask, pred, cropBorder=3):
    """Common scaffolding of stackL1Loss / stackL2Loss / stackcPSNR (models/loss.py:140-180):
    returns l1[49,B], mse[49,B] in the reference's (i outer, j inner) order."""
    hr = np.asarray(hr, F64)[..., 0]
    m = np.asarray(mask).astype(F64)[..., 0]                    # cropImage casts to f32 (utils/utils.py:44)
    p = np.asarray(pred, F64)[..., 0]
    S = hr.shape[1]
    c = cropBorder
    L = S - 2 * c                                               # loss.py:24-25
    P = p[:, c:c + L, c:c + L]                                  # loss.py:74-75
    l1, l2 = [], []
    for i in range(2 * c + 1):                                  # loss.py:79-81
        for j in range(2 * c + 1):
            H = hr[:, i:i + L, j:j + L]                         # :141
            M = m[:, i:i + L, j:j + L]                          # :142
            n = M.sum(axis=(1, 2))                              # :144
            b = (1.0 / n) * (H - P * M).sum(axis=(1, 2))        # :146, :182-187 (HR NOT masked)
            C = (P + b[:, None, None]) * M                      # :148-149
            l1.append((1.0 / n) * np.abs(H - C).sum(axis=(1, 2)))      # :226-228
            l2.append((1.0 / n) * np.square(H - C).sum(axis=(1, 2)))   # :230-232
    return np.stack(l1), np.stack(l2)


def shift_l1_loss(hr, mask, pred, cropBorder=3):
    """Losses.shiftCompensatedL1Loss (models/loss.py:73-84): mean_B min_shift L1."""
    l1, _ = _shift_terms(hr, mask, pred, cropBorder)
    return l1.min(axis=0).mean()


def shift_l2_loss(hr, mask, pred, cropBorder=3):
    """Losses.shiftCompensatedL2Loss (models/loss.py:55-71)."""
    _, l2 = _shift_terms(hr, mask, pred, cropBorder)
    return l2.min(axis=0).mean()


def shift_cpsnr(hr, mask, pred, cropBorder=3, bitDepth=16):
    """Losses.shiftCompensatedcPSNR (models/loss.py:37-53, 234-238): per-sample max over shifts."""
    _, l2 = _shift_terms(hr, mask, pred, cropBorder)
    nb = 2.0 ** bitDepth - 1.0
    return (10.0 * (np.log(nb * nb / l2) / np.log(10.0))).max(axis=0)


def shift_l1_grad(hr, mask, pred, cropBorder=3):
    """d(shiftCompensatedL1Loss)/d(pred), derived in SURVEY.md A.4: the gradient of the arg-min
    shift only (ties split equally, as tf.reduce_min does), through both C and the bias b."""
    hr64 = np.asarray(hr, F64)[..., 0]
    m = np.asarray(mask).astype(F64)[..., 0]
    p = np.asarray(pred, F64)[..., 0]
    B, S = hr64.shape[0], hr64.shape[1]
    c = cropBorder
    L = S - 2 * c
    l1, _ = _shift_terms(hr, mask, pred, cropBorder)
    lmin = l1.min(axis=0)
    g = np.zeros_like(p)
    P = p[:, c:c + L, c:c + L]
    for bi in range(B):
        ties = np.flatnonzero(l1[:, bi] == lmin[bi])
        for s in ties:
            i, j = divmod(int(s), 2 * c + 1)
            H = hr64[bi, i:i + L, j:j + L]
            M = m[bi, i:i + L, j:j + L]
            n = M.sum()
            b = (H - P[bi] * M).sum() / n
            sg = np.sign(H - (P[bi] + b) * M)
            gk = -(M / n) * (sg - (sg * M).sum() / n)
            g[bi, c:c + L, c:c + L] += gk / (len(ties) * B)
    return g[..., None]


# ----------------------------------------------------------------------------------------------
# per-candidate tables, per-sample minima and the gradient of ONE given shift, for all three cfg losses.
# The device differentiates the shift it selected (first minimum in shift order), not tf.reduce_min's equal
# split among exact ties: `*_grad_at(arg)` is the closed-form gradient of candidate `arg` alone.
# A shift under which a sample has no clear pixel (n = 0) is NaN in the tables and is no candidate.
# ----------------------------------------------------------------------------------------------
def shift_tables(hr, mask, pred, cropBorder=3):
    """(l1[ns^2, B], l2[ns^2, B]) of every candidate registration (models/loss.py:140-180, 226-232), (i outer, j inner)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _shift_terms(hr, mask, pred, cropBorder)


def select_min(table):
    """Column-wise minimum over the non-NaN rows and the FIRST row that attains it; a column of NaNs only gives (NaN, 0)."""
    table = np.asarray(table, F64)
    if table.ndim == 1:
        v, a = select_min(table[:, None])
        return v[0], a[0]
    arg = np.where(np.isnan(table), np.inf, table).argmin(axis=0)
    return table[arg, np.arange(table.shape[1])], arg.astype(np.int32)


def second_best_gap(table):
    """Column-wise (second smallest - smallest) / max(|second smallest|, tiny) over the non-NaN rows (inf with fewer than two)."""
    t = np.sort(np.where(np.isnan(np.asarray(table, F64).reshape(len(table), -1)), np.inf, np.asarray(table, F64).reshape(len(table), -1)), axis=0)
    if t.shape[0] < 2:
        return np.full(t.shape[1], np.inf)
    with np.errstate(invalid="ignore"):
        gap = (t[1] - t[0]) / np.maximum(np.abs(t[1]), 1e-300)
    return np.where(np.isfinite(t[1]), gap, np.inf)


def shift_per_sample(hr, mask, pred, cropBorder=3, bitDepth=16):
    """dict(l1[B], l2[B], cpsnr[B], arg_l1[B], arg_l2[B]): what one device launch returns per sample."""
    t1, t2 = shift_tables(hr, mask, pred, cropBorder)
    l1, a1 = select_min(t1)
    l2, a2 = select_min(t2)
    nb = 2.0 ** bitDepth - 1.0
    with np.errstate(divide="ignore"):
        cpsnr = 10.0 * (np.log(nb * nb / l2) / np.log(10.0))       # the maximum over the shifts is the cPSNR of the smallest l2
    return {"l1": l1, "l2": l2, "cpsnr": cpsnr, "arg_l1": a1, "arg_l2": a2}


def _crop_at(hr, mask, pred, arg, c):
    """H, M [B,L,L] at each sample's own shift arg[b], P [B,L,L], n [B], bias [B]."""
    hr64 = np.asarray(hr, F64)[..., 0]
    m = (np.asarray(mask)[..., 0] != 0).astype(F64)
    p = np.asarray(pred, F64)[..., 0]
    B, S = hr64.shape[0], hr64.shape[1]
    L, ns = S - 2 * c, 2 * c + 1
    arg = np.broadcast_to(np.asarray(arg), (B,))
    H = np.stack([hr64[b, arg[b] // ns:arg[b] // ns + L, arg[b] % ns:arg[b] % ns + L] for b in range(B)])
    M = np.stack([m[b, arg[b] // ns:arg[b] // ns + L, arg[b] % ns:arg[b] % ns + L] for b in range(B)])
    P = p[:, c:c + L, c:c + L]
    n = M.sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        bias = (H - P * M).sum(axis=(1, 2)) / n
    return H, M, P, n, bias


def _embed(g, S, c):
    out = np.zeros((g.shape[0], S, S, 1), F64)
    out[:, c:S - c, c:S - c, 0] = g
    return out


def shift_grad_at(hr, mask, pred, arg, cropBorder=3, which=1, upstream=1.0):
    """d(upstream * mean_B candidate arg[b])/d(pred) for the L1 (which=1) or L2 (which=2) term:
    dP = -(M/n) (s - sum(s M)/n),  s = sign(H - C) or 2 (H - C); zero on the border ring."""
    H, M, P, n, bias = _crop_at(hr, mask, pred, arg, cropBorder)
    B = H.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = H - (P + bias[:, None, None]) * M
        s = np.sign(e) if which == 1 else 2.0 * e
        nn = n[:, None, None]
        g = -(M / nn) * (s - (s * M).sum(axis=(1, 2), keepdims=True) / nn) * (upstream / B)
    return _embed(g, np.asarray(hr).shape[1], cropBorder)


def sobel_edges(D):
    """tf.image.sobel_edges on [B,L,L]: 3x3 cross-correlations with [[-1,-2,-1],[0,0,0],[1,2,1]] (Gy) and its transpose (Gx) of the
    REFLECT-padded image."""
    Dp = np.pad(np.asarray(D, F64), [(0, 0), (1, 1), (1, 1)], mode="reflect")
    gy = (Dp[:, 2:, :-2] + 2.0 * Dp[:, 2:, 1:-1] + Dp[:, 2:, 2:]) - (Dp[:, :-2, :-2] + 2.0 * Dp[:, :-2, 1:-1] + Dp[:, :-2, 2:])
    gx = (Dp[:, :-2, 2:] + 2.0 * Dp[:, 1:-1, 2:] + Dp[:, 2:, 2:]) - (Dp[:, :-2, :-2] + 2.0 * Dp[:, 1:-1, :-2] + Dp[:, 2:, :-2])
    return gy, gx


def shift_l1edge_table(hr, mask, pred, cropBorder=3, pi=0.7):
    """[ns^2, B] candidates of shiftCompensatedL1EdgeLoss (models/loss.py:86-97, 126-137, 214-219):
    pi * sum|D|/n + (1 - pi) * sum(|Gy| + |Gx|)/n with D = H - C; sobel_edges is linear, so edges(H) - edges(C) = edges(D)."""
    B, S = np.asarray(hr).shape[0], np.asarray(hr).shape[1]
    ns = 2 * cropBorder + 1
    out = []
    for s in range(ns * ns):
        H, M, P, n, bias = _crop_at(hr, mask, pred, np.full(B, s), cropBorder)
        with np.errstate(divide="ignore", invalid="ignore"):
            D = H - (P + bias[:, None, None]) * M
            gy, gx = sobel_edges(D)
            out.append((pi * np.abs(D).sum(axis=(1, 2)) + (1.0 - pi) * (np.abs(gy) + np.abs(gx)).sum(axis=(1, 2))) / n)
    return np.stack(out)


def shift_l1edge_sobel_at(hr, mask, pred, arg, cropBorder=3):
    """(D, Gy, Gx) [B,L,L] at each sample's shift arg[b]."""
    H, M, P, n, bias = _crop_at(hr, mask, pred, arg, cropBorder)
    D = H - (P + bias[:, None, None]) * M
    return (D,) + sobel_edges(D)


def shift_l1edge_grad_at(hr, mask, pred, arg, cropBorder=3, pi=0.7, upstream=1.0):
    """Gradient of upstream * mean_B candidate arg[b] of the edge loss:
    G = [pi sign(D) + (1 - pi) Sobel^T(sign Gy, sign Gx)] / n,  dP = -M (G - sum(G M)/n); Sobel^T scatters every output's taps onto the
    padded crop and folds the mirrored pad back (pad row -1 onto row 1, pad row L onto row L-2; likewise the columns)."""
    H, M, P, n, bias = _crop_at(hr, mask, pred, arg, cropBorder)
    B, L = H.shape[0], H.shape[1]
    D = H - (P + bias[:, None, None]) * M
    gy, gx = sobel_edges(D)
    sy, sx = np.sign(gy), np.sign(gx)
    ky = np.array([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]])
    gp = np.zeros((B, L + 2, L + 2), F64)
    for a in range(3):
        for b in range(3):
            gp[:, a:a + L, b:b + L] += ky[a, b] * sy + ky[b, a] * sx
    rows = gp[:, 1:-1, :].copy()
    rows[:, 1, :] += gp[:, 0, :]
    rows[:, L - 2, :] += gp[:, L + 1, :]
    A = rows[:, :, 1:-1].copy()
    A[:, :, 1] += rows[:, :, 0]
    A[:, :, L - 2] += rows[:, :, L + 1]
    nn = n[:, None, None]
    G = (pi * np.sign(D) + (1.0 - pi) * A) / nn
    g = -M * (G - (G * M).sum(axis=(1, 2), keepdims=True) / nn) * (upstream / B)
    return _embed(g, np.asarray(hr).shape[1], cropBorder)


_RS_SIGMA = (0.5, 1.0, 2.0, 4.0, 8.0)


def _revssim_parts(hr, mask, pred, s, c, bit_depth):
    """Everything of candidate s: H, Cc, M [B,L,L], n [B], normalised windows w [5,B,L,L] and the moment terms [5,B]."""
    B = np.asarray(hr).shape[0]
    H, M, P, n, bias = _crop_at(hr, mask, pred, np.full(B, s), c)
    L = H.shape[1]
    nb = 2.0 ** bit_depth - 1.0
    C1, C3 = (0.01 * nb) ** 2, (0.03 * nb) ** 2 / 2.0
    x = np.linspace(-L / 2.0, L / 2.0, L)
    Cc = (P + bias[:, None, None]) * M
    w = []
    for sig in _RS_SIGMA:
        w1 = np.exp(-x / (2.0 * sig * sig))                             # the reference's window: x is NOT squared
        ww = np.outer(w1, w1)[None] * M
        w.append(ww / ww.sum(axis=(1, 2), keepdims=True))
    w = np.stack(w)
    t = {"muH": (w * H).sum(axis=(2, 3)), "muS": (w * Cc).sum(axis=(2, 3))}
    t["sH"] = (w * H * H).sum(axis=(2, 3)) - t["muH"] ** 2
    t["sS"] = (w * Cc * Cc).sum(axis=(2, 3)) - t["muS"] ** 2
    t["cov"] = (w * H * Cc).sum(axis=(2, 3)) - t["muS"] * t["muH"]
    t["lum"] = (2 * t["muH"] * t["muS"] + C1) / (t["muH"] ** 2 + t["muS"] ** 2 + C1)
    t["con"] = (2 * t["sH"] * t["sS"] + C1) / (t["sH"] ** 2 + t["sS"] ** 2 + C1)
    t["str"] = (2 * t["cov"] + C3) / (t["sH"] * t["sS"] + C3)
    t["l1"] = (w * np.abs(H - Cc)).sum(axis=(2, 3))
    return H, Cc, M, n, w, t, nb, C1, C3


def shift_revssim_table(hr, mask, pred, cropBorder=3, bit_depth=16, eta=0.25):
    """[ns^2] candidates of shiftCompensatedRevSSIM (models/loss.py:99-124, 189-212): ONE scalar per shift for the whole batch."""
    B = np.asarray(hr).shape[0]
    ns = 2 * cropBorder + 1
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(ns * ns):
            _, _, _, _, _, t, nb, _, _ = _revssim_parts(hr, mask, pred, s, cropBorder, bit_depth)
            ssim = 1.0 - (t["lum"] * (t["con"] * t["str"]).prod(axis=0)).sum() / B
            out.append(eta * ssim + (1.0 - eta) * (t["l1"].sum() / B) / nb)
    return np.array(out)


def shift_revssim_grad_at(hr, mask, pred, arg, cropBorder=3, bit_depth=16, eta=0.25, upstream=1.0):
    """Gradient of upstream * candidate `arg` (one shift for the batch).  With T_b = (sum_s lum_s) prod_s con_s str_s and the window
    weights held fixed, d muS/dC_k = w_k, d sS/dC_k = 2 w_k (C_k - muS), d cov/dC_k = w_k (H_k - muH), d|H - C|/dC = -sign(H - C);
    then C = (P + bias) M gives dP = M (g - sum(g M)/n)."""
    B = np.asarray(hr).shape[0]
    H, Cc, M, n, w, t, nb, C1, C3 = _revssim_parts(hr, mask, pred, int(arg), cropBorder, bit_depth)
    cs = t["con"] * t["str"]                                            # [5,B]
    lsum = t["lum"].sum(axis=0)
    pcs = cs.prod(axis=0)
    g = np.zeros_like(H)
    for s in range(len(_RS_SIGMA)):
        pex = np.prod(np.delete(cs, s, axis=0), axis=0)
        muH, muS, sH, sS, cov = (t[k][s] for k in ("muH", "muS", "sH", "sS", "cov"))
        dl = muH ** 2 + muS ** 2 + C1
        dlum = (2 * muH * dl - (2 * muH * muS + C1) * 2 * muS) / dl ** 2
        dc = sH ** 2 + sS ** 2 + C1
        dcon = (2 * sH * dc - (2 * sH * sS + C1) * 2 * sS) / dc ** 2
        ds = sH * sS + C3
        dstr_cov, dstr_sS = 2.0 / ds, -(2 * cov + C3) * sH / ds ** 2
        a = (pcs * dlum)[:, None, None]
        bq = (lsum * pex * t["str"][s] * dcon + lsum * pex * t["con"][s] * dstr_sS)[:, None, None]
        cq = (lsum * pex * t["con"][s] * dstr_cov)[:, None, None]
        g += -(eta / B) * w[s] * (a + 2 * bq * (Cc - muS[:, None, None]) + cq * (H - muH[:, None, None]))
        g += -((1.0 - eta) / (nb * B)) * w[s] * np.sign(H - Cc)
    d = M * (g - (g * M).sum(axis=(1, 2), keepdims=True) / n[:, None, None]) * upstream
    return _embed(d, np.asarray(hr).shape[1], cropBorder)
