"""The case tables of the non-finite contracts ('Non-finite values'): one module serves tests/test_gpu_nonfinite.py (the
device against the references) and tests/test_nonfinite_host.py (the references alone, no GPU), which proves for every case that the
reference really is non-finite where the case says so -- a test that asserts "must be non-finite" is only worth something if the reference
satisfies the precondition on its own.

Values: NaN, +inf, -inf, written into ordinary float buffers.  They are data, not faults.

Single operators
  CONV_NAMES       the rows of tests/test_gpu_parity.py::CONV_CASES that are run (shipped-layer shapes and the ragged direct-kernel one)
  conv_positions   where one element of the poisoned sample is replaced: its first voxel, its last voxel, and an interior voxel in row 5 --
                   the first row of the second five-row strip of a 22-row patch, and the row the mirrored pads and the 'same' pads do not
                   duplicate (the first and last voxels are duplicated by the mirrored pads)
  PW_SHAPES        (nvox, voxels per sample) of the fused pointwise pair; pw_positions: voxel 0, voxels 31 and 32 (the tile boundary) and the
                   last voxel of the sample, which sits in the short last tile
Whole step (contracts T, S, I): a small engine, F = 32, R = 2, E = 8, decay 0.8, T = 9, P = 16, B = 3, shiftCompensatedL1Loss.
  STEP_CASES       (a) one LR pixel of sample 1; (b) the gain g of normConv_0 scaled until the fp32 network overflows behind it, parameters
                   finite; (c) the same on convReducer_1 and upscaleConv1; (d) one element of dy; (e) g of normConv_0 times 2^40, finite.
  The reference of the whole step is the fp32 evaluation of oracle/wdsr_torch.py on the CPU: fp64 would not overflow where fp32 does.
"""
import functools

import numpy as np
import torch

from oracle import wdsr_torch as ot
from probav_amd import synth

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
VALUES = (("nan", NAN), ("+inf", PINF), ("-inf", NINF))
POISONED = 1                                              # the sample that receives the value, in every case

# ---- single operators -------------------------------------------------------------------------------------------------------------
CONV_NAMES = ("normConv same 25->32 + skip", "convReducer_1 reflect+valid", "convReducer_2 valid relu", "bwd-data of reducer: full 32->32 gated",
              "upscaleConv1 valid 32->9", "mainConv1 same 1->32 relu", "normConv small ragged")
# the shipped-layer shapes that the matrix kernels behind impl 4 take (Cin 25 or 32: csrc/kernels_x6.hip): they must run there, not be refused.
# mainConv1's one input channel is not among them -- probav_conv3d_forward refuses 1 -> 32 at impl 2, 3 and 4, the engine runs its own
# one-channel kernel for that layer, which the whole-step tests reach in every family.
CONV_ON_IMPL4 = CONV_NAMES[:5]


def conv_positions(hwt):
    H, W, T = hwt
    return (("first", (0, 0, 0)), ("last", (H - 1, W - 1, T - 1)), ("interior", (5 if H > 10 else H // 2, W // 2, T // 2)))


PW_SHAPES = ((3 * 33, 33), (2 * 1640, 1640))


def pw_positions(vps):
    return (("v0", 0), ("v31", 31), ("v32", 32), ("last", vps - 1))


# ---- whole step ---------------------------------------------------------------------------------------------------------------------
ARCH = dict(numFilters=32, numResBlocks=2, expRate=8, decayRate=0.8, numImgLR=9)
BATCH, PARAM_SEED, BATCH_SEED = 3, 301, 302
PIXEL = (POISONED, 9, 13, 4, 0)                           # (a): one LR pixel of sample 1, interior, frame 4
DY_PIXEL = (POISONED, 20, 31, 0)                          # (d): one element of dy, inside the loss's crop
# (b), (c): the factor on the layer's gain g.  tests/test_nonfinite_host.py proves what each does in the fp32 reference (+inf in some voxels,
# finite values in others, finite parameters) and that 2^-4 of it overflows nothing: found there, fixed here.
# normConv_0 alone cannot overflow: a weight-normalised filter has unit norm, this network's decConv_0 output has patches of norm < 1, and
# no finite fp32 gain times a number below 1 leaves fp32.  So (b) also lifts the gain of decConv_0, the layer in front, by LIFT = 2^8
# (finite too): the overflow still happens in normConv_0's output, the block-1 input, which is where the case wants it.
OVERFLOW_FACTOR = {"normConv_0": 2.0 ** 122, "convReducer_1": 2.0 ** 121, "upscaleConv1": 2.0 ** 121}
LIFT = {"normConv_0": ("decConv_0", 2.0 ** 8)}
LARGE_FINITE = 2.0 ** 40


def _step_case(cid, site, **kw):
    return dict(id=cid, site=site, **kw)


STEP_CASES = [_step_case("a-input-nan", "input", value=NAN), _step_case("a-input-inf", "input", value=PINF),
              _step_case("b-overflow-normConv_0", "gain", layer="normConv_0", factor=OVERFLOW_FACTOR["normConv_0"]),
              _step_case("c-overflow-convReducer_1", "gain", layer="convReducer_1", factor=OVERFLOW_FACTOR["convReducer_1"]),
              _step_case("c-overflow-upscaleConv1", "gain", layer="upscaleConv1", factor=OVERFLOW_FACTOR["upscaleConv1"]),
              _step_case("d-dy-nan", "dy", value=NAN), _step_case("d-dy-inf", "dy", value=PINF)]
LARGE_CASE = _step_case("e-large-finite", "gain", layer="normConv_0", factor=LARGE_FINITE)
FORWARD_CASES = [c for c in STEP_CASES if c["site"] != "dy"]          # contract I: (a) - (c)


def ids(cases):
    return [c["id"] for c in cases]


def by_id(cid):
    return next(c for c in STEP_CASES + [LARGE_CASE] if c["id"] == cid)


def clean_inputs():
    """(x, hr, mask, params) of the small engine, all finite, from their seeds alone."""
    x, hr, mask = synth.synth_batch(BATCH, seed=BATCH_SEED)
    return x, hr, mask, synth.synth_params(seed=PARAM_SEED, perturb=True, **ARCH)


def apply_case(case, x, params, dy=None):
    """-> (x, params, dy) with the case applied to copies; dy: the upstream gradient [B, 48, 48, 1] of site 'dy' (else passed through)."""
    x = np.array(x, copy=True)
    params = {name: {k: np.array(v, copy=True) for k, v in p.items()} for name, p in params.items()}
    dy = None if dy is None else np.array(dy, copy=True)
    if case["site"] == "input":
        x[PIXEL] = case["value"]
    elif case["site"] == "gain":
        scaled = [(case["layer"], case["factor"])] + ([LIFT[case["layer"]]] if case["layer"] in LIFT and case["factor"] > LARGE_FINITE else [])
        for layer, factor in scaled:
            params[layer]["g"] = (params[layer]["g"].astype(np.float64) * factor).astype(np.float32)
            assert np.isfinite(params[layer]["g"]).all(), "the scaled gain must stay finite: the case poisons no parameter"
    elif case["site"] == "dy":
        dy[DY_PIXEL] = case["value"]
    else:
        raise ValueError(case["site"])
    return x, params, dy


def upstream():
    """The finite dy of site (d): seeded, the size of a loss gradient."""
    return (np.random.default_rng(303).normal(size=(BATCH, 48, 48, 1)) / (48 * 48 * BATCH)).astype(np.float32)


def block1_input(x, params, dtype=torch.float32):
    """The input of residual block 1 (= the output of block 0) of the oracle network, for (b)."""
    with torch.no_grad():
        p = ot.to_torch_params(params, dtype=dtype, requires_grad=False)
        h = ot.wn_conv((torch.tensor(x, dtype=dtype) - synth.NIR_MEAN) / synth.NIR_STD, p["mainConv1"], "same", True)
        e = ot.wn_conv(h, p["expConv_0"], "same", True)
        d = ot.wn_conv(e, p["decConv_0"], "same", False)
        return (ot.wn_conv(d, p["normConv_0"], "same", False) + h).numpy()


def reference_step(case, dtype=torch.float32):
    """The oracle's training step on the case, in `dtype` on the CPU: {"pred" [B,48,48,1], "loss" (None for site 'dy'), "grad" flat [n]}."""
    return _reference_step(case["id"], dtype)


@functools.lru_cache(maxsize=None)
def _reference_step(cid, dtype):
    case = by_id(cid)
    x, hr, mask, params = clean_inputs()
    x, params, dy = apply_case(case, x, params, upstream() if case["site"] == "dy" else None)
    pt = ot.to_torch_params(params, dtype=dtype)
    xt = torch.tensor(x, dtype=dtype)
    kw = dict(numResBlocks=ARCH["numResBlocks"], numImgLR=ARCH["numImgLR"])
    leaves = [t for p in pt.values() for t in (p["g"], p["v"], p["bias"])]
    if case["site"] == "dy":
        pred = ot.wdsr_forward(xt, pt, synth.NIR_MEAN, synth.NIR_STD, **kw)
        grads, loss = torch.autograd.grad(pred, leaves, torch.tensor(dy, dtype=dtype)), None
        pred = pred.detach()
    else:
        pred = ot.wdsr_forward(xt, pt, synth.NIR_MEAN, synth.NIR_STD, **kw)
        loss = ot.shift_l1_loss(torch.tensor(hr), torch.tensor(mask), pred)
        grads = torch.autograd.grad(loss, leaves)
        pred, loss = pred.detach(), float(loss.detach())
    flat = torch.cat([g.reshape(-1) for g in grads]).numpy()
    return {"pred": pred.numpy(), "loss": loss, "grad": flat}


def step_is_nonfinite(ref):
    """Contract T's precondition: the reference's loss or any element of its gradient is non-finite."""
    return (ref["loss"] is not None and not np.isfinite(ref["loss"])) or not np.isfinite(ref["grad"]).all()


def poisoned_samples(ref):
    """Contract I's precondition, per sample: the reference prediction of the sample holds a non-finite element."""
    return [b for b in range(ref["pred"].shape[0]) if not np.isfinite(ref["pred"][b]).all()]


# ---- single operators: inputs and references ------------------------------------------------------------------------------------------
def conv_case(name):
    from tests.test_gpu_parity import CONV_CASES
    return next(c for c in CONV_CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """Clean operands of a CONV_CASES row, seeded by its name: {"x", "w", "bias", "gate" | None, "skip" | None, "ho"}.  A gated case has its gate
    OPEN (= 1) at the three injection positions of x in the poisoned sample: a value under a closed gate is selected away by design
    (`gate > 0 ? x : 0`, as TensorFlow's ReluGrad), which `x * (gate > 0)` in the fp64 reference would turn into inf * 0 = NaN."""
    import zlib
    from tests.test_gpu_parity import _out_dims
    _, N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip = conv_case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 77)
    ho = _out_dims(hwt, k, pad, reflect)
    d = {"x": rng.normal(size=(N,) + hwt + (Cin,)).astype(np.float32),
         "w": (rng.normal(size=k + (Cin, Cout)) / np.sqrt(np.prod(k) * Cin)).astype(np.float32),
         "bias": rng.normal(size=Cout).astype(np.float32), "gate": None, "skip": None, "ho": ho}
    if use_gate:
        d["gate"] = rng.normal(size=d["x"].shape).astype(np.float32)
        for _, p in conv_positions(hwt):
            d["gate"][(POISONED,) + p] = 1.0
    if use_skip:
        d["skip"] = rng.normal(size=(N,) + ho + (Cout,)).astype(np.float32)
    return d


def conv_operands(name):
    """The operands that receive a value, per case: x always, skip and gate where the case has them, then one element of w and of bias."""
    c = conv_case(name)
    return ("x",) + (("skip",) if c[10] else ()) + (("gate",) if c[9] else ()) + ("w", "bias")


def conv_poisoned(name, operand, posname, value):
    """A copy of conv_inputs(name) with `value` in one element of `operand`: x / gate at conv_positions(input dims), skip at
    conv_positions(output dims), always of sample POISONED and in the LAST channel; w at its centre tap, last input and output channel;
    bias in its last channel (posname is ignored for w and bias)."""
    c, d = conv_case(name), dict(conv_inputs(name))
    a = np.array(d[operand], copy=True)
    if operand in ("x", "gate"):
        a[(POISONED,) + dict(conv_positions(c[2]))[posname] + (a.shape[-1] - 1,)] = value
    elif operand == "skip":
        a[(POISONED,) + dict(conv_positions(d["ho"]))[posname] + (a.shape[-1] - 1,)] = value
    elif operand == "w":
        a[tuple(s // 2 for s in a.shape[:3]) + (a.shape[3] - 1, a.shape[4] - 1)] = value
    else:
        a[-1] = value
    d[operand] = a
    return d


@functools.lru_cache(maxsize=None)
def _conv_core(name, operand, posname, valname):
    """_oracle_conv (tests/test_gpu_parity.py: fp64, IEEE) WITHOUT bias and skip -- both are added after the ReLU-free sum and cost nothing --
    of the poisoned sample alone (x, gate) or of all samples (w)."""
    from tests.test_gpu_parity import _oracle_conv
    c = conv_case(name)
    d = conv_inputs(name) if operand is None else conv_poisoned(name, operand, posname, dict(VALUES)[valname])
    sl = slice(None) if operand in (None, "w") else slice(POISONED, POISONED + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return _oracle_conv(d["x"][sl], None if d["gate"] is None else d["gate"][sl], d["w"], None, None, c[6], c[7], 0, d["ho"])


def conv_reference(name, operand, posname, valname):
    """The fp64 reference of the launch conv_poisoned(...) describes: all samples for w and bias, else the poisoned sample alone [1, ...]."""
    c = conv_case(name)
    d = conv_poisoned(name, operand, posname, dict(VALUES)[valname])
    whole = operand in ("w", "bias")
    core = _conv_core(name, operand, posname, valname) if operand in ("x", "gate", "w") else _conv_core(name, None, None, None)
    if not whole and core.shape[0] != 1:
        core = core[POISONED:POISONED + 1]
    sl = slice(None) if whole else slice(POISONED, POISONED + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        y = core + d["bias"].astype(np.float64)
        if c[8]:
            y = np.maximum(y, 0)                                  # np.maximum propagates NaN (IEEE maximum), as torch.relu and tf.nn.relu do
        if d["skip"] is not None:
            y = y + d["skip"][sl].astype(np.float64)
    return y


# backward-filter: the detector
WGRAD_NAMES = tuple(n for n in CONV_NAMES if "bwd-data" not in n)
# the shipped 3x3x3 layers whose backward-filter the split families take (Cin 25 or 32 and Cout 32: csrc/kernels_x6.hip, kernels_wg4.hip): they must
# not be refused at impl 4.  upscaleConv1 (9 filters) and mainConv1 (one input channel) are outside that predicate; the engine runs their
# backward-filter on other kernels, which the whole-step tests reach.
WGRAD_ON_IMPL4 = ("normConv same 25->32 + skip", "convReducer_1 reflect+valid", "convReducer_2 valid relu")
WGRAD_VARIANTS = tuple((kind, v) for kind in ("x-random", "x-zero", "dy-open", "dy-closed") for v in ("+inf", "nan"))


def wgrad_inputs(name, kind, valname):
    """{"x", "dy", "gate" | None} of probav_conv3d_wgrad with one value planted in sample POISONED.
    x-random / x-zero: the value in x at the interior position, last channel; dy random, or exactly zero over every output voxel within two
    of that position, all channels (inf * 0).  dy-open / dy-closed: the value in dy at the interior output position, last channel, under
    an open / a closed gate (a layer without ReLU has no gate: both are then the same launch)."""
    import zlib
    c = conv_case(name)
    _, N, hwt, Cin, Cout, k, pad, reflect, relu = c[:9]
    ho = conv_inputs(name)["ho"]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 78)
    x = rng.normal(size=(N,) + hwt + (Cin,)).astype(np.float32)
    dy = rng.normal(size=(N,) + ho + (Cout,)).astype(np.float32)
    gate = rng.normal(size=dy.shape).astype(np.float32) if relu else None
    value = dict(VALUES)[valname]
    pi, po = dict(conv_positions(hwt))["interior"], dict(conv_positions(ho))["interior"]
    if kind.startswith("x-"):
        x[(POISONED,) + pi + (Cin - 1,)] = value
        if kind == "x-zero":
            dy[(POISONED,) + tuple(slice(max(p - 2, 0), p + 3) for p in pi)] = 0.0
    else:
        dy[(POISONED,) + po + (Cout - 1,)] = value
        if gate is not None:
            gate[(POISONED,) + po + (Cout - 1,)] = 1.0 if kind == "dy-open" else -1.0
    return {"x": x, "dy": dy, "gate": gate}


@functools.lru_cache(maxsize=None)
def wgrad_reference(name, kind, valname):
    """(dw, db) by torch autograd in fp64, as tests/test_gpu_parity.py::test_conv3d_wgrad_matches_autograd forms them -- with the gate as the
    SELECT that autograd of a ReLU is (torch's threshold_backward, TensorFlow's ReluGrad): a value of dy under a closed gate is dropped,
    not multiplied by zero."""
    c = conv_case(name)
    _, N, hwt, Cin, Cout, k, pad, reflect, relu = c[:9]
    d = wgrad_inputs(name, kind, valname)
    F = torch.nn.functional
    if reflect:
        xp = torch.tensor(np.pad(d["x"].astype(np.float64), [(0, 0), (pad[0],) * 2, (pad[1],) * 2, (0, 0), (0, 0)], mode="reflect"))
        xp = F.pad(xp, (0, 0, pad[2], pad[2]))
    else:
        xp = F.pad(torch.tensor(d["x"], dtype=torch.float64), (0, 0, pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    wt = torch.zeros(k + (Cin, Cout), dtype=torch.float64, requires_grad=True)
    yt = F.conv3d(xp.permute(0, 4, 1, 2, 3), wt.permute(4, 3, 0, 1, 2)).permute(0, 2, 3, 4, 1)
    dyg = torch.tensor(d["dy"], dtype=torch.float64)
    if d["gate"] is not None:
        dyg = torch.where(torch.tensor(d["gate"]) > 0, dyg, torch.zeros_like(dyg))
    (dw,) = torch.autograd.grad(yt, wt, dyg)
    return dw.numpy(), dyg.sum(dim=(0, 1, 2, 3)).numpy()


# the fused pointwise pair (D = 25)
@functools.lru_cache(maxsize=None)
def pw_inputs(nvox):
    rng = np.random.default_rng(9000 + nvox)
    D = 25
    return {"x": rng.normal(size=(nvox, 32)).astype(np.float32), "w1": (rng.normal(size=(32, 256)) / np.sqrt(32)).astype(np.float32),
            "b1": rng.normal(scale=0.3, size=256).astype(np.float32), "w2": (rng.normal(size=(256, D)) / 16).astype(np.float32),
            "b2": rng.normal(scale=0.3, size=D).astype(np.float32), "ddec": rng.normal(size=(nvox, D)).astype(np.float32),
            "dskip": rng.normal(size=(nvox, 32)).astype(np.float32)}


def pw_poisoned(nvox, vps, posname, valname, zero_dy=False):
    """x[voxel of sample POISONED, last channel] = value; zero_dy: d_dec of that voxel exactly zero, all channels."""
    d = dict(pw_inputs(nvox))
    v = POISONED * vps + dict(pw_positions(vps))[posname]
    d["x"] = np.array(d["x"], copy=True)
    d["x"][v, 31] = dict(VALUES)[valname]
    if zero_dy:
        d["ddec"] = np.array(d["ddec"], copy=True)
        d["ddec"][v] = 0.0
    return d


@functools.lru_cache(maxsize=None)
def pw_reference(nvox, vps, posname, valname, zero_dy=False):
    """fp64 numpy of the pair and its reverse pass, as tests/test_gpu_parity.py::_fused_pointwise_case states them (posname None: clean)."""
    d = pw_inputs(nvox) if posname is None else pw_poisoned(nvox, vps, posname, valname, zero_dy)
    X, W1, W2, ddec = (d[k].astype(np.float64) for k in ("x", "w1", "w2", "ddec"))
    with np.errstate(invalid="ignore", over="ignore"):
        Hpre = X @ W1 + d["b1"]
        Hh = np.maximum(Hpre, 0)
        dH = np.where(Hpre > 0, ddec @ W2.T, 0.0)
        return {"dec": Hh @ W2 + d["b2"], "dx": d["dskip"] + dH @ W1.T, "dw1": X.T @ dH, "db1": dH.sum(0), "dw2": Hh.T @ ddec, "db2": ddec.sum(0)}
