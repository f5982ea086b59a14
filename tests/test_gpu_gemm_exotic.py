"""The general matrix route's exotic launches, on the device (include/probav_hip.h, 'the route's exotic launches'; csrc/engine.hip: conv_route / wgrad_route).

With probav_engine_set_gemm_exotic on, the 19-frame reducer's 5x5x5 layer and its 3x3x3 layers on mirrored pads of 2 -- forward and backward-filter of reducers
1-4, the backward-data of the 5x5x5 layer -- run on the route's kernels (gemm_conv_fwd_kernel / gemm_conv_fwd_x6_kernel / gemm_conv_wgrad_kernel) through the wide
predicates of csrc/kernels_gemm.h.  They have no single-operator entry point: they are reached, and held, through the engine.  Every test first asserts
probav_engine_gemm_exotic == 1 and, after a step, from probav_engine_launched_counts that no convolution and no backward-filter launch ran on the generic direct
kernels (a library without the switch would pass the oracle checks on those).

Rows are (F, R, E, decay, D), T, gray, B, P -- the smallest 19-frame engines on which each tiling decision of the new paths can go wrong: less than one K chunk, an
N-tile tail, M tiles that straddle samples (1 900 voxels per sample) and slabs with a ragged end (A); two accumulator tiles and a K tail of 8 (B); the NT = 4 instance
with a tail, 2 x 2 backward-filter tiles with tails on both sides and three input channels (C); the real use, the tuned block kernels around the reducers and at impl
4 the H3 neighbours that need the amax slots (D)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests import bands
from tests.test_gemm_route_host import make_engine
from tests.test_gpu_gemm_pair import _L, _layer, _view
from tests.test_gpu_gemm_route import _same
from tests.test_gpu_gemm_x6 import _arith, _err, _kind, _stepper

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32

A = ((9, 1, 2, 0.7, 6), 19, True, 3, 4)
B_ = ((40, 1, 2, 0.8, 32), 19, True, 2, 4)
C = ((72, 1, 2, 0.8, 57), 19, False, 1, 4)
D = ((32, 1, 8, 0.8, 25), 19, True, 2, 16)
ROWS = [A, B_, C, D]


def _id(c):
    return "f%d-r%d-e%d-d%d-t%d-%s-b%d-p%d" % (c[0][0], c[0][1], c[0][2], c[0][4], c[1], "gray" if c[2] else "rgb", c[3], c[4])


def _pair_kind(row, pair):
    """What probav_engine_pair_kind answers at family >= 1: the tuned pair of the shipped shape whatever the switches, else the general pair where it is wished and in range."""
    from tests import test_gpu_cfg_values as cv
    F, R, E, decay, Dc = row
    return 1 if cv.pw_fused(F, E, Dc) else (2 if pair and F <= 64 and Dc <= 64 else 0)


def _exotic(m):
    return _L().lib().probav_engine_gemm_exotic(m._handle())


def _launched(m, reset=True):
    c = (ctypes.c_int32 * 4)()
    assert _L().lib().probav_engine_launched_counts(m._handle(), ctypes.byref(c), int(reset)) == 0
    return tuple(c)


def _none_on_the_direct_kernels(m):
    """After at least one training step since the last reset: launches on the route, none on the generic direct kernels."""
    c = _launched(m)
    assert c[0] == 0 and c[2] == 0 and c[1] >= 5 and c[3] >= 4, c
    return c


def _model(dev, case, impl, pair=False, x6=True, exotic=True, seed=11):
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    m = cv._build(dev, row, T, gray, seed, P)[0]
    m.set_impl(impl)
    m.set_gemm_route(True)
    m.set_gemm_pair(pair)
    m.set_gemm_x6(x6)
    m.set_gemm_exotic(exotic)
    assert m.gemm_exotic is bool(exotic) and _exotic(m) == int(exotic) and _arith(m) == int(x6) and _kind(m) == _pair_kind(row, pair)
    return m


def _step_of(dev, m, case, seed=12):
    row, T, gray, B, P = case
    return _stepper(dev, m, B, T, 1 if gray else 3, P, seed)


@pytest.fixture(autouse=True)
def _keep_workspaces(monkeypatch):
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")                      # the gates and the saved activations are read from a pass's workspace


@pytest.fixture(scope="module", autouse=True)
def _release_the_arena(dev):
    yield
    bands.release(dev)


# ---- 1. the whole network against the fp64 oracle ---------------------------------------------------------------------------------------------------
NET = [(c, impl, x6) for c in ROWS for impl in (1, 4) for x6 in (0, 1)]             # (row outermost: one oracle per row); the pair on where it applies


@pytest.mark.parametrize("case,impl,x6", NET, ids=["%s-impl%d-x6%d" % (_id(c), i, x) for c, i, x in NET])
def test_whole_network_matches_the_oracle(dev, case, impl, x6, monkeypatch):
    """tests/test_gpu_cfg_values.py::_check_against_the_oracle, unchanged, on engines created with PROBAV_GEMM_ROUTE=1 PROBAV_GEMM_PAIR=1 PROBAV_GEMM_EXOTIC=1 and
    PROBAV_GEMM_X6 = 0 / 1: output 2e-5, loss 1e-5, every gradient tensor 1e-3 at the device's gates -- which holds the four reducer filter gradients and the folded
    backward-data -- and its bit-for-bit properties: repeated step, training = inference, sample alone, side-stream mode."""
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    for name, value in (("PROBAV_GEMM_ROUTE", "1"), ("PROBAV_GEMM_PAIR", "1"), ("PROBAV_GEMM_X6", str(x6)), ("PROBAV_GEMM_EXOTIC", "1")):
        monkeypatch.setenv(name, value)
    lib = _L().lib()
    h = make_engine(lib, row[0], row[1], row[2], row[4], T, 1 if gray else 3, P)
    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_gemm_exotic(h) == 1 and lib.probav_engine_gemm_arith(h) == x6
    assert lib.probav_engine_pair_kind(h) == _pair_kind(row, True)
    c = (ctypes.c_int32 * 4)()
    assert lib.probav_engine_route_counts(h, B, ctypes.byref(c)) == 0 and c[0] == 0 and c[2] == 0, tuple(c)
    lib.probav_engine_destroy(h)
    built = []
    build = cv._build
    monkeypatch.setattr(cv, "_build", lambda *a, **kw: built.append(build(*a, **kw)) or built[-1])
    cv._check_against_the_oracle(dev, row, T, gray, B, impl, P, "gemm-exotic %s x6 %d" % (_id(case), x6))
    m = built[0][0]
    assert len(built) == 1 and _exotic(m) == 1 and m.gemm_exotic is True and _arith(m) == x6 and _kind(m) == _pair_kind(row, True)       # the engine the check ran on
    _none_on_the_direct_kernels(m)


# ---- 2. layer by layer ------------------------------------------------------------------------------------------------------------------------------
LAYERED = [(c, impl, x6) for c, impl in ((A, 1), (C, 1), (D, 4)) for x6 in (0, 1)]


@pytest.mark.parametrize("case,impl,x6", LAYERED, ids=["%s-impl%d-x6%d" % (_id(c), i, x) for c, i, x in LAYERED])
def test_every_reducer_launch_of_a_forward_matches_the_single_operator_oracle(dev, case, impl, x6):
    """After a training forward: each of the ten reducers from its saved input, with its effective filter and bias, against an fp64 oracle written here --
    np.pad(mode="reflect") on H and W and, for reducers 1 and 2, on T (tests/test_gpu_parity.py::_oracle_conv zero-pads T), then oracle.wdsr_numpy.conv_valid,
    bias and ReLU.  Bar 2e-6 of max |ref|: the route's own single-operator bar, which its x6 kernels also meet."""
    from oracle import wdsr_numpy as on
    from probav_amd import introspect
    row, T, gray, B, P = case
    F, R = row[0], row[1]
    m = _model(dev, case, impl, x6=bool(x6))
    _step_of(dev, m, case)()
    _none_on_the_direct_kernels(m)
    flat = m.flat.detach()
    weff = introspect._effective_weights(m, flat, m.weight_cache())
    h, t = P + 6, T
    x = _view(m, B, 0, R).cpu().numpy().reshape(B, h, h, t, F)
    worst = 0.0
    plan = on.reducer_plan(T)
    assert len(plan) == 10 and plan[0] == (5, 2, 2) and plan[1] == (3, 2, 1)
    for k, (ks, p, pt) in enumerate(plan):
        Lh, off = _layer(m, "convReducer_%d" % (k + 1))
        w = weff[off: off + Lh.b_off - Lh.v_off].cpu().numpy().reshape(Lh.vshape)
        b = flat[Lh.b_off: Lh.b_off + Lh.cout].cpu().numpy()
        assert w.shape == (ks, ks, ks, F, F)
        xp = np.pad(x.astype(np.float64), [(0, 0), (p, p), (p, p), (pt, pt), (0, 0)], mode="reflect") if p or pt else x
        ref = np.maximum(on.conv_valid(xp, w) + b.astype(np.float64), 0.0)
        y = _view(m, B, 2, k)
        e = _err(y, ref)
        print("gemm exotic %s impl %d x6 %d convReducer_%d (k %d, mirrored pads %d %d %d): err / max |ref| = %.3g" % (_id(case), impl, x6, k + 1, ks, p, p, pt, e))
        worst = max(worst, e)
        x = y.cpu().numpy().reshape(ref.shape)
    assert x.shape == (B, P + 2, P + 2, 3, F)
    assert worst < 2e-6, worst


# ---- 3. switch on against switch off ----------------------------------------------------------------------------------------------------------------
AGAINST = [(A, 1), (A, 4), (D, 4)]


@pytest.mark.parametrize("case,impl", AGAINST, ids=["%s-impl%d" % (_id(c), i) for c, i in AGAINST])
def test_switch_on_against_switch_off(dev, case, impl):
    """The same engine and inputs with the switch on and off.  Both legs are held to the oracle by test 1, so the differences are printed, not bounded (they are recorded in
    profiles/gemm_exotic_accuracy.txt); asserted: each leg is bitwise reproducible, the legs differ (the switch did something), and a sample alone is the sample in its batch."""
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    m = _model(dev, case, impl, pair=True)
    step = _step_of(dev, m, case)
    on = step()
    _none_on_the_direct_kernels(m)
    assert _same(step(), on), "the switch on: a repeated step gives other bits"
    m.set_gemm_exotic(False)
    off = step()
    c = _launched(m)
    assert c[0] == 5 and c[2] == 4, c                              # the nine launches are back on the direct kernels
    assert _same(step(), off), "the switch off: a repeated step gives other bits"
    m.set_gemm_exotic(True)
    assert _same(step(), on)
    assert not torch.equal(on[0], off[0]), "the switch changed nothing: the exotic launches did not change hands"
    e_pred = float((on[0] - off[0]).abs().max() / off[0].abs().max())
    worst = (0.0, None)
    for name, key, a, b in cv._tensors(m):
        e = float((on[2][a:b] - off[2][a:b]).abs().max() / (off[2][a:b].abs().max() + 1e-30))
        if e > worst[0]:
            worst = (e, name + "/" + key)
    print("gemm exotic %s impl %d on against off: prediction %.3g of its max norm; worst gradient tensor %.3g of its max norm (%s)" % (_id(case), impl, e_pred, worst[0], worst[1]))
    # a sample alone: the same bits as in its batch (prediction; the forward's tiles straddle samples in row A)
    from probav_amd import synth
    x = torch.as_tensor(synth.synth_batch(B, seed=12, numImgLR=T, inChannels=1 if gray else 3, patchSizeLR=P)[0]).to(dev)
    with torch.no_grad():
        for s in range(B):
            assert torch.equal(m(x[s:s + 1].contiguous(), training=False), on[0][s:s + 1]), "sample %d depends on its batch mates" % s


# ---- 4. switch handling -----------------------------------------------------------------------------------------------------------------------------
def test_toggling_the_switch_between_two_steps(dev):
    always_on = _step_of(dev, _model(dev, A, 1), A)()
    always_off = _step_of(dev, _model(dev, A, 1, exotic=False), A)()
    assert not _same(always_on, always_off)
    m = _model(dev, A, 1, exotic=False)
    step = _step_of(dev, m, A)
    assert _same(step(), always_off) and _launched(m)[0] == 5
    m.set_gemm_exotic(True)
    assert _exotic(m) == 1 and _same(step(), always_on)
    _none_on_the_direct_kernels(m)
    m.set_gemm_exotic(False)
    assert _same(step(), always_off) and _launched(m)[2] == 4
    m.set_gemm_exotic(True)
    assert _same(step(), always_on)
    m.set_impl(4)                                                   # the other setters keep the wish ...
    m.set_gemm_pair(True)
    m.set_gemm_x6(False)
    assert m.gemm_exotic is True
    m.set_gemm_route(False)                                         # ... and the route decides whether it takes effect
    assert m.gemm_exotic is True
    _launched(m)
    step()
    c = _launched(m)
    assert c[1] == 0 and c[3] == 0 and c[0] > 5, c


def test_a_flip_between_forward_and_backward_is_refused(dev):
    from probav_amd import synth
    L, lib = _L(), _L().lib()
    row, T, gray, B, P = A
    m = _model(dev, A, 1)
    h = m._handle()
    x = torch.as_tensor(synth.synth_batch(B, seed=3, numImgLR=T, patchSizeLR=P)[0]).to(dev)
    n = B * 9 * P * P
    dy, y = torch.ones(n, device=dev), torch.empty(n, device=dev)
    flat = m.flat.detach()
    sizes = []
    for on in (1, 0):
        assert lib.probav_engine_set_gemm_exotic(h, on) == 0
        sizes.append(lib.probav_workspace_bytes(h, B, 1))
    assert sizes[0] != sizes[1]                                     # the four slab regions follow the switch
    ws = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
    for first in (1, 0):
        assert lib.probav_engine_set_gemm_exotic(h, first) == 0
        L.check(lib.probav_forward(h, L.ptr(flat), L.ptr(x), L.ptr(y), L.ptr(ws), ws.numel(), B, 1, L.current_stream()), "probav_forward")
        assert lib.probav_engine_set_gemm_exotic(h, 1 - first) == 0
        grads = torch.full((flat.numel(),), 7.0, device=dev)
        rc = lib.probav_backward(h, L.ptr(flat), L.ptr(dy), L.ptr(grads), L.ptr(ws), ws.numel(), B, L.current_stream())
        torch.cuda.synchronize()
        assert rc == L.PROBAV_EINVAL and bool((grads == 7.0).all()), (first, rc)
        assert lib.probav_engine_set_gemm_exotic(h, first) == 0     # flipped back: the backward of that forward runs
        L.check(lib.probav_backward(h, L.ptr(flat), L.ptr(dy), L.ptr(grads), L.ptr(ws), ws.numel(), B, L.current_stream()), "probav_backward")
        torch.cuda.synchronize()
        assert torch.isfinite(grads).all() and not bool((grads == 7.0).any())


# ---- 5. guard bands ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x6", [0, 1])
def test_bands_of_a_training_step(dev, x6):
    """probav_forward(training = 1) + probav_backward_split in the arena of tests/bands.py (row A): 0xFF / 0x00 fills of outputs and scratch, equal outputs, untouched
    bands and inputs, and the run on the late stream -- the route's kernels on the wide geometries write inside their outputs and slab regions only."""
    from probav_amd import synth
    row, T, gray, B, P = A
    L, lib = _L(), _L().lib()
    m = _model(dev, A, 4, x6=bool(x6))
    h = m._handle()
    Pp, S = L.ptr, L.current_stream
    flat = m.flat.detach().cpu().numpy().copy()
    x = np.ascontiguousarray(synth.synth_batch(B, seed=3, numImgLR=T, patchSizeLR=P)[0], dtype=np.float32)
    out = 3 * P
    dy = np.random.default_rng(4).standard_normal((B, out, out, 1)).astype(np.float32)
    saved, scr = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.probav_workspace_split(h, B, ctypes.byref(saved), ctypes.byref(scr)) == 0
    saved, scr = saved.value, scr.value
    bufs = [bands.inp("params", flat), bands.inp("x", x), bands.inp("dy", dy), bands.out("y", F32, B * out * out, lead_count=out * out),
            bands.out("grads", F32, flat.size), bands.scratch("saved", saved), bands.scratch("scratch", scr)]

    def step(t):
        rc = lib.probav_forward(h, Pp(t["params"]), Pp(t["x"]), Pp(t["y"]), Pp(t["saved"]), saved, B, 1, S())
        return rc or lib.probav_backward_split(h, Pp(t["params"]), Pp(t["dy"]), Pp(t["grads"]), Pp(t["saved"]), saved, Pp(t["scratch"]), scr, B, None, 0, S())
    assert lib.probav_engine_gemm_exotic(h) == 1
    _launched(m)
    rep = bands.check(bufs, step, dev)
    _none_on_the_direct_kernels(m)
    assert torch.isfinite(rep.outputs["grads"].view(F32)).all()
    bands.check_refusal(bufs, lambda t: lib.probav_backward_split(h, Pp(t["params"]), Pp(t["dy"]), Pp(t["grads"]), Pp(t["saved"]), saved, Pp(t["scratch"]), scr - 1, B, None, 0, S()),
                        dev, L.PROBAV_ENOSPACE)


# ---- 6. non-finite values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 4])
def test_a_non_finite_pixel_reaches_the_loss_and_spares_the_batch_mates(dev, impl):
    """Row A (three samples whose M tiles straddle samples): a NaN in one LR pixel of sample 1 reaches the loss and the gradient; every clean batch mate's prediction
    is the clean batch's bit for bit.  The mirrored layers have no zero padding; the pads-of-4 backward-data multiplies a padded tap by its zero, as elsewhere on
    the route ('The general matrix route')."""
    from probav_amd import synth
    from probav_amd.loss import Losses
    row, T, gray, B, P = A
    m = _model(dev, A, impl)
    lo = Losses(targetShape=(3 * P, 3 * P, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=302, numImgLR=T, patchSizeLR=P))

    def step(xx):
        m.flat.grad = None
        p = m(xx, training=True)
        l = lo.shiftCompensatedL1Loss(hr, mask, p)
        l.backward()
        return p.detach().clone(), float(l), m.flat.grad.detach().clone()
    clean = step(x)
    _none_on_the_direct_kernels(m)
    assert torch.isfinite(clean[0]).all() and np.isfinite(clean[1]) and torch.isfinite(clean[2]).all()
    poisoned, mates = 1, [0, 2]
    for pixel in ((poisoned, 4, 6, 8, 0), (poisoned, 0, 9, 18, 0)):       # interior; a corner, which the mirrored pads of the reducers read more than once
        xp = x.clone()
        xp[pixel] = float("nan")
        pred, loss, grad = step(xp)
        assert not np.isfinite(loss) and not torch.isfinite(grad).all() and not torch.isfinite(pred[poisoned]).all(), pixel
        assert torch.equal(pred[mates], clean[0][mates]), "a clean sample changed beside a poisoned one"
    assert _same(step(x), clean)
    _none_on_the_direct_kernels(m)


# ---- 7. the CLIs ------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_then_test_py_with_the_flags(dev, tmp_path):
    """The harness of tests/test_gpu_gemm_x6.py's last test on a 19-frame cfg of row A's size: train.py --gemm-route --gemm-pair --gemm-x6 --gemm-exotic runs two steps
    and resumes from a checkpoint written without the flags; test.py with the flags reads that checkpoint and its PNGs are within one grey level of test.py --gemm-route's."""
    from probav_amd import synth
    from probav_amd.pngio import imread_uint16
    from tests.test_gpu_cli import CFG, _run
    row, T, gray, _, P = A
    F, R, E, decay, Dc = row
    d = str(tmp_path)
    aug, res = os.path.join(d, "pre", "augmentedPatchesDir"), os.path.join(d, "pre", "resolverDir")
    os.makedirs(aug), os.makedirs(res)
    x, hr, mask = synth.synth_batch(4, seed=5, numImgLR=T, patchSizeLR=P)
    for tag, k in (("TRAIN", 4), ("TRAINVAL", 2)):
        np.ma.masked_array(x[:k], mask=np.zeros(x[:k].shape, bool)).dump(os.path.join(aug, "%spatchesLR_NIR.npy" % tag))
        np.ma.masked_array(hr[:k], mask=~mask[:k].astype(bool)).dump(os.path.join(aug, "%spatchesHR_NIR.npy" % tag))
    cfg_text = CFG.format(d=d)
    for old, new in (("num_filters=32", "num_filters=%d" % F), ("num_res_blocks=12", "num_res_blocks=%d" % R), ("batch_size=1", "batch_size=2"), ("exp_rate=8", "exp_rate=%d" % E),
                     ("decay_rate=0.8", "decay_rate=%s" % decay), ("num_low_res_imgs=9", "num_low_res_imgs=%d" % T), ("patch_size=16", "patch_size=%d" % P), ("patch_stride=16", "patch_stride=%d" % P),
                     ("num_low_res_imgs_pre=9", "num_low_res_imgs_pre=%d" % T)):
        assert cfg_text.count(old) == 1, old
        cfg_text = cfg_text.replace(old, new)
    sets, npatch = 2, 64                                             # 8 x 8 patches a scene, as test.py stitches them (here into 96 x 96 pixels)
    test_patches = synth.synth_batch(sets * npatch, seed=6, numImgLR=T, patchSizeLR=P)[0].reshape(sets, npatch, P + 6, P + 6, T, 1)
    np.ma.masked_array(test_patches.transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((sets, npatch, T, 1, P + 6, P + 6), bool)).dump(os.path.join(res, "TESTpatchesLR_NIR.npy"))
    cfg = os.path.join(d, "t19.cfg")
    with open(cfg, "w") as fh:
        fh.write(cfg_text)
    lib = _L().lib()
    h = make_engine(lib, F, R, E, Dc, T, 1, P)
    assert lib.probav_engine_set_gemm_route(h, 1) == 0 and lib.probav_engine_set_gemm_exotic(h, 1) == 0 and lib.probav_engine_gemm_exotic(h) == 1      # what the flags set
    c = (ctypes.c_int32 * 4)()
    assert lib.probav_engine_route_counts(h, 2, ctypes.byref(c)) == 0 and c[0] == 0 and c[2] == 0
    lib.probav_engine_destroy(h)
    flags = ["--gemm-route", "--gemm-pair", "--gemm-x6", "--gemm-exotic"]
    out = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
    assert "[ EPOCH 0/1 ] - [ STEP " in out.stderr and "/2 ]" in out.stderr, out.stderr[-2000:]          # two steps of batch 2
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.trainClass import ModelTrainer
    ck = os.path.join(d, "modelInfo", "ckpt_t19", "NIR")
    m = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, F, (3, 3, 3), R, E, decay, T, P, True, seed=3).to(dev)
    assert m.gemm_exotic is False and ModelTrainer(m, None, None, None, ck, os.path.join(d, "lg")).save() == "ckpt-1.pt"      # a checkpoint written without the flags
    images = []
    for fl in (flags, ["--gemm-route"]):
        for p in glob.glob(os.path.join(d, "testout_t19", "*.png")):
            os.remove(p)
        _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR"] + fl, cwd=d)
        pngs = sorted(glob.glob(os.path.join(d, "testout_t19", "*.png")))
        assert len(pngs) == sets, pngs
        images.append([imread_uint16(p).astype(np.int64) for p in pngs])
    for a, b in zip(*images):
        assert np.abs(a - b).max() <= 1
    out2 = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
    assert "Model restored from checkpoint at step 0" in out2.stdout
