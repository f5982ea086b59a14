"""The general matrix route's fused pointwise pair on the device (csrc/kernels_gemm_pw.hip; include/probav_hip.h, 'the route's fused pointwise pair').

The kernels have no single-operator entry point: they are reached, and held, through probav_forward / probav_backward* / probav_debug_hidden on engines whose
probav_engine_pair_kind is 2 -- every test asserts that first (a library without the pair ignores PROBAV_GEMM_PAIR and would pass the oracle checks un-fused).
The whole network against the fp64 oracle with tests/test_gpu_cfg_values.py's check and bars, unchanged; the forward's bits against the un-fused route's; the
hidden tile against the route's expConv launch, bit for bit; the launch census; the switch toggled between steps and flipped between a forward and its backward;
the guard bands of tests/bands.py; non-finite inputs and parameters; the weight cache; the CLIs.

Rows are (F, R, E, decay, D), T, gray, B, P -- the smallest shapes at which each tiling decision can go wrong: two row tiles each way and a voxel count that is
no multiple of anything (1), F no multiple of 32 and an odd chunk count (2), H3 neighbours that want the amax slots of dec and dX (3, 4), less than two chunks
with nothing aligned (5), 7 and 13 frames, three input channels (6, 7), and fewer voxel tiles than a workgroup's waves (8: P = 4)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests import bands
from tests.test_gemm_route_host import make_engine
from tests.test_gpu_gemm_route import _same, _stepper

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32

ROWS = [((64, 2, 8, 0.8, 51), 9, True, 3, 16), ((48, 2, 6, 0.9, 43), 9, True, 2, 16), ((32, 2, 8, 0.9, 28), 9, True, 2, 16), ((32, 2, 4, 0.8, 25), 9, True, 2, 16),
        ((20, 1, 3, 0.5, 10), 9, True, 2, 16), ((16, 2, 8, 0.75, 12), 7, True, 2, 16), ((64, 1, 8, 0.8, 51), 13, False, 2, 16), ((20, 1, 3, 0.5, 10), 9, True, 2, 4)]
SHIPPED = ((32, 12, 8, 0.8, 25), 9, True, 2, 16)


def _id(c):
    return "f%d-r%d-e%d-d%d-t%d-b%d-p%d" % (c[0][0], c[0][1], c[0][2], c[0][4], c[1], c[3], c[4])


def _L():
    from probav_amd import _lib as L
    return L


def _kind(m):
    return _L().lib().probav_engine_pair_kind(m._handle())


def _model(dev, row, T=9, gray=True, seed=11, P=16, impl=None):
    """The network on the route with the pair on: probav_engine_pair_kind == 2, or the test has nothing to say."""
    from tests import test_gpu_cfg_values as cv
    m = cv._build(dev, row, T, gray, seed, P)[0]
    if impl is not None:
        m.set_impl(impl)
    m.set_gemm_route(True)
    m.set_gemm_pair(True)
    assert m.gemm_pair is True and _kind(m) == (1 if row == SHIPPED[0] else 2)
    return m


@pytest.fixture(autouse=True)
def _keep_workspaces(monkeypatch):
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")                      # the gates and the saved block inputs are read from a pass's workspace


@pytest.fixture(scope="module", autouse=True)
def _release_the_arena(dev):
    yield
    bands.release(dev)


# ---- the whole network against the fp64 oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 4])
@pytest.mark.parametrize("case", ROWS, ids=[_id(c) for c in ROWS])
def test_whole_network_with_the_pair_matches_the_oracle(dev, case, impl, monkeypatch):
    """tests/test_gpu_cfg_values.py::_check_against_the_oracle, unchanged, on engines created with PROBAV_GEMM_ROUTE=1 PROBAV_GEMM_PAIR=1: output 2e-5, loss 1e-5,
    every gradient tensor 1e-3 at the device's gates -- which now come from probav_debug_hidden -- and its bit-for-bit properties: repeated step, training =
    inference, sample alone, side-stream mode."""
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    monkeypatch.setenv("PROBAV_GEMM_ROUTE", "1")
    monkeypatch.setenv("PROBAV_GEMM_PAIR", "1")
    lib = _L().lib()
    h = make_engine(lib, row[0], row[1], row[2], row[4], T, 1 if gray else 3, P)
    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_pair_kind(h) == 2
    lib.probav_engine_destroy(h)
    built = []
    build = cv._build
    monkeypatch.setattr(cv, "_build", lambda *a, **kw: built.append(build(*a, **kw)) or built[-1])
    cv._check_against_the_oracle(dev, row, T, gray, B, impl, P, "gemm-pair " + _id(case))
    assert len(built) == 1 and _kind(built[0][0]) == 2 and built[0][0].gemm_pair is True       # the engine the check ran on


# ---- forward bits ---------------------------------------------------------------------------------------------------------------------------------
def _view(m, B, kind, idx):
    L = _L()
    off, cnt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().probav_workspace_view(m._handle(), B, 1, kind, idx, ctypes.byref(off), ctypes.byref(cnt)), "probav_workspace_view")
    return m._workspace(B, True)[off.value: off.value + cnt.value]


def _layer(m, name):
    """(layer, offset of its filter in the effective-weight tensor)."""
    off = 0
    for Lh in m.layers:
        if Lh.name == name:
            return Lh, off
        off += Lh.b_off - Lh.v_off
    raise KeyError(name)


def _route_conv(x, w, bias, nvox, cin, cout, relu):
    """probav_gemm_conv3d_forward of a 1x1x1 layer on [nvox][cin]: the launch of the un-fused route."""
    L = _L()
    g = (ctypes.c_int32 * 17)(1, nvox, 1, 1, cin, nvox, 1, 1, cout, 1, 1, 1, 0, 0, 0, 0, relu)
    y = torch.full((nvox * cout,), float("nan"), device=x.device)
    L.check(L.lib().probav_gemm_conv3d_forward(ctypes.byref(g), L.ptr(x), None, L.ptr(w), L.ptr(bias), None, L.ptr(y), L.current_stream()), "probav_gemm_conv3d_forward")
    return y


@pytest.mark.parametrize("impl", [1, 4])
@pytest.mark.parametrize("case", [ROWS[0], ROWS[3], ROWS[4]], ids=[_id(ROWS[0]), _id(ROWS[3]), _id(ROWS[4])])
def test_forward_bits_are_the_unfused_routes(dev, case, impl):
    from probav_amd import introspect, synth
    from tests import test_gpu_cfg_values as cv
    row, T, gray, B, P = case
    F, R, E, decay, D = row
    H = F * E
    m = _model(dev, row, T, gray, impl=impl)
    step = _stepper(dev, m, B, T, 1 if gray else 3)
    x = torch.as_tensor(synth.synth_batch(B, seed=12, numImgLR=T, inChannels=1 if gray else 3)[0]).to(dev)      # (the stepper's own input)
    on = step()
    with torch.no_grad():
        on_inf = m(x, training=False).clone()
    # block 0's hidden tile and output from the fused forward kernel, against the route's own launches on the saved block input
    L = _L()
    on2 = step()                                                   # (the training pass whose workspace is read below)
    assert _same(on, on2)
    act0 = _view(m, B, 0, 0)
    nvox = act0.numel() // F
    flat = m.flat.detach()
    hid = torch.full((nvox * H,), float("nan"), device=dev)
    dec = torch.full((nvox * D,), float("nan"), device=dev)
    ws = m._workspace(B, True)
    L.check(L.lib().probav_debug_hidden(m._handle(), L.ptr(flat), L.ptr(ws), ws.numel() * 4, B, 0, L.ptr(hid), L.ptr(dec), L.ptr(m.weight_cache()), L.current_stream()),
            "probav_debug_hidden")
    weff = introspect._effective_weights(m, flat, m.weight_cache())
    (le, oe), (ld, od) = _layer(m, "expConv_0"), _layer(m, "decConv_0")
    w1, b1 = weff[oe: oe + F * H], flat[le.b_off: le.b_off + H]
    w2, b2 = weff[od: od + H * D], flat[ld.b_off: ld.b_off + D]
    hid_route = _route_conv(act0, w1, b1, nvox, F, H, 1)
    assert torch.equal(hid, hid_route), "the fused kernel's hidden tile is not the route's expConv, bit for bit"
    assert torch.equal(dec, _route_conv(hid_route, w2, b2, nvox, H, D, 0)), "the fused kernel's output is not the route's decConv, bit for bit"
    assert torch.equal(dec, _view(m, B, 1, 0)), "probav_debug_hidden's output is not what the forward pass saved"
    x64, w1_64, w2_64 = act0.double().view(nvox, F).cpu().numpy(), w1.double().view(F, H).cpu().numpy(), w2.double().view(H, D).cpu().numpy()
    ref_h = np.maximum(x64 @ w1_64 + b1.double().cpu().numpy(), 0.0)
    ref_d = ref_h @ w2_64 + b2.double().cpu().numpy()
    e_h = np.abs(hid.double().view(nvox, H).cpu().numpy() - ref_h).max() / np.abs(ref_h).max()
    e_d = np.abs(dec.double().view(nvox, D).cpu().numpy() - ref_d).max() / np.abs(ref_d).max()
    print("gemm pair %s impl %d: hidden err / max |ref| = %.3g, dec err / max |ref| = %.3g" % (_id(case), impl, e_h, e_d))
    assert e_h < 2e-6 and e_d < 2e-6, (e_h, e_d)
    # the un-fused route: the same prediction and loss, bit for bit; gradients to fp32 rounding
    m.set_gemm_pair(False)
    assert _kind(m) == 0
    off = step()
    with torch.no_grad():
        off_inf = m(x, training=False).clone()
    assert torch.equal(on[0], off[0]) and on[1] == off[1], "the fused forward is not the un-fused route's, bit for bit"
    assert torch.equal(on_inf, off_inf) and torch.equal(on_inf, on[0])
    worst = (0.0, None)
    for name, key, a, b in cv._tensors(m):
        e = float((on[2][a:b] - off[2][a:b]).abs().max() / (off[2][a:b].abs().max() + 1e-30))
        if e > worst[0]:
            worst = (e, name + "/" + key)
    print("gemm pair %s impl %d: largest gradient difference to the un-fused route, of a tensor's max norm: %.3g (%s)" % (_id(case), impl, worst[0], worst[1]))
    assert worst[0] < 1e-5, worst


# ---- census ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 4])
@pytest.mark.parametrize("case", [ROWS[0], ROWS[4], SHIPPED], ids=[_id(ROWS[0]), _id(ROWS[4]), "shipped"])
def test_the_census_is_what_a_step_launches_with_the_pair(dev, case, impl):
    row, T, gray, B, P = case
    lib = _L().lib()
    m = _model(dev, row, T, gray, impl=impl)
    step = _stepper(dev, m, B, T, 1 if gray else 3)
    got, want = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert lib.probav_engine_launched_counts(m._handle(), ctypes.byref(got), 1) == 0            # (clear)
    step()
    assert lib.probav_engine_launched_counts(m._handle(), ctypes.byref(got), 1) == 0
    assert lib.probav_engine_route_counts(m._handle(), B, ctypes.byref(want)) == 0
    print("census with the pair %s impl %d: %s" % (_id(case), impl, tuple(want)))
    assert tuple(got) == tuple(want)


# ---- toggling -------------------------------------------------------------------------------------------------------------------------------------
def test_toggling_the_pair_between_steps(dev):
    m = _model(dev, (64, 1, 8, 0.8, 51), impl=1)
    step = _stepper(dev, m)
    m.set_gemm_pair(False)
    off = step()
    m.set_gemm_pair(True)
    assert _kind(m) == 2
    on = step()
    assert torch.equal(on[0], off[0]) and on[1] == off[1]           # the forward's bits ...
    assert not torch.equal(on[2], off[2])                           # ... and another order of additions in the reverse pass
    m.set_gemm_pair(False)
    assert _same(step(), off)
    m.set_gemm_pair(True)
    assert _same(step(), on)
    m.set_impl(4)                                                   # set_impl keeps the switch
    assert m.gemm_pair is True and _kind(m) == 2
    m.set_gemm_route(False)                                         # ... and so does the route's, which alone decides whether the wish takes effect
    assert m.gemm_pair is True and _kind(m) == 0


def test_a_flip_between_forward_and_backward_is_refused(dev):
    from probav_amd import synth
    L, lib = _L(), _L().lib()
    B = 2
    m = _model(dev, (20, 1, 3, 0.5, 10), impl=1)
    h = m._handle()
    x = torch.as_tensor(synth.synth_batch(B, seed=3)[0]).to(dev)
    dy = torch.ones(B * 48 * 48, device=dev)
    y = torch.empty(B * 48 * 48, device=dev)
    flat = m.flat.detach()
    sizes = []
    for pair in (1, 0):
        assert lib.probav_engine_set_gemm_pair(h, pair) == 0
        sizes.append(lib.probav_workspace_bytes(h, B, 1))
    ws = torch.empty(max(sizes), dtype=torch.uint8, device=dev)     # (large enough for either layout: the refusal is the form's, not the size's)
    for first in (1, 0):
        assert lib.probav_engine_set_gemm_pair(h, first) == 0
        L.check(lib.probav_forward(h, L.ptr(flat), L.ptr(x), L.ptr(y), L.ptr(ws), ws.numel(), B, 1, L.current_stream()), "probav_forward")
        assert lib.probav_engine_set_gemm_pair(h, 1 - first) == 0
        grads = torch.full((flat.numel(),), 7.0, device=dev)
        rc = lib.probav_backward(h, L.ptr(flat), L.ptr(dy), L.ptr(grads), L.ptr(ws), ws.numel(), B, L.current_stream())
        torch.cuda.synchronize()
        assert rc == L.PROBAV_EINVAL and bool((grads == 7.0).all()), (first, rc)
        assert lib.probav_engine_set_gemm_pair(h, first) == 0       # flipped back: the backward of that forward runs
        L.check(lib.probav_backward(h, L.ptr(flat), L.ptr(dy), L.ptr(grads), L.ptr(ws), ws.numel(), B, L.current_stream()), "probav_backward")
        torch.cuda.synchronize()
        assert torch.isfinite(grads).all() and not bool((grads == 7.0).any())


# ---- buffers, poisoned scratch, the stream --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ROWS[4], ROWS[7]], ids=[_id(ROWS[4]), _id(ROWS[7])])
def test_bands_of_a_training_step_with_the_pair(dev, case):
    """probav_forward(training = 1) + probav_backward_split in the arena of tests/bands.py: 0xFF / 0x00 fills of outputs and scratch, equal outputs, untouched
    bands and inputs, and the run on the late stream -- the fused kernels write inside dec, dX and their slab region only, and on the stream they were given."""
    from probav_amd import synth
    row, T, gray, B, P = case
    L, lib = _L(), _L().lib()
    m = _model(dev, row, T, gray, P=P, impl=4)
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
    rep = bands.check(bufs, step, dev)
    assert torch.isfinite(rep.outputs["grads"].view(F32)).all()
    bands.check_refusal(bufs, lambda t: lib.probav_backward_split(h, Pp(t["params"]), Pp(t["dy"]), Pp(t["grads"]), Pp(t["saved"]), saved, Pp(t["scratch"]), scr - 1, B, None, 0, S()),
                        dev, L.PROBAV_ENOSPACE)


# ---- non-finite values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 4])
def test_non_finite_values_with_the_pair(dev, impl):
    from probav_amd import synth
    from probav_amd.loss import Losses
    row, T, gray, B, P = ROWS[4]
    m = _model(dev, row, T, gray, impl=impl)
    lo = Losses(targetShape=(48, 48, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=12, numImgLR=T))

    def step(xx):
        m.flat.grad = None
        p = m(xx, training=True)
        l = lo.shiftCompensatedL1Loss(hr, mask, p)
        l.backward()
        return p.detach().clone(), float(l), m.flat.grad.detach().clone()
    clean = step(x)
    assert torch.isfinite(clean[0]).all() and np.isfinite(clean[1]) and torch.isfinite(clean[2]).all()
    xp = x.clone()
    xp[0, 9, 11, 4, 0] = float("nan")
    xp[0, 3, 17, 2, 0] = float("inf")
    pred, loss, grad = step(xp)
    assert torch.equal(pred[1], clean[0][1]), "a clean sample changed beside a poisoned one"
    assert not torch.isfinite(pred[0]).all() and not np.isfinite(loss) and not torch.isfinite(grad).all()
    # a NaN in expConv_0's bias reaches every voxel's hidden tile
    Lh = next(l for l in m.layers if l.name == "expConv_0")
    with torch.no_grad():
        keep = m.flat[Lh.b_off].clone()
        m.flat[Lh.b_off] = float("nan")
    try:
        pred, loss, grad = step(x)
        assert not torch.isfinite(pred[0]).any() and not torch.isfinite(pred[1]).any() and not np.isfinite(loss) and not torch.isfinite(grad).all()
    finally:
        with torch.no_grad():
            m.flat[Lh.b_off] = keep
    assert _same(step(x), clean)


# ---- the weight cache -----------------------------------------------------------------------------------------------------------------------------
def test_optimizer_steps_and_the_weight_cache_with_the_pair(dev):
    """tests/test_gpu_gemm_route.py::test_optimizer_steps_and_the_weight_cache_on_the_route with the pair on: the fused kernels read weff, cached or not."""
    from probav_amd.trainClass import make_optimizer
    m = _model(dev, (64, 1, 8, 0.8, 51), seed=4164)
    step = _stepper(dev, m)
    opt = make_optimizer("nadam", m, 5e-4)
    for k in range(2):
        assert (m.weight_cache() is not None) == (k > 0)
        step()
        opt.step()
    assert m.weight_cache() is not None and _kind(m) == 2
    cached = step()
    m._wcache_version = None
    assert m.weight_cache() is None
    assert _same(step(), cached)


# ---- the CLIs -------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_then_test_py_with_both_flags(dev, tmp_path):
    """The harness of tests/test_gpu_gemm_route.py::test_train_py_then_test_py_with_the_flag: train.py --gemm-route --gemm-pair runs two steps; the PNGs of
    test.py --gemm-route --gemm-pair are those of test.py --gemm-route byte for byte (the forward's bits are equal)."""
    from probav_amd import synth
    from tests.test_gpu_cli import CFG, _run
    d = str(tmp_path)
    aug, res = os.path.join(d, "pre", "augmentedPatchesDir"), os.path.join(d, "pre", "resolverDir")
    os.makedirs(aug), os.makedirs(res)
    x, hr, mask = synth.synth_batch(4, seed=5)
    for tag, k in (("TRAIN", 4), ("TRAINVAL", 2)):
        np.ma.masked_array(x[:k], mask=np.zeros(x[:k].shape, bool)).dump(os.path.join(aug, "%spatchesLR_NIR.npy" % tag))
        np.ma.masked_array(hr[:k], mask=~mask[:k].astype(bool)).dump(os.path.join(aug, "%spatchesHR_NIR.npy" % tag))
    sets = 2
    test_patches = synth.synth_batch(sets * 64, seed=6)[0].reshape(sets, 64, 22, 22, 9, 1)
    np.ma.masked_array(test_patches.transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((sets, 64, 9, 1, 22, 22), bool)).dump(os.path.join(res, "TESTpatchesLR_NIR.npy"))
    cfg = os.path.join(d, "f64.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d).replace("num_filters=32", "num_filters=64").replace("num_res_blocks=12", "num_res_blocks=2").replace("batch_size=1", "batch_size=2"))
    lib = _L().lib()
    h = make_engine(lib, 64, 2, 8, 51, 9)
    assert lib.probav_engine_set_gemm_route(h, 1) == 0 and lib.probav_engine_set_gemm_pair(h, 1) == 0 and lib.probav_engine_pair_kind(h) == 2      # what the flags set
    lib.probav_engine_destroy(h)
    out = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR", "--gemm-route", "--gemm-pair"], cwd=d)
    assert "[ EPOCH 0/1 ] - [ STEP " in out.stderr and "/2 ]" in out.stderr, out.stderr[-2000:]          # two steps of batch 2
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.trainClass import ModelTrainer
    ck = os.path.join(d, "modelInfo", "ckpt_f64", "NIR")
    m = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, 64, (3, 3, 3), 2, 8, 0.8, 9, 16, True, seed=3).to(dev)
    assert ModelTrainer(m, None, None, None, ck, os.path.join(d, "lg")).save() == "ckpt-1.pt"
    images = []
    for flags in (["--gemm-route", "--gemm-pair"], ["--gemm-route"]):
        for p in glob.glob(os.path.join(d, "testout_f64", "*.png")):
            os.remove(p)
        _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
        pngs = sorted(glob.glob(os.path.join(d, "testout_f64", "*.png")))
        assert len(pngs) == sets, pngs
        images.append([open(p, "rb").read() for p in pngs])
    assert images[0] == images[1]
