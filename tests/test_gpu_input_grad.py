"""Input gradients on the device: d loss / d LR frames from probav::wdsr_forward (probav::wdsr_backward_input, probav_backward_input) and the
kernel behind it alone (probav_input_grad through ctypes).

Bars.  The kernel alone: max error over max |ref| under the 2e-6 that test_conv3d_forward_matches_oracle holds every convolution to, against the
fp64 numpy statement of its formula (tests/input_grad_helpers.py).  The whole network at the device's ReLU gates (families 3 and 4): 1e-3 of the
tensor's max norm, the bar _gate_masked_parity holds the 132 weight gradients to.  Families 0 - 2 (which do not expose their gates) and the other
patch size: the relative-L2 bar of the fp32-family tests, imported from tests/test_gpu_parity.py."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from probav_amd import synth
from tests import load_golden
from tests.input_grad_helpers import input_grad_numpy, oracle_input_grad
from tests.test_gpu_parity import _grad_l2_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _keep_workspaces(monkeypatch):
    """device_gates reads a pass's workspace after its backward has run."""
    monkeypatch.setenv("PROBAV_KEEP_WS", "1")


def _lib():
    from probav_amd import _lib as L
    return L


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
# (H = W, T, C, B): every 'same' border in h, w and t with the smallest image the residual chain admits (7); more than one tile per sample and tiles that
# overhang the image (22, 30, 38); the largest row (T = 19); three input channels; 38: the size whose residual path the engine runs un-fused (gate1 given)
KERNEL_CASES = [(7, 1, 1, 1), (8, 3, 3, 2), (22, 9, 1, 2), (22, 19, 1, 1), (30, 13, 3, 1), (38, 9, 1, 1)]


def _kernel_inputs(H, T, C, B, closed=False):
    rng = np.random.default_rng(1000 * H + 10 * T + C)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    act0 = f(B, H, H, T, 32)                                   # a normal draw: about half of the gates are closed
    if closed:
        act0 = -np.abs(act0)
        act0[0, 0, 0, 0, :4] = 0.0                             # (a post-ReLU zero is a closed gate)
    return dict(g=f(B, H, H, T, 32), act0=act0, wmain=0.2 * f(3, 3, 3, C, 32), d1=f(B, H - 2, H - 2, 9), gate1=f(B, H - 2, H - 2, 9), w1=0.3 * f(3, 3, 1, C, 9))


def _run_kernel(dev, z, H, T, C, B, std, gated):
    L = _lib()
    d = {k: _t(v, dev) for k, v in z.items()}
    dx = torch.full((B, H, H, T, C), float("nan"), device=dev)
    L.check(L.lib().probav_input_grad(B, H, T, C, L.ptr(d["g"]), L.ptr(d["act0"]), L.ptr(d["wmain"]), L.ptr(d["d1"]), L.ptr(d["gate1"]) if gated else None,
                                      L.ptr(d["w1"]), std, L.ptr(dx), L.current_stream()), "probav_input_grad")
    torch.cuda.synchronize()
    return dx.cpu().double().numpy()


@pytest.mark.parametrize("H,T,C,B", KERNEL_CASES, ids=["h%d-t%d-c%d-b%d" % c for c in KERNEL_CASES])
def test_kernel_matches_the_fp64_formula(dev, H, T, C, B):
    z = _kernel_inputs(H, T, C, B)
    std = 3160.7272
    for gated in (True, False):                                # gate1 given (the un-fused residual route) and d1 taken as it is (the fused one)
        got = _run_kernel(dev, z, H, T, C, B, std, gated)
        ref, main, res = input_grad_numpy(z["g"], z["act0"], z["wmain"], z["d1"], z["gate1"] if gated else None, z["w1"], std)
        e = np.abs(got - ref).max() / np.abs(ref).max()
        print("probav_input_grad H %d T %d C %d B %d gate1 %s: max err / max |ref| = %.3e (residual share %.2f of max |ref|)"
              % (H, T, C, B, gated, e, np.abs(res).max() / np.abs(ref).max()))
        assert np.isfinite(got).all()
        assert e < 2e-6, e


def test_kernel_with_every_gate_closed_is_the_residual_share(dev):
    H, T, C, B = 22, 9, 1, 2
    z = _kernel_inputs(H, T, C, B, closed=True)
    got = _run_kernel(dev, z, H, T, C, B, 2.5, True)
    ref, main, res = input_grad_numpy(z["g"], z["act0"], z["wmain"], z["d1"], z["gate1"], z["w1"], 2.5)
    assert np.abs(main).max() == 0.0                           # the main path's share is exactly 0 ...
    assert np.array_equal(got[:, :, :, 0], got[:, :, :, T - 1])   # ... so every frame holds the same value: the residual share
    e = np.abs(got - res).max() / np.abs(res).max()
    assert e < 2e-6, e


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole network
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(dev, T=9, C=1, P=16, params=None, seed=0):
    from probav_amd.modelsTF import WDSRConv3D
    m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, T, P, C == 1, seed=seed)
    if params is not None:
        m.load_variables(params)
    return m.to(dev)


def _inputs(T, B, C):
    if (T, B, C) == (9, 2, 1):
        z = load_golden("wdsr_t9_b2")
        return z["x"], z["hr"], z["mask"]
    return synth.synth_batch(B, seed=300 + 10 * T + B, numImgLR=T, inChannels=C)


def _params(T, C):
    return synth.synth_params(seed=101, perturb=True, numImgLR=T, inChannels=C)


def _step(m, x, hr, mask, S=48, x_grad=True):
    """forward + L1 loss + backward -> (x.grad or None, flat.grad or None, loss)"""
    from probav_amd.loss import Losses
    m.flat.grad = None
    xd = x.detach().clone().requires_grad_(x_grad)
    loss = Losses(targetShape=(S, S, 1)).shiftCompensatedL1Loss(hr, mask, m(xd, training=True))
    loss.backward()
    return xd.grad, (None if m.flat.grad is None else m.flat.grad.detach().clone()), loss.detach()


GATED_CASES = [(9, 2, 1), (9, 2, 3), (7, 3, 1), (13, 2, 1), (19, 2, 1)]


@pytest.mark.parametrize("impl", [3, 4], ids=["x6", "h3"])
@pytest.mark.parametrize("T,B,C", GATED_CASES, ids=["t%d-b%d-c%d" % c for c in GATED_CASES])
def test_input_gradient_matches_the_oracle_at_the_devices_gates(dev, T, B, C, impl):
    from probav_amd.introspect import device_gates
    x, hr, mask = _inputs(T, B, C)
    params = _params(T, C)
    m = _model(dev, T, C, params=params)
    m.set_impl(impl)
    dx, _, loss = _step(m, *(torch.as_tensor(a).to(dev) for a in (x, hr, mask)))
    assert dx is not None and tuple(dx.shape) == tuple(x.shape) and dx.dtype == torch.float32
    gates = device_gates(m, m.flat.detach(), B, T)
    ref, loss_o = oracle_input_grad(x, hr, mask, params, synth.NIR_MEAN, synth.NIR_STD, T, gates)
    assert abs(float(loss) - loss_o) < 1e-5 * loss_o
    e = np.abs(dx.cpu().double().numpy() - ref).max() / np.abs(ref).max()
    print("impl %d T %d B %d C %d: x.grad max err / max |ref| = %.3e at the device's gates" % (impl, T, B, C, e))
    assert e < 1e-3, e


@functools.lru_cache(maxsize=None)
def _ungated_reference():
    x, hr, mask = _inputs(9, 2, 1)
    return oracle_input_grad(x, hr, mask, _params(9, 1), synth.NIR_MEAN, synth.NIR_STD, 9)[0]


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_input_gradient_on_the_fp32_families(dev, impl):
    """Families 0 - 2 do not expose their gates: relative L2 against the un-gated fp64 oracle, the bar of the fp32-family gradient tests."""
    x, hr, mask = _inputs(9, 2, 1)
    m = _model(dev, params=_params(9, 1))
    m.set_impl(impl)
    dx, _, _ = _step(m, *(torch.as_tensor(a).to(dev) for a in (x, hr, mask)))
    ref = _ungated_reference()
    e = np.sqrt(((dx.cpu().double().numpy() - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum())
    print("impl %d: x.grad relative L2 error against the un-gated oracle = %.3e" % (impl, e))
    assert e < _grad_l2_tol(9, impl), e


def test_other_patch_size_agrees_across_engines(dev):
    """P = 24 (inputs 30 wide): the generic kernels with the un-fused residual path (impl 0) against the default family."""
    P, T, B = 24, 9, 2
    m = _model(dev, T, 1, P, seed=3)
    rng = np.random.default_rng(P * 100 + T)
    x = torch.as_tensor((rng.uniform(size=(B, P + 6, P + 6, T, 1)) * 8000).astype(np.float32)).to(dev)
    hr = torch.as_tensor((rng.uniform(size=(B, 3 * P, 3 * P, 1)) * 8000).astype(np.float32)).to(dev)
    mask = torch.as_tensor((rng.uniform(size=(B, 3 * P, 3 * P, 1)) > 0.1).astype(np.float32)).to(dev)
    res = []
    for impl in (0, 4):
        m.set_impl(impl)
        res.append(_step(m, x, hr, mask, S=3 * P)[0])
    assert torch.isfinite(res[1]).all() and float(res[0].abs().max()) > 0
    assert float((res[0] - res[1]).norm()) < _grad_l2_tol(T, 0) * float(res[0].norm())


# ---------------------------------------------------------------------------------------------------------------------------------
# nothing existing moves
# ---------------------------------------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch):
    """Counting wrappers around the two C entry points of the reverse pass."""
    lib = _lib().lib()
    n = {"probav_backward_split": 0, "probav_backward_input": 0}
    for name in n:
        fn = getattr(lib, name)

        def wrapped(*a, _fn=fn, _name=name):
            n[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    return n


@pytest.mark.parametrize("impl", [4, 0], ids=["h3", "generic"])
def test_parameter_gradients_keep_their_bits_and_the_plain_op_stays_in_use(dev, impl, monkeypatch):
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in _inputs(9, 2, 1))
    m = _model(dev, params=_params(9, 1))
    m.set_impl(impl)
    n = _count_calls(monkeypatch)
    dx0, g_plain, _ = _step(m, x, hr, mask, x_grad=False)
    assert dx0 is None and n == {"probav_backward_split": 1, "probav_backward_input": 0}          # x does not require grad: the plain op, once
    dx1, g1, _ = _step(m, x, hr, mask)
    assert n == {"probav_backward_split": 1, "probav_backward_input": 1}
    assert torch.equal(_bits(g1), _bits(g_plain))                                                  # flat.grad of the same call: bit for bit the plain backward's
    dx2, g2, _ = _step(m, x, hr, mask)
    assert torch.equal(_bits(dx2), _bits(dx1)) and torch.equal(_bits(g2), _bits(g_plain))          # two runs: identical bits
    _, g3, _ = _step(m, x, hr, mask, x_grad=False)
    assert torch.equal(_bits(g3), _bits(g_plain))                                                  # ... and the plain pass after it is the plain pass
    # frozen weights: the pass computes the filter gradients and drops them; x.grad has the same bits
    m.flat.requires_grad_(False)
    try:
        dx3, g4, _ = _step(m, x, hr, mask)
    finally:
        m.flat.requires_grad_(True)
    assert g4 is None and torch.equal(_bits(dx3), _bits(dx1))
    assert n == {"probav_backward_split": 2, "probav_backward_input": 3}


def test_eval_mode_forward_still_refuses_backward(dev):
    m = _model(dev, params=_params(9, 1))
    x = torch.as_tensor(_inputs(9, 2, 1)[0]).to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="training=True"):
        m(x, training=False).sum().backward()
    with m.weights_from(m.flat.detach().clone()):
        with pytest.raises(RuntimeError, match="weights_from"):
            m(x, training=True)
    assert x.grad is None


def test_an_inf_in_dy_stays_in_its_sample(dev):
    """INTEGRATION.md, 'Non-finite values': an inf planted in sample 0's output gradient makes that sample's dx non-finite; sample 1's dx keeps its bits."""
    m = _model(dev, params=_params(9, 1))
    x = torch.as_tensor(_inputs(9, 2, 1)[0]).to(dev)
    dy = torch.as_tensor(np.random.default_rng(5).normal(size=(2, 48, 48, 1)).astype(np.float32)).to(dev)

    def run(dy_):
        xd = x.detach().clone().requires_grad_(True)
        m.flat.grad = None
        m(xd, training=True).backward(dy_)
        return xd.grad
    clean = run(dy)
    assert torch.isfinite(clean).all()
    bad = dy.clone()
    bad[0, 20, 21, 0] = float("inf")
    got = run(bad)
    assert not torch.isfinite(got[0]).all()
    assert torch.equal(_bits(got[1]), _bits(clean[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_opcheck_and_direct_use_of_the_op(dev):
    m = _model(dev, params=_params(9, 1))
    x = torch.as_tensor(_inputs(9, 2, 1)[0]).to(dev)
    eng = int(m._handle().value)
    flat = m.flat.detach().clone().requires_grad_(True)
    xg = x.detach().clone().requires_grad_(True)
    # (the workspace output holds uninitialised scratch beyond the saved activations: the output-comparing AOT test is left out, as in tests/test_gpu_ops.py)
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.probav.wdsr_forward.default, (flat, xg, eng, 48, True), test_utils=tests)
    torch.library.opcheck(torch.ops.probav.wdsr_forward.default, (flat.detach(), xg, eng, 48, True), test_utils=tests)
    y, ws = torch.ops.probav.wdsr_forward(flat, xg, eng, 48, True)
    dy = torch.randn_like(y)
    torch.library.opcheck(torch.ops.probav.wdsr_backward_input.default, (flat.detach(), dy, ws.clone(), eng), test_utils=("test_schema", "test_faketensor"))
    g, dx = torch.ops.probav.wdsr_backward_input(flat.detach(), dy, ws, eng)
    assert tuple(dx.shape) == tuple(x.shape) and tuple(g.shape) == tuple(flat.shape)
    (y * dy).sum().backward()
    assert torch.equal(_bits(xg.grad), _bits(dx)) and torch.equal(_bits(flat.grad), _bits(g))
    assert torch.equal(_bits(g), _bits(torch.ops.probav.wdsr_backward(flat.detach(), dy, ws, eng)))


def test_compiled_step_with_an_input_that_requires_grad(dev):
    m = _model(dev, params=_params(9, 1))
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in _inputs(9, 2, 1))
    mk = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
    eng = int(m._handle().value)

    def step(flat, x, hr, mk):
        y, _ = torch.ops.probav.wdsr_forward(flat, x, eng, 48, True)
        return torch.ops.probav.shift_loss(y, hr, mk, 3, 16, 1)[0]
    flat = m.flat.detach().clone().requires_grad_(True)
    xg = x.detach().clone().requires_grad_(True)
    step(flat, xg, hr, mk).backward()
    want_x, want_f = xg.grad.clone(), flat.grad.clone()
    flat.grad = xg.grad = None
    try:                                                       # ONLY a torch build without dynamo may skip
        dynamo = importlib.import_module("torch._dynamo")
        dynamo.reset()
        cstep = torch.compile(step, backend="aot_eager", fullgraph=True)
    except (ImportError, ModuleNotFoundError) as exc:
        pytest.skip("torch.compile (dynamo) is not part of this torch build: %r" % (exc,))
    cstep(flat, xg, hr, mk).backward()
    assert torch.equal(_bits(xg.grad), _bits(want_x)) and torch.equal(_bits(flat.grad), _bits(want_f))


def test_frame_shares_of_the_golden_batch_sum_to_one(dev):
    from probav_amd.attribution import frame_shares, input_gradient
    from probav_amd.loss import Losses
    x, hr, mask = _inputs(9, 2, 1)
    m = _model(dev, params=_params(9, 1))
    lo = Losses(targetShape=(48, 48, 1))
    dx = input_gradient(m, lo.shiftCompensatedL1Loss, x, hr, mask, micro_batch=128)
    assert tuple(dx.shape) == tuple(x.shape) and m.flat.grad is None
    s = frame_shares(dx)
    assert tuple(s.shape) == (2, 9) and float((s.sum(1) - 1).abs().max()) < 1e-12 and float(s.min()) > 0
    # micro-batches of one: every sample still receives the gradient of its own loss (the batch-mean loss scaled by the micro-batch size)
    dx1 = input_gradient(m, lo.shiftCompensatedL1Loss, x, hr, mask, micro_batch=1)
    assert float((dx1 - dx).abs().max()) <= 1e-5 * float(dx.abs().max())


def test_frame_attribution_tool_writes_the_csv(dev, tmp_path):
    from tests.test_gpu_cli import CFG
    d = str(tmp_path)
    aug = os.path.join(d, "pre", "augmentedPatchesDir")
    os.makedirs(aug)
    x, hr, mask = synth.synth_batch(2, seed=5)
    np.ma.masked_array(x, mask=np.zeros(x.shape, bool)).dump(os.path.join(aug, "TRAINVALpatchesLR_NIR.npy"))
    np.ma.masked_array(hr, mask=~mask.astype(bool)).dump(os.path.join(aug, "TRAINVALpatchesHR_NIR.npy"))      # mask: True = obscured
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d))
    spec = importlib.util.spec_from_file_location("frame_attribution_tool", os.path.join(ROOT, "tools", "frame_attribution.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = os.path.join(d, "shares.csv")
    tool.main(["--cfg", cfg, "--band", "NIR", "--split", "val", "--max-patches", "8", "--out", out])
    rows = [ln.strip().split(",") for ln in open(out) if ln.strip()]
    assert len(rows) == 1 + 2 + 1 and all(len(r) == 9 + 1 for r in rows)
    assert rows[0][0] == "patch" and [r[0] for r in rows[1:]] == ["0", "1", "mean"]
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert np.abs(vals.sum(1) - 1).max() < 1e-6
    assert np.abs(vals[2] - vals[:2].mean(0)).max() < 1e-8
