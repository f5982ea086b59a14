"""The argument contract of the torch custom ops ('Custom ops: what an op accepts') on the device, from the table of
tests/ops_contract.py:

  accepted rows   each op on its well-formed operands and on the row's view of them (a slice of a larger allocation, dense with exchanged
                  strides, zero stride, a contiguous view off a 16-byte boundary, a bool mask, an empty batch): the outputs are bit for bit those
                  of a fresh contiguous clone, the inputs are bitwise what they were, the outputs have contiguous strides;
  autograd paths  an upstream gradient that arrives expanded (the gradient of .sum()) or strided gives the parameter and input gradients of the
                  same graph fed a contiguous gradient, bit for bit;
  refusal rows    through torch.ops (the dispatcher path).  The host check of the row runs first; the device call is made only if that refused
                  the row before any entry point, and afterwards the operands the op writes are bitwise what they were;
  late stream     each op's well-formed row, and one whole training step through autograd, while the current stream is a stream still busy
                  with a delay (tests/late_stream.py): the bits of the default stream, and the call back on the host before the delay has passed.

Shapes: the engine at T = 9, B = 2 (22 x 22 x 9 x 1 in, 48 x 48 out) in its default family, the rest as tests/ops_contract.py states them."""
import numpy as np
import pytest
import torch

from probav_amd import synth
from tests import ops_contract as oc

pytestmark = pytest.mark.gpu


class RealEngine:
    """What tests/ops_contract.StubEngine describes, from a live engine: the reference's network at T = 9."""

    def __init__(self, dev):
        from probav_amd import ops
        from probav_amd.modelsTF import WDSRConv3D
        m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
        m.load_variables(synth.synth_params(seed=61, perturb=True, numImgLR=9))
        self.model, self.dev = m.to(dev), dev
        self.handle, self.out = int(self.model._handle().value), 48
        self.nparams, self.weff, self.cout, self.in_shape, self.wc_floats = ops.engine_sizes(self.handle)
        self._flat = self.model.flat.detach().clone()
        self._x = torch.as_tensor(synth.synth_batch(2, seed=62)[0]).to(dev)
        self._kept = {}

    def _keep(self, key, make):
        if key not in self._kept:
            self._kept[key] = make()
        return self._kept[key]

    def flat(self):
        return self._flat.clone()

    def x(self, B):
        return self._x[:B].clone()

    def _built_cache(self):
        wc = torch.zeros(self.wc_floats, dtype=torch.float32, device=self.dev)      # (the cache has alignment gaps no kernel writes)
        torch.ops.probav.weight_cache_build(self._flat, wc, self.handle)
        return wc

    def wcache(self):
        return self._keep("wcache", self._built_cache).clone()

    def ws(self, B, wcache=False):
        return self._keep(("ws", B, wcache), lambda: torch.ops.probav.wdsr_forward(self._flat, self._x[:B], self.handle, self.out, True,
                                                                                   self.wcache() if wcache else None)[1])

    def inv_norm(self):
        return self._keep("inv", lambda: torch.ops.probav.wn_weight_fwd(self._flat, self.handle)[2]).clone()


@pytest.fixture(scope="module")
def env(dev):
    yield oc.Env("cuda", RealEngine(dev))
    from tests import late_stream
    print("\n" + late_stream.summary())


def _bytes(t):
    t = t.detach()
    return torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t).reshape(-1).view(torch.uint8)        # (fresh, standard strides)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b))


def _call(case, args):
    """-> the tensors a run leaves: the outputs the case compares, or the operands it wrote."""
    out = getattr(torch.ops.probav, case.op)(*oc.values(args))
    if case.outs is None:
        d = dict(args)
        return [d[n] for n in case.mutated if d.get(n) is not None]
    out = [out] if isinstance(out, torch.Tensor) else list(out)
    for t in out:
        assert t.is_contiguous(), (case.id, tuple(t.shape), t.stride())
    return out if case.compare is None else [out[i] for i in case.compare]


def _fresh(args):
    """A freshly allocated contiguous clone of every tensor operand."""
    return [(n, v.contiguous().clone() if isinstance(v, torch.Tensor) else v) for n, v in args]


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_accepted_rows_give_the_bits_of_a_contiguous_clone(env, case):
    failures = []
    base = _call(case, case.args(env))
    again = _call(case, case.args(env))
    assert all(_same(a, b) for a, b in zip(base, again)), "%s: two runs of the well-formed call differ" % case.id
    for row in [r for r in oc.accepted_rows() if r.case is case]:
        args = row.apply(env, case.args(env))
        read = [(n, v, v.clone()) for n, v in args if isinstance(v, torch.Tensor) and n not in case.mutated]
        want = _call(case, _fresh(args))
        got = _call(case, args)
        torch.cuda.synchronize()
        if len(got) != len(want) or not all(_same(g, w) for g, w in zip(got, want)):
            failures.append("%s: not the bits of the contiguous clone" % row.id)
        if row.kind in ("strided", "permuted", "offset") and not all(_same(g, b) for g, b in zip(got, base)):
            failures.append("%s: not the bits of the well-formed call" % row.id)
        for n, v, before in read:
            if not _same(v, before):
                failures.append("%s: the op changed its input %s" % (row.id, n))
        if row.outs is not None and case.outs is not None:
            for t, (shape, dtype) in zip(got, row.outs):
                if tuple(t.shape) != tuple(shape):
                    failures.append("%s: output %s, stated %s" % (row.id, tuple(t.shape), shape))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_refusal_rows_through_the_dispatcher_change_nothing(env, case):
    failures = []
    for row in [r for r in oc.refusal_rows() if r.case is case]:
        exc, calls, _ = oc.host_check(row)
        if not isinstance(exc, row.exc) or calls:
            failures.append("%s: the host check did not refuse it before the library (%r, %s): no device call made" % (row.id, exc, calls))
            continue
        args = row.apply(env, case.args(env))
        written = [(n, v, v.clone()) for n, v in args if isinstance(v, torch.Tensor) and n in case.mutated]
        try:
            getattr(torch.ops.probav, case.op)(*oc.values(args))
            failures.append("%s: accepted on the device" % row.id)
        except row.exc:
            pass
        except Exception as e:                             # noqa: BLE001
            failures.append("%s: %r instead of %s" % (row.id, e, row.exc.__name__))
        torch.cuda.synchronize()
        for n, v, before in written:
            if not _same(v, before):
                failures.append("%s: the refused call changed %s" % (row.id, n))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# autograd paths: the upstream gradient arrives expanded or strided
# ---------------------------------------------------------------------------------------------------------------------------------
def _swap_long(t):
    i, j = [d for d, n in enumerate(t.shape) if n > 1][:2]
    return t.transpose(i, j)


def _grads_under(forward, leaves, seed=7):
    """forward() -> the differentiable output y.  -> {how: [leaf gradients]} for the gradient of .sum() (expanded), a strided gradient, and the
    same two values handed over as freshly allocated contiguous tensors."""
    out = {}

    def run(how, drive):
        for p in leaves:
            p.grad = None
        drive(forward())
        out[how] = [p.grad.clone() for p in leaves]

    y = forward()
    r = torch.as_tensor(np.random.default_rng(seed).normal(size=tuple(y.shape)).astype(np.float32)).to(y.device)
    run("expanded", lambda y: y.sum().backward())
    run("expanded-contiguous", lambda y: y.backward(gradient=torch.ones_like(y)))
    if sum(n > 1 for n in y.shape) >= 2:
        rt = _swap_long(r).contiguous()                    # the factor of the transposed output: d / dy arrives as its transposed view
        run("strided", lambda y: (_swap_long(y) * rt).sum().backward())
        run("strided-contiguous", lambda y: y.backward(gradient=_swap_long(rt).contiguous()))
    else:
        big = torch.zeros(tuple(y.shape[:-1]) + (2 * y.shape[-1],), device=y.device)
        big[..., ::2] = r
        run("strided", lambda y: y.backward(gradient=big[..., ::2]))
        run("strided-contiguous", lambda y: y.backward(gradient=r.clone()))
    return out


def _assert_same_grads(out, names):
    for how in ("expanded", "strided"):
        for n, a, b in zip(names, out[how], out[how + "-contiguous"]):
            assert _same(a, b), "%s gradient: d/d%s differs from the same graph fed a contiguous gradient" % (how, n)
            assert a.is_contiguous()


def _leaves(args, names):
    d = dict(args)
    for n in names:
        d[n] = d[n].clone().requires_grad_(True)
    return d, [d[n] for n in names]


def test_network_op_gradients_under_expanded_and_strided_upstream(env):
    g = env.engine
    flat, x = g.flat().requires_grad_(True), g.x(2).requires_grad_(True)
    out = _grads_under(lambda: torch.ops.probav.wdsr_forward(flat, x, g.handle, g.out, True)[0], [flat, x])
    _assert_same_grads(out, ["flat", "x"])


@pytest.mark.parametrize("cid", ["shift_loss", "shift_l1edge_loss", "revssim_loss"])
def test_loss_op_gradients_under_expanded_and_offset_upstream(env, cid):
    """A scalar loss: the gradient of .expand(3).sum() and a 0-dim view one element into a larger tensor, against the same values as fresh
    tensors; and the prediction itself as a strided view."""
    case = oc.CASE[cid]
    d, (pred,) = _leaves(case.args(env), ["pred"])
    fwd = lambda: getattr(torch.ops.probav, case.op)(*[d[n] for n, _ in case.args(env)])[0]

    def grad(drive):
        pred.grad = None
        drive(fwd())
        return pred.grad.clone()

    buf = torch.full((4,), 1.3, device=pred.device)
    assert _same(grad(lambda l: l.expand(3).sum().backward()), grad(lambda l: l.backward(gradient=torch.tensor(3.0, device=pred.device))))
    assert _same(grad(lambda l: l.backward(gradient=buf[1])), grad(lambda l: l.backward(gradient=torch.tensor(1.3, device=pred.device))))
    want = grad(lambda l: l.backward())
    view = oc.strided(env, pred.detach()).requires_grad_(True)
    d["pred"] = view
    fwd().backward()
    assert _same(view.grad, want)


def test_conv_op_gradients_under_expanded_and_strided_upstream(env):
    case = oc.CASE["conv3d_k3_fwd"]
    d, leaves = _leaves(case.args(env), ["x", "w", "bias"])
    out = _grads_under(lambda: torch.ops.probav.conv3d_k3_fwd(*[d[n] for n, _ in case.args(env)]), leaves)
    _assert_same_grads(out, ["x", "w", "bias"])


def test_pointwise_pair_gradients_under_expanded_and_strided_upstream(env):
    case = oc.CASE["pw_expand_relu_decay_fwd"]
    names = ["x", "w1", "b1", "w2", "b2"]
    d, leaves = _leaves(case.args(env), names)
    out = _grads_under(lambda: torch.ops.probav.pw_expand_relu_decay_fwd(*[d[n] for n, _ in case.args(env)]), leaves)
    _assert_same_grads(out, names)


def test_weight_norm_gradients_under_expanded_and_strided_upstream(env):
    g = env.engine
    flat = g.flat().requires_grad_(True)
    out = _grads_under(lambda: torch.ops.probav.wn_weight_fwd(flat, g.handle)[0], [flat])
    _assert_same_grads(out, ["flat"])


# ---------------------------------------------------------------------------------------------------------------------------------
# late stream: every op, and one whole step through autograd, while the current stream is not the default one (tests/late_stream.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _held_back(args):
    """The operands of a row that arrive late: its floating tensors hold zeros until their values are copied in behind the delay (zeros are ordinary data for every
    op); integer and boolean operands hold their values from the start, so indices stay valid.  An op without a floating operand (scoring, the baseline, the window
    counts) would prove nothing that way: there the uint16 images and uint8 masks -- pixel data, never an index -- arrive late instead."""
    tensors = [(n, v) for n, v in args if isinstance(v, torch.Tensor)]
    held = [n for n, v in tensors if v.is_floating_point()]
    return held or [n for n, v in tensors if v.dtype in (torch.uint16, torch.uint8)]


def _single_operator_entries():
    """The entry points whose every call the header lets wait on the host: the one table, tests/test_gpu_bands.py."""
    from tests import test_gpu_bands as tb
    return {n for n, (sentence, _) in tb.HOST_WAIT_EXEMPT.items() if sentence is tb._SINGLE_OP}


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_accepted_row_on_a_late_stream(env, case):
    """The well-formed row of the case while the current stream is a stream that is still busy: the op must hand THAT stream to the library, and every launch behind it must
    be on it -- the outputs are the default stream's bit for bit although the operands' values arrive only behind the delay -- and, after one warm-up call on the stream
    (allocator pools, first-call uploads, table growth), the op must come back before the delay has passed."""
    from tests import late_stream
    dev = env.device
    real = case.args(env)
    held = _held_back(real)
    snapshot = lambda ts: [t.detach().clone() for t in ts]
    zeroed = lambda: [(n, (torch.zeros_like(v) if n in held else v.clone()) if isinstance(v, torch.Tensor) else v) for n, v in real]
    want = snapshot(_call(case, _fresh(real)))
    proof = snapshot(_call(case, zeroed()))
    torch.cuda.synchronize()
    assert held and not all(_same(p, w) for p, w in zip(proof, want)), "%s: the row proves nothing, zeroed operands %s give the real outputs" % (case.id, held)
    s = late_stream.stream(dev)
    with torch.cuda.stream(s):
        _call(case, _fresh(real))
    s.synchronize()
    values = {n: v.clone() for n, v in real if n in held}
    for factor in (1, late_stream.RETRY_FACTOR):
        args = zeroed()
        torch.cuda.synchronize()
        gate = late_stream.begin(dev, factor, case.id)
        with torch.cuda.stream(s):
            for n, v in args:
                if n in held:
                    v.copy_(values[n])
            got = _call(case, args)
            early = gate.returned()
            same = len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))        # (read through the stream: torch.equal waits for it alone)
        s.synchronize()
        if early:
            break
        late_stream.stats["retries"] += factor == 1
    if not early and set(case.entries) & _single_operator_entries():
        late_stream.note_wait("op " + case.id)
    assert same, "%s: on a late stream the outputs are not those of the default stream" % case.id
    assert early or set(case.entries) & _single_operator_entries(), "%s: the op came back only after a delay of %d x %.1f ms had passed on its stream" % (
        case.id, factor, late_stream.delay_ms(dev))


@pytest.mark.parametrize("impl", [0, 4])
def test_training_step_on_a_late_stream(dev, impl):
    """tests/late_step.py with the engine's default side-stream mode (2): the fork to the side stream is from the late stream and the join is back into it."""
    from tests import late_step
    failures, early = late_step.run(impl)
    assert not failures, "family %d: on a late stream %s differ from the default stream's" % (impl, failures)
    assert early, "family %d: the step came back only after the delay on its stream had passed" % impl


@pytest.mark.parametrize("impl", [0, 4])
def test_training_step_on_a_late_stream_without_the_side_stream(dev, impl):
    """The same with PROBAV_NO_SIDE_STREAM=1, which the library reads once per process: a child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PROBAV_NO_SIDE_STREAM="1")
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests import late_step; late_step.main()" % root, str(impl)],
                         env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    assert "LATE_STEP failures=none early=True" in out.stdout, out.stdout[-2000:]
