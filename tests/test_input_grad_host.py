"""Input gradients (d loss / d LR frames from probav::wdsr_forward), the parts that need no GPU: the autograd formula traces on fake tensors and
picks the op with the second output only when the input requires grad; the two C entry points are bound; the new op declares no mutation; the
arithmetic of attribution.frame_shares; and the fp64 numpy statement of the kernel's formula (the reference of tests/test_gpu_input_grad.py)
agrees with autograd through torch's own convolutions."""
import ctypes

import numpy as np
import pytest
import torch


class _Stop(Exception):
    pass


def _trace(monkeypatch, x_requires_grad):
    """The joint graph of tests/test_ops_trace_cpu.py's step (fake tensors, AOT-autograd), with the model input a leaf that does or does not
    require grad."""
    pytest.importorskip("torch._dynamo")
    from functorch.compile import min_cut_rematerialization_partition
    from torch._functorch.aot_autograd import aot_module_simplified
    from probav_amd import ops
    # the sizes come from the engine (a device object): any constant does for the trace
    monkeypatch.setattr(ops, "_ws_floats", lambda engine, batch, training: 4096)
    monkeypatch.setattr(ops, "_input_shape", lambda engine, batch: (int(batch), 22, 22, 9, 1))
    seen = {}

    def fw_compiler(gm, example_inputs):
        def run(*args):
            raise _Stop()
        return run

    def partition(joint, inputs, **kw):
        seen["joint"] = joint.print_readable(print_output=False)
        return min_cut_rematerialization_partition(joint, inputs, **kw)

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=fw_compiler, bw_compiler=lambda g, e: g, partition_fn=partition)

    def step(flat, x, hr, mk):
        y, _ = torch.ops.probav.wdsr_forward(flat, x, 1234, 48, True)
        return torch.ops.probav.shift_loss(y, hr, mk, 3, 16, 1)[0]

    flat = torch.zeros(535267, requires_grad=True)
    x = torch.zeros(2, 22, 22, 9, 1, requires_grad=x_requires_grad)
    hr, mk = torch.zeros(2, 48, 48, 1), torch.ones(2, 48, 48, 1, dtype=torch.uint8)
    torch._dynamo.reset()
    with pytest.raises(_Stop):
        torch.compile(step, backend=backend, fullgraph=True)(flat, x, hr, mk)
    torch._dynamo.reset()
    return seen["joint"]


def test_joint_graph_holds_the_input_gradient_op_when_x_requires_grad(built_lib, monkeypatch):
    joint = _trace(monkeypatch, True)
    assert "probav.wdsr_backward_input" in joint and "probav.shift_loss_backward" in joint
    assert "copy_" not in joint


def test_joint_graph_keeps_the_plain_backward_when_x_does_not_require_grad(built_lib, monkeypatch):
    joint = _trace(monkeypatch, False)
    assert "probav.wdsr_backward" in joint and "probav.wdsr_backward_input" not in joint
    assert "copy_" not in joint


def test_entry_points_are_bound_and_the_op_declares_no_mutation(built_lib):
    from probav_amd import _lib
    import probav_amd.ops  # noqa: F401
    assert "probav_backward_input" in _lib.SIGNATURES and "probav_input_grad" in _lib.SIGNATURES
    L = _lib.lib()                                         # every signature resolves against the built library
    assert L.probav_abi_version() == 7
    split, inp = _lib.SIGNATURES["probav_backward_split"], _lib.SIGNATURES["probav_backward_input"]
    assert inp[0] is split[0] and len(inp[1]) == len(split[1]) + 1          # the arguments of probav_backward_split plus dx
    schema = str(torch.ops.probav.wdsr_backward_input.default._schema)
    assert "!" not in schema, schema
    assert schema.endswith("(Tensor flat, Tensor dy, Tensor ws, SymInt engine, Tensor? wcache=None) -> (Tensor, Tensor)"), schema


def test_input_grad_refuses_bad_arguments_without_a_device(built_lib):
    """The argument checks of the single-operator entry run before anything touches a device."""
    from probav_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p
    ok = [p(4096)] * 3 + [p(4096), None, p(4096)]
    assert L.probav_input_grad(1, 8, 3, 2, *ok, 1.0, p(4096), None) == _lib.PROBAV_EINVAL          # C = 2
    assert L.probav_input_grad(1, 2, 3, 1, *ok, 1.0, p(4096), None) == _lib.PROBAV_EINVAL          # H < 3: residConv1 has no output
    assert L.probav_input_grad(1, 8, 3, 1, *ok, 0.0, p(4096), None) == _lib.PROBAV_EINVAL          # std
    assert L.probav_input_grad(1, 8, 3, 1, p(4100), *ok[1:], 1.0, p(4096), None) == _lib.PROBAV_EINVAL      # g not 16-byte aligned
    assert L.probav_input_grad(1, 8, 3, 1, *ok, 1.0, None, None) == _lib.PROBAV_EINVAL             # no dx
    assert L.probav_input_grad(1, 8, 100, 1, *ok, 1.0, p(4096), None) == _lib.PROBAV_EINVAL        # no tile of 100 frames fits the LDS budget


def test_frame_shares_arithmetic():
    from probav_amd.attribution import frame_shares
    dx = torch.zeros(4, 2, 2, 3, 2)
    dx[0, :, :, 0, :] = -1.0                      # 8 of |.| on frame 0
    dx[0, 0, 0, 1, 0] = 2.0                       # 2 on frame 1
    dx[0, 1, 1, 2, 1] = -6.0                      # 6 on frame 2
    dx[1, 0, 0, 2, 0] = 1e-30                     # a tiny gradient is still a preference
    dx[3, 0, 0, 0, 0] = float("inf")
    s = frame_shares(dx)
    assert s.dtype == torch.float64 and tuple(s.shape) == (4, 3)
    assert s[0].tolist() == [0.5, 0.125, 0.375]
    assert s[1].tolist() == [0.0, 0.0, 1.0]
    # an all-zero sample (a fully masked target) has no preference: the uniform row, which still sums to 1
    assert s[2].tolist() == [1.0 / 3] * 3
    assert torch.isnan(s[3]).all()                # a non-finite gradient is reported, not averaged in
    assert torch.allclose(s[:3].sum(1), torch.ones(3, dtype=torch.float64), rtol=0, atol=1e-15)
    rng = np.random.default_rng(0)
    r = frame_shares(rng.normal(size=(5, 4, 4, 9, 3)).astype(np.float32))
    assert float((r.sum(1) - 1).abs().max()) < 1e-14 and float(r.min()) > 0
    with pytest.raises(ValueError):
        frame_shares(torch.zeros(2, 3))


@pytest.mark.parametrize("H,T,C,B", [(7, 1, 1, 1), (8, 3, 3, 2)])
def test_numpy_statement_of_the_formula_agrees_with_autograd(H, T, C, B):
    """dx of  sum(G * relu(conv3d_same(xn, wmain))) + sum(D1 * relu(conv2d_valid(mn, w1)))  with xn = (x - mean) / std, mn = mean_T(xn): autograd through
    torch's convolutions against tests/input_grad_helpers.input_grad_numpy at the gates of that evaluation."""
    from oracle import wdsr_torch as ot
    from tests.input_grad_helpers import input_grad_numpy
    rng = np.random.default_rng(H * 10 + T)
    x = torch.tensor(rng.normal(size=(B, H, H, T, C)) * 3 + 5, requires_grad=True)
    wmain, w1 = torch.tensor(rng.normal(size=(3, 3, 3, C, 32))), torch.tensor(rng.normal(size=(3, 3, 1, C, 9)))
    g, d1 = torch.tensor(rng.normal(size=(B, H, H, T, 32))), torch.tensor(rng.normal(size=(B, H - 2, H - 2, 9)))
    mean, std = 5.0, 3.0
    xn, mn = (x - mean) / std, (x.mean(dim=3) - mean) / std
    act0 = torch.relu(ot._conv(xn, wmain, None, True))
    r1 = torch.relu(ot._conv(mn, w1[:, :, 0], None, False))
    ((act0 * g).sum() + (r1 * d1).sum()).backward()
    dx, main, res = input_grad_numpy(g.numpy(), act0.detach().numpy(), wmain.numpy(), d1.numpy(), r1.detach().numpy(), w1.numpy(), std)
    assert np.abs(dx - x.grad.numpy()).max() < 1e-12 * np.abs(dx).max()
    assert np.abs(main).max() > 0 and np.abs(res).max() > 0
    # already-gated d1 and no gate tensor: the same residual share
    dg = np.where(r1.detach().numpy() > 0, d1.numpy(), 0.0)
    assert np.array_equal(input_grad_numpy(g.numpy(), act0.detach().numpy(), wmain.numpy(), dg, None, w1.numpy(), std)[2], res)
