"""The dynamic-LDS limit of every kernel that needs more than the default 64 KB is raised by launch_lds (csrc/probav_common.h) on the kernel's first such
launch on each device.  A warmed-up process cannot see an instance that the helper misses: some earlier launch may have raised the limit of the same
kernel.  So every case here is the FIRST library call of a fresh child process, and its results must equal, bit for bit, those of the same call made in
this (warmed-up) process.  The children run one after another.

  * a training step (forward + shift-L1 loss + backward, batch 2) of the shipped network (patch 16, T = 9) on every kernel family;
  * the same at T = 13 on family 4: the column-half instances of the backward-filter kernel, which live in two other translation units;
  * the sobel_l1_mix loss at its largest crop (its backward holds 161 616 bytes of dynamic LDS beside its static slots);
  * with two devices: the family-4 step on device 0 and then on device 1 of ONE process (the limit is an attribute per device).

The refused-raise path (PROBAV_EHIP for that call, nothing sticky) is not provoked on a device; it is reviewed by reading."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_BORDER = 3


def _step(impl, T, device):
    """pred, loss, gradient of one training step of the shipped network at batch 2: numpy arrays."""
    from probav_amd import synth
    from probav_amd.loss import Losses
    from probav_amd.modelsTF import WDSRConv3D
    with torch.cuda.device(device):
        m = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, T, 16, True, seed=0)
        m.load_variables(synth.synth_params(seed=900 + T, perturb=True, numImgLR=T))
        m = m.to(device)
        m.set_impl(impl)
        x, hr, mask = (torch.as_tensor(a).to(device) for a in synth.synth_batch(2, seed=901 + T, numImgLR=T))
        pred = m(x, training=True)
        loss = Losses(targetShape=(48, 48, 1)).shiftCompensatedL1Loss(hr, mask, pred)
        loss.backward()
        torch.cuda.synchronize()
        return dict(pred=pred.detach().cpu().numpy(), loss=loss.detach().cpu().numpy(), grad=m.flat.grad.detach().cpu().numpy())


def _edge(device):
    """sobel_l1_mix at the largest crop the library accepts: value and gradient."""
    from probav_amd.loss import L1EDGE_MAX_CROP, Losses
    S = L1EDGE_MAX_CROP + 2 * EDGE_BORDER
    rng = np.random.default_rng(77)
    hr = torch.as_tensor(rng.uniform(0.0, 0.4, (2, S, S, 1)).astype(np.float32)).to(device)
    mask = torch.as_tensor(rng.uniform(size=(2, S, S, 1)) > 0.1).to(device)
    pred = torch.as_tensor(rng.uniform(0.0, 0.4, (2, S, S, 1)).astype(np.float32)).to(device).requires_grad_(True)
    v = Losses(targetShape=(S, S, 1), cropBorder=EDGE_BORDER).shiftCompensatedL1EdgeLoss(hr, mask, pred)
    v.backward()
    torch.cuda.synchronize()
    return dict(loss=v.detach().cpu().numpy(), grad=pred.grad.cpu().numpy())


def _call(what, args):
    dev0 = torch.device("cuda:0")
    if what == "step":
        return _step(int(args[0]), int(args[1]), dev0)
    if what == "edge":
        return _edge(dev0)
    if what == "two":
        a, b = _step(4, 9, dev0), _step(4, 9, torch.device("cuda:1"))
        return dict([(k + "0", v) for k, v in a.items()] + [(k + "1", v) for k, v in b.items()])
    raise ValueError(what)


def _child(what, *args):
    """The call as the first library call of a fresh process -> its arrays."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.npz")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out, what] + [str(a) for a in args]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


_warm = {}


def _warmed(what, *args):
    """The same call in this process, after it has run here once already."""
    key = (what,) + args
    if key not in _warm:
        _call(what, args)
        _warm[key] = _call(what, args)
    return _warm[key]


def _same_bits(cold, warm):
    assert set(cold) == set(warm)
    for k in warm:
        assert np.isfinite(cold[k]).all(), k
        assert cold[k].dtype == warm[k].dtype and cold[k].shape == warm[k].shape, k
        assert np.array_equal(cold[k], warm[k]), "%s of a process's first call differs from the warmed-up process's" % k


@pytest.mark.parametrize("impl,T", [(0, 9), (1, 9), (2, 9), (3, 9), (4, 9), (4, 13)], ids=lambda v: str(v))
def test_first_call_of_a_process_is_a_training_step(dev, impl, T):
    _same_bits(_child("step", impl, T), _warmed("step", impl, T))


def test_first_call_of_a_process_is_the_edge_loss_at_its_largest_crop(dev):
    _same_bits(_child("edge"), _warmed("edge"))


def test_one_process_steps_on_two_devices(dev):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    r = _child("two")
    for k in ("pred", "loss", "grad"):
        assert np.isfinite(r[k + "0"]).all() and np.array_equal(r[k + "0"], r[k + "1"]), "%s differs between device 0 and device 1" % k
    _same_bits({k: r[k + "0"] for k in ("pred", "loss", "grad")}, _warmed("step", 4, 9))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **_call(sys.argv[2], sys.argv[3:]))
