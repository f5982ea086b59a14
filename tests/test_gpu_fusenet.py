"""FuseNet on the device (csrc/kernels_fusenet.hip) against the fp64 statement (probav_amd/fusenet_numpy.py).

The accuracy bar for y and dK: e_dev <= 4 e_cpu32, where e_cpu32 is the max-norm error of torch's CPU float32 evaluation of the same composition
against the statement and e_dev the device's, each backward judged at the gates of its own leg.  The factor 4 allows for two legitimate fp32
summation orders over 2304 (y) or B H W (dK) products; it is a judgement, not a measurement.  Every check is made on the branch m (residual=False):
out - x carries half an ulp of x, about 1 % of m.  Measured figures: profiles/fusenet_accuracy.txt."""
import numpy as np
import pytest
import torch

from probav_amd import fusenet_numpy as fn
from tests import fusenet_helpers as fh

pytestmark = pytest.mark.gpu


def _run(dev, x, P, g=None, residual=False):
    flat = torch.tensor(fh.flat_of(*P), device=dev)
    xd = torch.tensor(np.asarray(x, dtype=np.float32), device=dev)
    out, y, stats = torch.ops.probav.fusenet_forward(xd, flat, residual)
    res = dict(out=out, y=y, stats=stats, flat=flat, x=xd)
    if g is not None:
        res["dflat"] = torch.ops.probav.fusenet_backward(torch.tensor(g, device=dev), xd, y, stats, flat)
    return res


def _check_against_statement(dev, c, label):
    P, x, g, f = c["P"], c["x"], c["g"], c["fwd"]
    r = _run(dev, x, P, g)
    y = r["y"].cpu().double().numpy().transpose(0, 3, 1, 2)
    stats = r["stats"].cpu().double().numpy()
    bias = P[1].reshape(1, -1, 1, 1)
    e_y = fh.abserr(y, f["y"] - bias)
    gates = fh.device_gates(r["y"].cpu().numpy(), r["stats"].cpu().numpy(), P[2], P[3])
    b = fn.backward(g, x, *P, gates=gates, fwd=f)
    dK, dbias, dgamma, dbeta = fn.split_flat(r["dflat"].cpu().double().numpy())
    e_dK = fh.abserr(dK, b["dK"])
    print("fusenet accuracy %s: y e_dev %.3e e_cpu32 %.3e ratio %.2f | dK e_dev %.3e e_cpu32 %.3e ratio %.2f"
          % (label, e_y, c["e_cpu32_y"], e_y / c["e_cpu32_y"], e_dK, c["e_cpu32_dK"], e_dK / c["e_cpu32_dK"]))
    assert e_y <= 4 * c["e_cpu32_y"]
    assert e_dK <= 4 * c["e_cpu32_dK"]
    assert fh.maxerr(r["out"].cpu().numpy(), f["m"]) < 1e-3
    assert fh.maxerr(dgamma, b["dgamma"]) < 1e-3 and fh.maxerr(dbeta, b["dbeta"]) < 1e-3
    assert not dbias.any()
    mu = f["mu"] - P[1][None]
    assert np.abs(stats[:, :, 0] - mu).max() <= 1e-5 * np.abs(mu).max()
    assert np.abs(stats[:, :, 1] / f["rstd"] - 1).max() <= 1e-5


@pytest.mark.parametrize("shape", fh.SHAPES, ids=str)
def test_forward_and_backward_against_the_statement(dev, shape):
    _check_against_statement(dev, fh.case(shape), str(shape))


def test_shipped_size_through_the_fft_statement(dev):
    _check_against_statement(dev, fh.case((1, 384, 384)), "(1, 384, 384)")


def test_zero_image_takes_the_eps_path_exactly(dev):
    """A constant-zero image: y = 0, var = 0, xhat = 0, so m = mean_c leaky(beta_c)."""
    P = fh.params()
    r = _run(dev, np.zeros((1, 20, 33), np.float32), P)
    beta = P[3].astype(np.float32)
    want = np.float64(np.where(beta >= 0, beta, np.float32(0.3) * beta)).mean()
    m = r["out"].cpu().double().numpy()
    assert not r["y"].cpu().numpy().any()
    assert np.ptp(m) == 0.0 and abs(m[0, 0, 0] - want) <= 2e-8          # 64 float32 terms of at most 0.05, summed and divided by 64
    st = r["stats"].cpu().numpy()
    assert not st[:, :, 0].any() and np.all(st[:, :, 1] == np.float32(1.0 / np.sqrt(1e-3)))


def test_constant_image_and_a_zero_filter(dev):
    """A constant non-zero image (interior y constant, the zero padding shapes the rim) and a filter whose channel 5 is all zero (y = 0, var = 0 there)."""
    K, bias, gamma, beta = fh.params()
    K = K.copy()
    K[..., 5] = 0.0
    P = (K, bias, gamma, beta)
    x = np.full((1, 50, 70), 9000.0, np.float32)
    f = fn.forward(x, *P)
    r = _run(dev, x, P)
    assert fh.maxerr(r["out"].cpu().numpy(), f["m"]) < 1e-3
    y = r["y"].cpu().numpy()
    assert not y[..., 5].any()
    st = r["stats"].cpu().numpy()
    assert st[0, 5, 0] == 0.0 and st[0, 5, 1] == np.float32(1.0 / np.sqrt(1e-3))


def test_samples_that_differ_in_scale_by_2_to_10(dev):
    P = fh.params()
    x = fh.image((2, 40, 56))
    x[1] = np.rint(x[1] / 1024.0)                        # 0..16: 2^10 below its batch mate
    f = fn.forward(x, *P)
    c32 = fh.torch_compose(x, *P, dtype=torch.float32)
    r = _run(dev, x, P)
    for b in range(2):
        assert fh.maxerr(r["out"][b].cpu().numpy(), f["m"][b]) < 1e-3, b
        yb = r["y"][b].cpu().double().numpy().transpose(2, 0, 1)
        ref = f["y"][b] - P[1].reshape(-1, 1, 1)
        e_dev, e_cpu = fh.abserr(yb, ref), fh.abserr(c32["y"][b], f["y"][b])
        print("fusenet scale 2^10, sample %d: y e_dev %.3e e_cpu32 %.3e" % (b, e_dev, e_cpu))
        assert e_dev <= 4 * e_cpu, b                     # each sample to ITS OWN fp32 error: no scale shared across the batch


def test_exact_properties(dev):
    shape = (3, 40, 96)
    c = fh.case(shape)
    P, x, g = c["P"], c["x"], c["g"]
    r = _run(dev, x, P, g)
    rr = _run(dev, x, P, g, residual=True)
    # residual=True is fl32(x + m) of the residual=False call
    assert torch.equal(rr["out"], r["x"] + r["out"])
    assert torch.equal(rr["y"], r["y"]) and torch.equal(rr["stats"], r["stats"])
    # two calls, the same bits
    r2 = _run(dev, x, P, g)
    for key in ("out", "y", "stats", "dflat"):
        assert torch.equal(r[key].view(torch.int32), r2[key].view(torch.int32)), key
    # a sample alone and as any member of a batch
    for b in range(3):
        one = _run(dev, x[b:b + 1], P)
        assert torch.equal(one["out"][0].view(torch.int32), r["out"][b].view(torch.int32))
        assert torch.equal(one["y"][0].view(torch.int32), r["y"][b].view(torch.int32))
        assert torch.equal(one["stats"][0].view(torch.int32), r["stats"][b].view(torch.int32))
    # dbias: exact zeros
    assert not r["dflat"][147456:147456 + 64].any()
    # autograd gives the functional op's bits
    flat = r["flat"].clone().requires_grad_(True)
    out, _, _ = torch.ops.probav.fusenet_forward(r["x"], flat, True)
    gd = torch.tensor(g, device=dev)
    (out * gd).sum().backward()
    assert torch.equal(flat.grad.view(torch.int32), r["dflat"].view(torch.int32))


def test_opcheck(dev):
    P = fh.params()
    flat = torch.tensor(fh.flat_of(*P), device=dev, requires_grad=True)
    x = torch.tensor(fh.image((1, 9, 11)), device=dev)
    torch.library.opcheck(torch.ops.probav.fusenet_forward, (x, flat, True), test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    out, y, stats = torch.ops.probav.fusenet_forward(x, flat.detach(), True)
    torch.library.opcheck(torch.ops.probav.fusenet_backward, (torch.ones_like(x), x, y, stats, flat.detach()), test_utils=("test_schema", "test_faketensor"))


def test_bad_arguments_are_refused_and_nothing_is_launched(dev):
    from probav_amd import _lib
    L = _lib.lib()
    flat = torch.zeros(147648, device=dev)
    x = torch.zeros(1, 8, 8, device=dev)
    out, y, stats = torch.full((1, 8, 8), 7.0, device=dev), torch.full((1, 8, 8, 64), 7.0, device=dev), torch.full((1, 64, 2), 7.0, device=dev)
    dflat = torch.full((147648,), 7.0, device=dev)
    nf, nb = L.probav_fusenet_workspace_bytes(1, 8, 8, 0), L.probav_fusenet_workspace_bytes(1, 8, 8, 1)
    assert nf > 0 and nb > nf
    assert L.probav_fusenet_workspace_bytes(1, 0, 8, 0) == 0 and L.probav_fusenet_workspace_bytes(1, 8, 0, 1) == 0
    ws = torch.zeros(nb // 8 + 1, dtype=torch.float64, device=dev)
    s = _lib.current_stream()
    p = _lib.ptr

    def fwd(H=8, W=8, count=147648, wsb=nb):
        return L.probav_fusenet_forward(p(x), p(flat), count, 1, H, W, 1, p(out), p(y), p(stats), p(ws), wsb, s)

    def bwd(H=8, W=8, count=147648, wsb=nb):
        return L.probav_fusenet_backward(p(x), p(x), p(y), p(stats), p(flat), count, 1, H, W, p(dflat), p(ws), wsb, s)

    for call in (fwd, bwd):
        assert call(H=0) == _lib.PROBAV_EINVAL and call(W=0) == _lib.PROBAV_EINVAL and call(H=-3) == _lib.PROBAV_EINVAL
        assert call(count=147647) == _lib.PROBAV_EINVAL
    assert fwd(wsb=nf - 1) == _lib.PROBAV_EINVAL and bwd(wsb=nb - 1) == _lib.PROBAV_EINVAL
    assert L.probav_fusenet_forward(None, p(flat), 147648, 1, 8, 8, 1, p(out), p(y), p(stats), p(ws), nb, s) == _lib.PROBAV_EINVAL
    torch.cuda.synchronize()
    for t in (out, y, stats, dflat):
        assert bool((t == 7.0).all())
    assert fwd() == _lib.PROBAV_OK and bwd() == _lib.PROBAV_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        torch.ops.probav.fusenet_forward(x, flat[:-1], True)


def test_input_that_requires_grad_is_refused(dev):
    from probav_amd.modelsTF import FuseNetConv2D
    m = FuseNetConv2D("fuse", "NIR").build(seed=0).to(dev)
    x = torch.zeros(1, 8, 8, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="no gradient for its input"):
        m(x, training=True)
    out, _, _ = torch.ops.probav.fusenet_forward(x, m.flat, True)
    with pytest.raises(RuntimeError, match="no gradient for its input"):
        out.sum().backward()


def _planted_seam(B, S, seed=4):
    """Input = target + a ramp at every 48th column (the seam of side-by-side patches); clear mask."""
    hr = fh.image((B, S, S), seed).astype(np.float32)
    x = hr.copy()
    for c0 in range(47, S, 48):
        x[:, :, c0] += 400.0
        if c0 + 1 < S:
            x[:, :, c0 + 1] -= 400.0
    return x, hr[..., None], np.ones((B, S, S, 1), np.uint8)


def _trainer(dev, tmp, seed=0):
    from probav_amd.loss import Losses
    from probav_amd.modelsTF import FuseNetConv2D
    from probav_amd.trainClass import ModelTrainer, make_optimizer
    model = FuseNetConv2D("fuse", "NIR").build(seed=seed).to(dev)
    losses = Losses(targetShape=(96, 96, 1))
    return ModelTrainer(model, losses.shiftCompensatedL1Loss, losses.shiftCompensatedcPSNR, make_optimizer("nadam", model, 1e-5), str(tmp / "ckpt"),
                        str(tmp / "log"), multiGPU=False)


def test_trainer_steps_lower_the_loss_checkpoint_and_resume(dev, tmp_path):
    x, hr, mk = _planted_seam(4, 96)
    xd, hd, md = (torch.tensor(a, device=dev) for a in (x[..., None], hr, mk))
    tr = _trainer(dev, tmp_path / "a")
    with torch.no_grad():
        before = float(tr.loss(hd, md, tr.model(xd)))
    tr.trainStep(xd, hd, md)
    tr.step += 1
    tr.save()
    saved = tr.model.flat.detach().clone()
    tr.trainStep(xd, hd, md)
    with torch.no_grad():
        after = float(tr.loss(hd, md, tr.model(xd)))
    print("fusenet planted seam: loss %.6f -> %.6f after two steps" % (before, after))
    assert after < before
    # a second trainer on the same directory restores the checkpoint bit for bit and continues to the same bits
    tr2 = _trainer(dev, tmp_path / "a", seed=9)
    assert tr2.step == 1 and torch.equal(tr2.model.flat.detach().view(torch.int32), saved.view(torch.int32))
    tr2.trainStep(xd, hd, md)
    assert torch.equal(tr2.model.flat.detach().view(torch.int32), tr.model.flat.detach().view(torch.int32))


def test_fuse_flag_end_to_end(dev, tmp_path):
    """test.py --fuse writes round-half-even(clip(FuseNet(plain PNG))) computed through the op, evaluate.py --model --fuse scores those images, and
    without the flag the plain PNGs are what they were."""
    import glob
    import json
    import os
    from probav_amd import testClass
    from probav_amd.modelsTF import FuseNetConv2D
    from probav_amd.pngio import imread_uint16
    from probav_amd.trainClass import ModelTrainer
    from tests import test_gpu_tiles as tt
    d = str(tmp_path)
    res, trm = os.path.join(d, "pre", "resolverDir"), os.path.join(d, "pre", "trimmedArrayDir")
    os.makedirs(res), os.makedirs(trm)
    frames = tt.cloudy_frames()
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(tt.CFG.format(d=d))
    for key in ("TEST", "TRAIN"):
        np.ma.masked_array(tt._frames_parts(frames, 16).transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((3, 64, 9, 1, 22, 22), bool)).dump(
            os.path.join(res, "%spatchesLR_NIR.npy" % key), protocol=4)
    rng = np.random.default_rng(4)
    hr = rng.integers(0, 2 ** 14, (4, 1, 1, 384, 384)).astype(np.float64)              # ids 594 .. 597; 595 is removed
    np.ma.masked_array(hr, mask=rng.random(hr.shape) < 0.1).dump(os.path.join(res, "TRAINimgHR_NIR.npy"))
    with open(os.path.join(d, "removedTrainSetsNIR.txt"), "w") as fh:
        fh.write("1307\n1308.0\n595\n")
    model = tt._model(dev)
    ck = os.path.join(d, "modelInfo", "ckpt_mini", "NIR")
    assert ModelTrainer(model, None, None, None, ck, os.path.join(d, "modelInfo", "logs_mini", "NIR")).save() == "ckpt-1.pt"
    test_py, eval_py = os.path.join(tt.ROOT, "test.py"), os.path.join(tt.ROOT, "evaluate.py")
    names = ["imgset1306.png", "imgset1309.png", "imgset1310.png"]
    read = lambda: [imread_uint16(os.path.join(d, "testout_mini", n)) for n in names]

    # no FuseNet checkpoint yet: an error that names the directory looked in
    fck = os.path.join(d, "modelInfo", "fuseNetCkpt_mini", "NIR")
    out = tt.subprocess.run([tt.sys.executable, test_py, "--cfg", cfg, "--band", "NIR", "--fuse"], cwd=d, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and fck in out.stderr and "no FuseNet checkpoint" in out.stderr

    tt._run([test_py, "--cfg", cfg, "--band", "NIR"], cwd=d)
    plain = read()
    want_plain = testClass.evaluate_device(model, tt._frames_parts(frames, 16))
    for got, w in zip(plain, want_plain):
        np.testing.assert_array_equal(got, w[:, :, 0].astype(np.uint16))               # the plain path, untouched by the flag's existence

    fuse = FuseNetConv2D("fusionNet", "NIR").build(seed=3)
    with torch.no_grad():
        fuse.flat[147456 + 64:147456 + 128] *= 400.0        # gamma: a branch of a few DN, so that the fused PNGs differ from the plain ones
    fuse = fuse.to(dev)
    assert ModelTrainer(fuse, None, None, None, fck, os.path.join(d, "lg")).save() == "ckpt-1.pt"
    for f in glob.glob(os.path.join(d, "testout_mini", "*.png")):
        os.remove(f)
    tt._run([test_py, "--cfg", cfg, "--band", "NIR", "--fuse"], cwd=d)
    fused = read()
    x = torch.tensor(np.stack(plain).astype(np.float32), device=dev)
    out, _, _ = torch.ops.probav.fusenet_forward(x, fuse.flat.detach(), True)
    want = torch.ops.probav.clip_round(out, 0.0, 65535.0).cpu().numpy().astype(np.uint16)
    for got, w in zip(fused, want):
        np.testing.assert_array_equal(got, w)
    assert any(not np.array_equal(a, b) for a, b in zip(fused, plain))

    # evaluate.py --model --fuse scores the images test.py --totest TRAIN --fuse writes (the TRAIN patches here are the TEST patches)
    tt._run([test_py, "--cfg", cfg, "--band", "NIR", "--totest", "TRAIN", "--fuse"], cwd=d)
    last = lambda out: json.loads(out.stdout.strip().splitlines()[-1])
    line = last(tt._run([eval_py, "--cfg", cfg, "--band", "NIR", "--model", "--fuse", "--out", os.path.join(d, "scores")], cwd=d))
    folder = last(tt._run([eval_py, "--cfg", cfg, "--band", "NIR", "--toCompare", os.path.join(d, "trainout_mini"), "--out", os.path.join(d, "scores2")], cwd=d))
    plain_line = last(tt._run([eval_py, "--cfg", cfg, "--band", "NIR", "--model", "--out", os.path.join(d, "scores3")], cwd=d))
    assert (line["scored"], line["missing"], line["removed"]) == (3, 0, 3)
    assert line["NIR"] == folder["NIR"] and line["NIR"]["mean_cpsnr"] != plain_line["NIR"]["mean_cpsnr"]


def test_train_py_fusion_net_writes_a_checkpoint_that_fuse_reads(dev, tmp_path):
    """train.py --modelType fusionNet --fusion-input DIR on five stitched images: trains, saves under <model_out>/fuseNetCkpt_<cfg>/<band>, and a
    second run restores it."""
    import os
    from probav_amd.pngio import imsave_uint16
    from tests import test_gpu_cli as tc
    d = str(tmp_path)
    trm, png = os.path.join(d, "pre", "trimmedArrayDir"), os.path.join(d, "trainout_mini")
    os.makedirs(trm), os.makedirs(png)
    x, hr, mk = _planted_seam(5, 384)
    np.ma.masked_array(hr[:, None, None, :, :, 0].astype(np.float64), mask=np.zeros((5, 1, 1, 384, 384), bool)).dump(os.path.join(trm, "TRAINimgHR_NIR.npy"), protocol=4)
    for k in range(5):
        imsave_uint16(os.path.join(png, "imgset%04d.png" % (594 + k)), x[k].astype(np.uint16))
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(tc.CFG.format(d=d))
    args = [os.path.join(tc.ROOT, "train.py"), "--cfg", cfg, "--band", "NIR", "--modelType", "fusionNet", "--fusion-input", png]
    out = tc._run(args, cwd=d)
    ck = os.path.join(d, "modelInfo", "fuseNetCkpt_mini", "NIR")
    assert open(os.path.join(ck, "checkpoint.pt-index")).read().split() == ["ckpt-1.pt"], out.stderr[-2000:]
    assert "5 images (4 training, 1 validation)" in out.stderr and "[ EPOCH 0/1 ] - [ STEP 4/4 ]" in out.stderr
    state = torch.load(os.path.join(ck, "ckpt-1.pt"), map_location="cpu")
    assert state["step"] == 4 and sorted(state["model"]) == ["conv2d", "instance_normalization"]
    assert not state["model"]["conv2d"]["bias"].any()               # its gradient is exact zeros: the bias never moves
    from probav_amd.inference import load_fusenet
    from probav_amd.parseConfig import parseConfig
    m = load_fusenet(parseConfig(cfg), cfg, "NIR", "test")
    assert torch.equal(m.trainable_variables[0].detach().cpu(), state["model"]["conv2d"]["kernel"])
