"""The online augmentation on the device (csrc/kernels_augment.hip, probav_amd/augment.py): the kernel against its numpy statement bit for
bit over every code, shape and batch size; DeviceDataset over a whole virtual set against what the builder's functions materialise; the
trainer and train.py fed either way, step by step and weight by weight.  (The kernel's guard against recipes that point outside the
base arrays is a safety net and is deliberately not exercised here: recipes are validated on the host, tests/test_augment_host.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probav_amd.ops  # noqa: F401  (registers torch.ops.probav.augment_batch)
from probav_amd import augment, prep, synth
from probav_amd.augment import AugmentSpec, apply_recipe_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPES = [(22, 9, 1), (22, 13, 1), (22, 7, 1), (22, 19, 1), (22, 9, 3), (30, 9, 1), (38, 9, 1)]


def _bits(rng, shape):
    """float32 with arbitrary bit patterns (NaN payloads, denormals, infinities included): the kernel moves bits."""
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def _recipes(rng, B, N, T):
    """All 16 (f, k) codes in turn; identity / reversed / random frame orders in turn; base indices repeated and unsorted."""
    r = np.empty((B, 3 + T), np.int32)
    b = np.arange(B)
    r[:, 0] = rng.integers(0, N, B)
    r[:, 1], r[:, 2] = b % 4, (b // 4) % 4
    for j in range(B):
        r[j, 3:] = (np.arange(T), np.arange(T)[::-1], rng.permutation(T))[(j // 16) % 3]
    return r[rng.permutation(B)] if B > 16 else r


def _eq_bits(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    as_int = {4: np.uint32, 1: np.uint8}[want.dtype.itemsize]
    np.testing.assert_array_equal(got.view(as_int), np.ascontiguousarray(want).view(as_int))


@pytest.mark.parametrize("mask_dtype", [np.bool_, np.uint8], ids=["bool", "uint8"])
@pytest.mark.parametrize("H,T,C", SHAPES, ids=["h%dt%dc%d" % s for s in SHAPES])
def test_kernel_equals_numpy_bit_for_bit(dev, H, T, C, mask_dtype):
    rng = np.random.default_rng(H * 1000 + T * 10 + C)
    N, S = 6, 3 * (H - 6)
    lr, hr = _bits(rng, (N, H, H, T, C)), _bits(rng, (N, S, S, 1))
    mask = rng.random((N, S, S, 1)) < 0.7 if mask_dtype is np.bool_ else rng.integers(0, 256, (N, S, S, 1)).astype(np.uint8)
    dl, dh, dm = (torch.from_numpy(a).to(dev) for a in (lr, hr, mask))
    for B in (1, 3, 128, 2048):
        rec = _recipes(rng, B, N, T)
        if B >= 48:
            assert len({(f, k, tuple(p)) for f, k, p in zip(rec[:, 1], rec[:, 2], rec[:, 3:])}) >= 48 - 16     # codes x orders really vary
        augment.validate_recipe(rec, N, T)
        got = torch.ops.probav.augment_batch(dl, dh, dm, torch.from_numpy(rec).to(dev))
        for g, w in zip(got, apply_recipe_numpy(lr, hr, mask, rec)):
            _eq_bits(g, w)
    # the sixteen codes one by one at B = 1 (a batch of one takes each code through the launch alone)
    for f in range(4):
        for k in range(4):
            rec = np.array([[N - 1, f, k] + rng.permutation(T).tolist()], np.int32)
            got = torch.ops.probav.augment_batch(dl, dh, dm, torch.from_numpy(rec).to(dev))
            for g, w in zip(got, apply_recipe_numpy(lr, hr, mask, rec)):
                _eq_bits(g, w)


def test_opcheck(dev):
    rng = np.random.default_rng(2)
    lr, hr = rng.random((4, 22, 22, 9, 1), dtype=np.float32), rng.random((4, 48, 48, 1), dtype=np.float32)
    mask = rng.random((4, 48, 48, 1)) < 0.5
    rec = _recipes(rng, 32, 4, 9)
    args = tuple(torch.from_numpy(a).to(dev) for a in (lr, hr, mask, rec))
    torch.library.opcheck(torch.ops.probav.augment_batch.default, args)
    torch.library.opcheck(torch.ops.probav.augment_batch.default, (args[0], args[1], args[2].view(torch.uint8), args[3]))


def _masked_base(n, seed):
    x, hr, mask = synth.synth_batch(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    lr = np.ma.masked_array(x, mask=rng.random(x.shape) < 0.1)
    return lr, np.ma.masked_array(hr, mask=~mask)                    # mask: True = obscured, as the builder writes it


def _materialise(lr, hr, numPermute, flip, rotate, rng):
    a = prep.augmentByShufflingLRImgs(lr, numPermute=numPermute, rng=rng)
    h = np.tile(hr, (numPermute + 1, 1, 1, 1))
    if flip:
        a, h = prep.augmentByFlipping(a), prep.augmentByFlipping(h)
    if rotate:
        a, h = prep.augmentByRotating(a), prep.augmentByRotating(h)
    return a, h


def test_device_dataset_equals_the_materialised_set(dev):
    lr, hr = _masked_base(37, 31)
    a, h = _materialise(lr, hr, 3, 1, 1, np.random.RandomState(5))
    X, y, mk = np.array(a), np.array(h), ~np.ma.getmaskarray(h)
    spec = AugmentSpec(3, 1, 1, seed=5)
    ds = augment.DeviceDataset(np.array(lr), np.array(hr), ~np.ma.getmaskarray(hr), dev)
    assert ds.nbytes == 37 * (22 * 22 * 9 * 4 + 48 * 48 * 4 + 48 * 48) and len(ds) == 37
    V = 37 * spec.multiplicity
    assert V == 2368 == len(X)
    for lo in range(0, V, 128):
        v = np.arange(lo, min(lo + 128, V))
        xb, hb, mb = ds.batch(v, spec)
        assert mb.dtype == torch.bool and xb.dtype == hb.dtype == torch.float32
        _eq_bits(xb, X[v].astype(np.float32))
        _eq_bits(hb, y[v].astype(np.float32))
        _eq_bits(mb, mk[v])
    with pytest.raises(ValueError):
        ds.batch([V], spec)
    bad = augment.make_recipe([0, 1], 37, 9, spec)
    bad[1, 3] = bad[1, 4]
    with pytest.raises(ValueError):
        ds.batch_from_recipe(bad)


def _trainer(dev, d, cls):
    from probav_amd.loss import Losses
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.trainClass import make_optimizer
    model = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)
    losses = Losses(targetShape=(48, 48, 1))
    return cls(model, losses.shiftCompensatedL1Loss, losses.shiftCompensatedcPSNR, make_optimizer("nadam", model, 5e-4),
               os.path.join(d, "ckpt"), os.path.join(d, "logs"))


def test_trainer_consumes_the_same_tensors_and_reaches_the_same_weights(dev, tmp_path):
    from probav_amd.trainClass import ModelTrainer

    class Recording(ModelTrainer):
        def trainStep(self, x, hr, mk):
            self.__dict__.setdefault("seen", []).append((x.clone(), hr.clone(), mk.clone()))
            self.trainLoss(torch.zeros(1, device=x.device)), self.trainPSNR(torch.zeros(1, device=x.device))

    lr, hr = _masked_base(5, 41)
    spec = AugmentSpec(3, 1, 0, seed=9)                              # V = 5 x 4 x 4 = 80: five batches of 16 per epoch
    a, h = _materialise(lr, hr, 3, 1, 0, np.random.RandomState(9))
    X, y, mk = np.array(a), np.array(h), ~np.ma.getmaskarray(h)
    bX, by, bmk = np.array(lr), np.array(hr), ~np.ma.getmaskarray(hr)
    val = [bX, by, bmk]
    host = _trainer(dev, str(tmp_path / "rec_host"), Recording)
    host.fitTrainData(X, [y, mk], 16, 3, val, bufferSize=32, seed=3)
    online = _trainer(dev, str(tmp_path / "rec_online"), Recording)
    online.fitTrainData(bX, [by, bmk], 16, 3, val, bufferSize=32, seed=3, augment=spec)
    assert len(host.seen) == len(online.seen) == 15 and host.step == online.step == 15       # three epochs: two boundaries crossed
    for step, ((x1, h1, m1), (x2, h2, m2)) in enumerate(zip(host.seen, online.seen)):
        assert x1.dtype == x2.dtype and h1.dtype == h2.dtype and m1.dtype == m2.dtype, step
        assert torch.equal(x1.view(torch.int32), x2.view(torch.int32)) and torch.equal(h1.view(torch.int32), h2.view(torch.int32)), step
        assert torch.equal(m1, m2), step

    def run(name, online_path):
        tr = _trainer(dev, str(tmp_path / name), ModelTrainer)
        if online_path:
            tr.fitTrainData(bX, [by, bmk], 16, 6, val, bufferSize=32, seed=3, augment=spec)
        else:
            tr.fitTrainData(X, [y, mk], 16, 6, val, bufferSize=32, seed=3)
        torch.cuda.synchronize()
        assert tr.step == 30
        return tr.model.flat.detach().clone()
    h1, h2, o = run("host1", False), run("host2", False), run("online", True)
    assert torch.isfinite(o).all()
    bar, diff = float((h1 - h2).abs().max()), float((o - h1).abs().max())
    print("max |online - host| = %g, max |host - host'| = %g" % (diff, bar))
    assert diff <= bar, (diff, bar)                                  # the bar is the materialised path's own run-to-run difference


CFG = """[Directories]
raw_data={d}/raw
preprocessing_out={d}/pre
model_out={d}/modelInfo
train_out={d}/trainout
test_out={d}/testout

[Train]
batch_size=1
epochs=1
learning_rate=0.0005
optimizer=nadam
loss=l1
split=0.2

[Net]
num_res_blocks=12
num_low_res_imgs=9
scale=3
num_filters=32
kernel_size=3
exp_rate=8
decay_rate=0.8
is_grayscale=1

[Preprocessing]
max_shift=6
patch_size=16
patch_stride=16
num_low_res_imgs_pre=9
low_res_patch_thresholds=0.85
low_res_threshold=0.3
high_res_threshold=0.85
num_low_res_permute=2
to_flip=1
to_rotate=1
ckpt=1,2,3,4,5
"""


def _run(args, cwd, **extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PROBAV_FORCE_DP"):
        env.pop(k, None)
    env.update(extra)
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return out


def test_train_py_online_aug_equals_train_py(dev, tmp_path):
    d = str(tmp_path)
    aug = os.path.join(d, "pre", "augmentedPatchesDir")
    os.makedirs(aug)
    # 21 base patches x 3 frame orders x 4 flips x 4 turns = 1008 virtual patches at batch_size 1: the epoch reaches the evaluation (and
    # checkpoint) of step 1000 once (models/trainClass.py:25,110-122)
    lr, hr = _masked_base(21, 51)
    perms = augment.draw_perms(2, 9, np.random.RandomState(13))
    a, h = _materialise(lr, hr, 2, 1, 1, np.random.RandomState(13))
    assert len(a) == 1008
    a.dump(os.path.join(aug, "TRAINpatchesLR_NIR.npy"), protocol=4)
    h.dump(os.path.join(aug, "TRAINpatchesHR_NIR.npy"), protocol=4)
    lr.dump(os.path.join(aug, "TRAINbasepatchesLR_NIR.npy"), protocol=4)
    hr.dump(os.path.join(aug, "TRAINbasepatchesHR_NIR.npy"), protocol=4)
    np.save(os.path.join(aug, "TRAINaugperms_NIR.npy"), perms)
    lr[:6].dump(os.path.join(aug, "TRAINVALpatchesLR_NIR.npy"), protocol=4)
    hr[:6].dump(os.path.join(aug, "TRAINVALpatchesHR_NIR.npy"), protocol=4)
    weights = {}
    for name, flags, env in (("mat1", [], {}), ("mat2", [], {}), ("onl", ["--online-aug"], {}),
                             ("onldp", ["--online-aug"], {"PROBAV_FORCE_DP": "1", "MASTER_PORT": "29581"})):
        cfg = os.path.join(d, name + ".cfg")
        with open(cfg, "w") as fh:
            fh.write(CFG.format(d=d))
        out = _run([os.path.join(ROOT, "train.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d, **env)
        assert "[ EPOCH 0/1 ] - [ STEP 1008/1008 ]" in out.stderr and "[ SAVE ] Saving checkpoint..." in out.stderr, out.stderr[-2000:]
        ck = os.path.join(d, "modelInfo", "ckpt_" + name, "NIR")
        assert open(os.path.join(ck, "checkpoint.pt-index")).read().split() == ["ckpt-1.pt"]
        state = torch.load(os.path.join(ck, "ckpt-1.pt"), map_location="cpu")
        assert state["step"] == 1000
        weights[name] = torch.cat([t.reshape(-1) for layer in sorted(state["model"]) for _, t in sorted(state["model"][layer].items())])
        if flags:
            assert "un-augmented samples on the device" in out.stderr
    bar = float((weights["mat1"] - weights["mat2"]).abs().max())
    for name in ("onl", "onldp"):
        diff = float((weights[name] - weights["mat1"]).abs().max())
        print("%s: max |online - materialised| = %g, materialised run to run = %g" % (name, diff, bar))
        assert diff <= bar, (name, diff, bar)
