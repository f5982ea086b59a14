"""Dataset builder on the device (csrc/kernels_prep.hip via probav_amd.prep): registration against the exact integer correlation,
the fp32 surface against its declared bound, the patch unfold against the reference's gather map, and utils/dataGenerator.py end to end
on a synthetic raw dataset in the ESA layout."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.prep_helpers import encode_png, exact_shift, exact_xcorr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
N = 128


def _texture(rng, lo=2000, hi=20000):
    f = np.fft.fft2(rng.standard_normal((N, N)))
    k = np.fft.fftfreq(N)
    f *= 1.0 / (1e-3 + np.hypot(k[:, None], k[None, :]) ** 1.5)
    t = np.fft.ifft2(f).real
    t = (t - t.min()) / (t.max() - t.min())
    return (lo + t * (hi - lo)).astype(np.int64)


def _corpus():
    rng = np.random.default_rng(11)
    sets = []
    # 9 frames: one texture rolled by known shifts (+-64, 0, wrap-around), plus noise
    base = _texture(rng)
    shifts = [(0, 0), (64, 64), (-64, 3), (1, 127), (127, 1), (5, -7), (64, -64), (-1, -1), (33, 90)]
    sets.append([np.clip(np.roll(base, s, axis=(0, 1)) + rng.integers(-40, 40, (N, N)), 0, 65535) for s in shifts])
    # 10 frames: uncorrelated textures, a constant and an all-zero frame
    fr = [_texture(rng) for _ in range(8)] + [np.full((N, N), 777), np.zeros((N, N), np.int64)]
    sets.append(fr)
    # 35 frames: sparse low values (exact ties, +-1 near-ties), full-range 16-bit noise, constants, rolled textures
    fr = [_texture(rng, 0, 65535)]
    for i in range(12):
        a = np.zeros((N, N), np.int64)
        idx = rng.integers(0, N * N, 6 + i)
        a.flat[idx] = rng.integers(1, 3, len(idx))
        fr.append(a)
    fr += [rng.integers(0, 65536, (N, N)) for _ in range(10)]
    fr += [np.full((N, N), 65535), np.zeros((N, N), np.int64), np.full((N, N), 1)]
    fr += [np.roll(fr[0], (int(rng.integers(0, N)), int(rng.integers(0, N))), axis=(0, 1)) for _ in range(9)]
    sets.append(fr)
    sets.insert(0, [sets[2][13], np.full((N, N), 3)] + [sets[2][i] for i in range(14, 21)])     # a set whose reference is noise
    # 10 frames whose reference is itself sparse and low-valued: a few exact ties inside the window on the fast path, +-1 near-ties
    sp = np.zeros((N, N), np.int64)
    sp.flat[rng.integers(0, N * N, 12)] = rng.integers(1, 3, 12)
    fr = [sp]
    for i in range(9):
        a = np.roll(sp, (int(rng.integers(0, N)), int(rng.integers(0, N))), axis=(0, 1)) if i % 3 else np.zeros((N, N), np.int64)
        a.flat[rng.integers(0, N * N, 4 + i)] = rng.integers(1, 3, 4 + i)
        fr.append(a)
    sets.append(fr)
    frames = [np.stack(s).astype(np.uint16) for s in sets]
    masks = [rng.random((len(s), N, N)) < 0.9 for s in sets]
    return frames, masks


def test_registration_equals_the_exact_argmax(dev):
    from probav_amd import prep
    frames, masks = _corpus()
    sizes = [len(f) for f in frames]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    F, M = np.concatenate(frames), np.concatenate(masks)
    shifts, rf, rm, rc = prep.device_register(F, M, off, off[:-1])
    for s in range(len(sizes)):
        ref = F[off[s]]
        for f in range(off[s], off[s + 1]):
            if f == off[s]:
                want, raw = (0, 0), (0, 0)
            else:
                want, raw = exact_shift(ref, F[f])
            assert tuple(shifts[f]) == tuple(int(v) for v in want), (s, f - off[s], shifts[f], want)
            np.testing.assert_array_equal(rf[f], np.roll(F[f], raw, axis=(0, 1)))
            np.testing.assert_array_equal(rm[f], np.roll(M[f], raw, axis=(0, 1)))
            assert rc[f] == np.count_nonzero(M[f])
    # the sparse set does take the tie rule on the fast path: several shifts share the exact maximum, fewer than 512 of them
    ties = [int((exact_xcorr(F[off[4]], F[f]) == exact_xcorr(F[off[4]], F[f]).max()).sum()) for f in range(off[4] + 1, off[5])]
    assert any(1 < t < 512 for t in ties), ties
    with pytest.raises(ValueError):
        prep.device_register(F[:9], M[:9], np.array([0, 4, 4, 9]), np.array([0, 4, 4]))      # an empty set is refused, not launched


def test_surface_stays_within_the_declared_bound(dev):
    from probav_amd import prep
    frames, _ = _corpus()
    pairs = [(frames[1][0], frames[1][k]) for k in (1, 4, 8)] + [(frames[3][0], frames[3][k]) for k in (1, 14, 20, 30)]
    for ref, img in pairs:
        surf, info = prep.device_xcorr_surface(ref, img)
        r, g = ref.astype(np.int64), img.astype(np.int64)
        exact = exact_xcorr(r, g) - info["c_img"] * r.sum() - info["c_ref"] * g.sum() + N * N * info["c_ref"] * info["c_img"]
        assert info["c_ref"] == r.sum() // (N * N) and info["c_img"] == g.sum() // (N * N)
        err = np.abs(surf.astype(np.float64) - exact).max()
        assert err <= info["B"] / 4, (err, info)


def _ids(Z, key):
    return np.cumsum(Z[key + "_diff"].astype(np.int64)).reshape(Z[key + "_shape"])


def test_patch_unfold_matches_the_reference_gather_map(dev):
    from probav_amd import prep
    Z = np.load(os.path.join(ROOT, "tests", "golden", "ref_plumbing.npz"))
    for shape_key, key in (("unfold_frames_shape", "unfold_patches"),):
        s, T, C, H, W = Z[shape_key].tolist()
        frames = np.arange(s * T * H * W, dtype=np.float32).reshape(s, T, C, H, W)
        rng = np.random.default_rng(1)
        mask = rng.random(frames.shape) < 0.3
        p, counts = prep._patches(np.ma.masked_array(frames, mask=mask), 22, 16, 3)
        got = np.ma.getdata(p).transpose(0, 1, 4, 5, 2, 3)
        np.testing.assert_array_equal(got.astype(np.int64), _ids(Z, key))
        pm = np.pad(mask, [(0, 0)] * 3 + [(3, 3), (3, 3)], mode="reflect")
        want = np.stack([np.stack([pm[:, :, 0, i * 16:i * 16 + 22, j * 16:j * 16 + 22] for i in range(4) for j in range(4)], 1)], 0)[0]
        np.testing.assert_array_equal(np.ma.getmaskarray(p)[:, :, :, 0], want)
        np.testing.assert_array_equal(counts, want.reshape(*want.shape[:3], -1).sum(-1))
    # HR geometry: no pad, window = stride = 48
    hr = np.arange(2 * 384 * 384, dtype=np.float32).reshape(2, 1, 1, 384, 384)
    p, _ = prep._patches(np.ma.masked_array(hr, mask=np.zeros(hr.shape, bool)), 48, 48, 0)
    want = hr[:, 0, 0].reshape(2, 8, 48, 8, 48).transpose(0, 1, 3, 2, 4).reshape(2, 64, 1, 1, 48, 48)
    np.testing.assert_array_equal(np.ma.getdata(p), want)


def test_count_nonzero_kernel(dev):
    from probav_amd import prep
    a = np.random.default_rng(2).random((37, 1000)) < 0.4
    np.testing.assert_array_equal(prep.device_count_nonzero(a, 1000), a.sum(1))


CFG = """[Directories]
raw_data={d}/raw
preprocessing_out={d}/pre
model_out={d}/modelInfo
train_out={d}/trainout
test_out={d}/testout

[Train]
batch_size=4
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
num_low_res_permute=1
to_flip=1
to_rotate=1
ckpt=1,2,3,4,5
"""


def _write_raw(root, rng):
    """4 train + 4 test sets: set 1 of train is corrupt (every frame < 30 % clear), set 2 has only 6 clear frames of 9."""
    raw = {}
    for split in ("train", "test"):
        for k in range(4):
            d = os.path.join(root, "raw", split, "NIR", "imgset%04d" % (k + (0 if split == "train" else 1160)))
            os.makedirs(d)
            base = _texture(rng, 1000, 30000)
            n = 9 + k
            lr = [np.clip(np.roll(base, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(0, 1)) + rng.integers(0, 50, (N, N)), 0, 65535)
                  for _ in range(n)]
            qm = [rng.random((N, N)) < (0.97 if i % 4 else 0.8) for i in range(n)]
            if split == "train" and k == 1:
                qm = [rng.random((N, N)) < 0.2 for _ in range(n)]
            if split == "train" and k == 2:
                qm = [m if i < 6 else rng.random((N, N)) < 0.1 for i, m in enumerate(qm)]
            for i in range(n):
                open(os.path.join(d, "LR%03d.png" % i), "wb").write(encode_png(lr[i], 16))
                open(os.path.join(d, "QM%03d.png" % i), "wb").write(encode_png(qm[i], 1))
            if split == "train":
                hr = np.kron(base, np.ones((3, 3), np.int64))
                open(os.path.join(d, "HR.png"), "wb").write(encode_png(hr, 16))
                open(os.path.join(d, "SM.png"), "wb").write(encode_png(rng.random((3 * N, 3 * N)) < 0.97, 1))
            raw[(split, k)] = (np.stack(lr).astype(np.uint16), np.stack(qm))
    return raw


def _oracle_register(lr, qm):
    cnt = np.array([-np.count_nonzero(m) for m in qm])
    o = np.argsort(cnt)
    lr, qm = lr[o], qm[o]
    out, msk = [lr[0].astype(np.float64)], [~qm[0]]
    for i in range(1, len(lr)):
        _, s = exact_shift(lr[0], lr[i])
        out.append(np.roll(lr[i], s, axis=(0, 1)).astype(np.float64))
        msk.append(~np.roll(qm[i], s, axis=(0, 1)))
    return np.ma.masked_array(np.stack(out)[:, None], mask=np.stack(msk)[:, None])


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(np.ma.getdata(a), np.ma.getdata(b))
    np.testing.assert_array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b))


def test_data_generator_cli_end_to_end(dev, tmp_path):
    from probav_amd import prep
    from probav_amd.parseConfig import parseConfig
    d = str(tmp_path)
    raw = _write_raw(d, np.random.default_rng(5))
    cfgp = os.path.join(d, "t.cfg")
    open(cfgp, "w").write(CFG.format(d=d))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "utils", "dataGenerator.py"), "--cfg", cfgp, "--band", "NIR", "--seed", "3"],
                         cwd=d, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    cfg = parseConfig(cfgp)
    pre = os.path.join(d, "pre")
    load = lambda sub, n: np.load(os.path.join(pre, sub, n + "_NIR.npy"), allow_pickle=True)

    # checkpoint 1: ragged sets as object arrays of per-set arrays
    a = load("arrayDir", "TRAINimgLR")
    assert a.dtype == object and len(a) == 4 and a[3].shape == (12, 1, N, N) and a[3].dtype == np.uint16
    np.testing.assert_array_equal(a[0][:, 0], raw[("train", 0)][0])
    q = load("arrayDir", "TESTmskLR")
    assert q[2].dtype == np.bool_ and np.array_equal(q[2][:, 0], raw[("test", 2)][1])

    # checkpoint 2 against the CPU restatement: exact registration + the host bookkeeping under the same seed
    rng = np.random.RandomState(3)
    reg = prep._objects([_oracle_register(*raw[("train", k)]) for k in range(4)])
    hr = prep.convertToMaskedArray(load("arrayDir", "TRAINimgHR"), load("arrayDir", "TRAINmskHR"))
    _same(load("resolverDir", "TRAINimgHR"), hr)
    tl, th, removed = prep.removeCorruptedTrainImageSets(reg, hr, cfg["low_res_threshold"])
    assert list(removed) == [1]
    np.testing.assert_array_equal(np.loadtxt(os.path.join(d, "removedTrainSetsNIR.txt")), [595.0])
    tl = prep.pickClearLRImgsPerImgSet(tl, cfg["num_low_res_imgs_pre"], cfg["low_res_threshold"], rng)
    regt = prep._objects([_oracle_register(*raw[("test", k)]) for k in range(4)])
    tt = prep.pickClearLRImgsPerImgSet(prep.removeCorruptedTestImageSets(regt, cfg["low_res_threshold"]), 9, cfg["low_res_threshold"], rng)
    _same(load("trimmedArrayDir", "TRAINimgLR"), tl)
    _same(load("trimmedArrayDir", "TRAINimgHR"), th)
    _same(load("trimmedArrayDir", "TESTimgLR"), tt)
    assert tl.dtype == np.float64 and tl.shape == (3, 9, 1, N, N)

    # checkpoint 3: numpy pad + unfold of the trimmed arrays
    def unfold(x, k, st, pad):
        d_ = np.pad(np.ma.getdata(x).astype(np.float32), [(0, 0)] * 3 + [(pad, pad)] * 2, mode="reflect")
        m_ = np.pad(np.ma.getmaskarray(x), [(0, 0)] * 3 + [(pad, pad)] * 2, mode="reflect")
        n = (d_.shape[-1] - k) // st + 1
        cut = lambda a: np.stack([a[:, :, :, i * st:i * st + k, j * st:j * st + k] for i in range(n) for j in range(n)], 1)
        return np.ma.masked_array(cut(d_), mask=cut(m_))
    _same(load("patchesDir", "TESTpatchesLR"), unfold(tt, 22, 16, 3))
    _same(load("patchesDir", "TRAINpatchesLR"), unfold(tl, 22, 16, 3))
    _same(load("patchesDir", "TRAINpatchesHR"), unfold(th, 48, 48, 0))

    # checkpoint 4 and 5: the host functions on the restated patches
    t4 = prep.pickClearPatchesLR(unfold(tt, 22, 16, 3), 9, 0.85)
    l4 = prep.pickClearPatchesLR(unfold(tl, 22, 16, 3), 9, 0.85)
    _same(load("resolverDir", "TESTpatchesLR"), t4)
    assert t4.shape == (4, 64, 9, 1, 22, 22)
    _same(load("resolverDir", "TRAINpatchesLR"), l4)
    l4, h4 = prep.pickClearPatches(*prep.removeCorruptedTrainPatchSets(l4, unfold(th, 48, 48, 0), 0.85), 0.85)
    l4, h4 = l4.transpose((0, 3, 4, 1, 2)), h4.transpose((0, 3, 4, 1, 2)).squeeze(4)
    _same(load("trimmedPatchesDir", "TRAINpatchesLR"), l4)
    _same(load("trimmedPatchesDir", "TRAINpatchesHR"), h4)
    assert l4.ndim == 5 and l4.shape[1:] == (22, 22, 9, 1) and h4.shape[1:] == (48, 48, 1)
    l5, lv, h5, hv = prep.splitPatches(l4, h4, cfg)
    _same(load("augmentedPatchesDir", "TRAINVALpatchesLR"), lv)
    _same(load("augmentedPatchesDir", "TRAINVALpatchesHR"), hv)
    l5 = prep.augmentByRotating(prep.augmentByFlipping(prep.augmentByShufflingLRImgs(l5, 1, rng)))
    h5 = prep.augmentByRotating(prep.augmentByFlipping(np.tile(h5, (2, 1, 1, 1))))
    _same(load("augmentedPatchesDir", "TRAINpatchesLR"), l5)
    _same(load("augmentedPatchesDir", "TRAINpatchesHR"), h5)
    assert len(l5) >= 4000                                  # >= 1000 steps at batch 4: train.py's first evaluation and checkpoint

    # the consumers: train.py for one epoch on augmentedPatchesDir, then test.py on resolverDir/TESTpatchesLR and removedTrainSetsNIR.txt
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PROBAV_FORCE_DP")}
    for script in ("train.py", "test.py"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--cfg", cfgp, "--band", "NIR"], cwd=d, env=env,
                             capture_output=True, text=True, timeout=1500)
        assert out.returncode == 0, (script, out.stdout[-1500:], out.stderr[-3000:])
    assert open(os.path.join(d, "modelInfo", "ckpt_t", "NIR", "checkpoint.pt-index")).read().split() == ["ckpt-1.pt"]
    pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "testout_t", "*.png")))
    assert pngs == ["imgset1306.png", "imgset1307.png", "imgset1308.png", "imgset1309.png"], pngs      # the four test sets, first NIR id 1306
