"""The test-time self-ensemble on the device (csrc/kernels_ensemble.hip, probav_amd/ensemble.py, testClass.resolve_ensemble): both kernels
against their numpy statements bit for bit, the whole path against a composition of parts that existed before it (torch.flip / rot90 /
index_select around resolve_device, summed in float64), V = 1 against the plain path, equivariance, launch-set independence, the CLI.
Every comparison is an equality: members are integers, their sum is exact, and there is one correctly rounded division."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probav_amd.ops  # noqa: F401  (registers torch.ops.probav.ensemble_*)
from probav_amd import _lib, augment, synth, testClass
from probav_amd.augment import FLIP_AXES, apply_recipe_numpy
from probav_amd.ensemble import EnsembleSpec, ensemble_reduce_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HI = float(2 ** 16)


def _model(dev, impl=None):
    from probav_amd.modelsTF import WDSRConv3D
    m = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)
    if impl is not None:
        m.set_impl(impl)
    return m


def _eq_bits(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


EXPAND_SHAPES = [(22, 9, 1), (22, 9, 3), (22, 13, 1), (15, 7, 1)]          # 15 * 15 * 7 floats: a sample that is not a multiple of 16 bytes


@pytest.mark.parametrize("H,T,C", EXPAND_SHAPES, ids=["h%dt%dc%d" % s for s in EXPAND_SHAPES])
def test_expand_equals_numpy_bit_for_bit(dev, H, T, C):
    rng = np.random.default_rng(H * 100 + T * 10 + C)
    N = 5
    assert ((H * H * T * C * 4) % 16 != 0) == (H == 15)
    lr = rng.integers(0, 2 ** 32, size=(N, H, H, T, C), dtype=np.uint32).view(np.float32)          # arbitrary bits: the kernel moves them
    hr, mask = np.zeros((N, 3, 3, 1), np.float32), np.zeros((N, 3, 3, 1), bool)
    dl = torch.from_numpy(lr).to(dev)
    for B in (16, 1, 131):
        rec = np.empty((B, 3 + T), np.int32)
        b = np.arange(B)
        rec[:, 0], rec[:, 1], rec[:, 2] = rng.integers(0, N, B), b % 4, (b // 4) % 4                 # all 16 (f, k) codes
        for j in range(B):
            rec[j, 3:] = rng.permutation(T)
        augment.validate_recipe(rec, N, T)
        got = torch.ops.probav.ensemble_expand(dl, torch.from_numpy(rec).to(dev))
        _eq_bits(got, apply_recipe_numpy(lr, hr, mask, rec)[0])
    # the recipes the ensemble itself makes
    spec = EnsembleSpec("d8", permute=2, seed=H)
    rec = spec.recipe(N, T)
    _eq_bits(torch.ops.probav.ensemble_expand(dl, torch.from_numpy(rec).to(dev)), apply_recipe_numpy(lr, hr, mask, rec)[0])


def _synthetic_predictions(rng, rows, S):
    sr = rng.integers(-3000, 2 ** 16 + 3000, (rows, S, S)).astype(np.float32)
    sr += rng.integers(0, 2, (rows, S, S)).astype(np.float32) * np.float32(0.5)                    # half of them ties
    sr[:, 1, :4] = np.array([0.5, 1.5, 2.5, -0.5], np.float32)
    sr[:, 2, :4] = np.array([65535.5, 65536.5, 1e9, -1e9], np.float32)
    sr[:, 3] = rng.random((rows, S)).astype(np.float32) * 5
    return sr


@pytest.mark.parametrize("S", [48, 30])
@pytest.mark.parametrize("V", [1, 3, 8, 24, 256])
def test_reduce_equals_numpy_bit_for_bit(dev, V, S):
    rng = np.random.default_rng(V * 100 + S)
    spec = {1: EnsembleSpec(None), 3: EnsembleSpec(None, permute=2, seed=1), 8: EnsembleSpec("d8"), 24: EnsembleSpec("d8", permute=2, seed=2),
            256: EnsembleSpec("d8", permute=31, seed=3)}[V]
    assert spec.V == V
    sets, grid = 2, 2
    N = sets * grid * grid
    rec = spec.recipe(N, 9)
    if V == 3:                                          # frame orders alone have no geometry: give these rows all 16 codes over the patches
        rec[:, 1], rec[:, 2] = np.arange(N * V) % 4, (np.arange(N * V) // 4) % 4
    sr = _synthetic_predictions(rng, N * V, S)
    dsr, drec = torch.from_numpy(sr).to(dev), torch.from_numpy(rec).to(dev)
    for final in ("mean", "round"):
        want = ensemble_reduce_numpy(sr, rec, V, final=final)
        got = torch.ops.probav.ensemble_reduce(dsr, drec, V, 0.0, HI, final == "round", 0, 0)
        _eq_bits(got, want)
        _eq_bits(torch.ops.probav.ensemble_reduce(dsr.unsqueeze(-1), drec, V, 0.0, HI, final == "round", 0, 0), want)
        img = torch.ops.probav.ensemble_reduce(dsr, drec, V, 0.0, HI, final == "round", sets, grid)
        assert torch.equal(img, testClass.stitch_device(got.unsqueeze(-1), sets))
        _eq_bits(img, ensemble_reduce_numpy(sr, rec, V, final=final, sets=sets, grid=grid))
    if V == 3:
        assert np.any(ensemble_reduce_numpy(sr, rec, V) % 1 != 0)                                    # thirds occur: the two forms really differ
    _eq_bits(torch.ops.probav.ensemble_reduce(dsr, drec, V, 100.0, 4000.0, False, 0, 0), ensemble_reduce_numpy(sr, rec, V, lo=100.0, hi=4000.0))


def test_reduce_refuses_bad_arguments_and_skips_a_bad_row(dev):
    L = _lib.lib()
    S, V, N = 48, 8, 3
    rec = EnsembleSpec("d8").recipe(N, 9)
    sr = torch.from_numpy(_synthetic_predictions(np.random.default_rng(0), N * V, S)).to(dev)
    drec = torch.from_numpy(rec).to(dev)
    out = torch.full((N, S, S), -7.0, device=dev)
    call = lambda n, v, s, lo, hi, grid, r=drec: L.probav_ensemble_reduce(_lib.ptr(sr), _lib.ptr(r), n, v, 9, s, lo, hi, 0, grid, _lib.ptr(out),
                                                                         _lib.current_stream())
    for args, word in (((N, 257, S, 0.0, HI, 0), "256"), ((N, 0, S, 0.0, HI, 0), "256"), ((N, V, 91, 0.0, HI, 0), "LDS"), ((N, V, S, 1.0, 0.0, 0), "lo <= hi"),
                       ((N, V, S, 0.0, HI, 2), "whole images"), ((0, V, S, 0.0, HI, 0), "n_base")):
        assert call(*args) == _lib.PROBAV_EINVAL
        assert word in L.probav_last_error().decode(), (args, L.probav_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                 # nothing was launched
    with pytest.raises(ValueError, match="sum exactly in fp32"):
        torch.ops.probav.ensemble_reduce(torch.zeros(257, S, S, device=dev), torch.zeros(257, 12, dtype=torch.int32, device=dev), 257, 0.0, HI, False, 0, 0)
    # a code outside 0..3 in the device recipe: that base patch is skipped, the others are reduced
    bad = rec.copy()
    bad[V + 5, 2] = 4
    dbad = torch.from_numpy(bad).to(dev)
    assert call(N, V, S, 0.0, HI, 0, dbad) == _lib.PROBAV_OK
    torch.cuda.synchronize()
    want = ensemble_reduce_numpy(sr.cpu().numpy(), rec, V)
    assert bool((out[1] == -7.0).all())
    _eq_bits(out[0], want[0])
    _eq_bits(out[2], want[2])
    # expand: the same guard as augment_batch
    lr = torch.ones(2, 22, 22, 9, 1, device=dev)
    xo = torch.full((3, 22, 22, 9, 1), -7.0, device=dev)
    r3 = EnsembleSpec("d8").recipe(2, 9)[[0, 9, 3]].copy()
    r3[1, 0] = 2                                                     # base index past the end
    dr3 = torch.from_numpy(r3).to(dev)
    assert L.probav_ensemble_expand(_lib.ptr(lr), 2, 22, 9, 1, _lib.ptr(dr3), 3, _lib.ptr(xo), _lib.current_stream()) == _lib.PROBAV_OK
    torch.cuda.synchronize()
    assert bool((xo[1] == -7.0).all()) and bool((xo[0] == 1.0).all()) and bool((xo[2] == 1.0).all())
    assert L.probav_ensemble_expand(_lib.ptr(lr), 2, 22, 65, 1, _lib.ptr(drec), 3, _lib.ptr(xo), _lib.current_stream()) == _lib.PROBAV_EINVAL


def _compose(model, xd, table):
    """E(x) from parts that exist without the feature: each variant through torch.flip / rot90 / index_select and resolve_device, turned back,
    summed in float64, divided, cast."""
    acc = torch.zeros((xd.shape[0], 48, 48, 1), dtype=torch.float64, device=xd.device)
    for row in table:
        f, k, perm = int(row[0]), int(row[1]), torch.as_tensor(row[2:].astype(np.int64)).to(xd.device)
        dims = [a + 1 for a in FLIP_AXES[f]]
        xv = xd.index_select(3, perm)
        xv = torch.rot90(torch.flip(xv, dims) if dims else xv, k, dims=(1, 2)).contiguous()
        m = torch.rot90(testClass.resolve_device(model, xv), -k, dims=(1, 2))
        acc += (torch.flip(m, dims) if dims else m).double()
    return (acc / len(table)).float()


@pytest.mark.parametrize("impl", [None, 2, 3], ids=["default", "impl2", "impl3"])
def test_whole_path_equals_the_composition_of_existing_parts(dev, impl):
    model = _model(dev, impl)
    x = synth.synth_batch(12, seed=7)[0]
    xd = torch.as_tensor(x).to(dev)
    for spec in (EnsembleSpec("d8"), EnsembleSpec("d8", permute=1, seed=3), EnsembleSpec(None, permute=2, seed=4)):
        want = _compose(model, xd, spec.table(9))
        got = testClass.resolve_ensemble(model, x, spec)
        assert got.shape == want.shape == (12, 48, 48, 1) and got.dtype == torch.float32
        assert torch.equal(got, want), (impl, spec.V, float((got - want).abs().max()))
        assert torch.equal(testClass.resolve_ensemble(model, xd, spec, final="round"), torch.round(want))          # torch.round: half to even
        assert torch.equal(testClass.resolve_ensemble(model, x, spec, launch_batch=5 * spec.V), want)               # 5 + 5 + 2 patches
    plain = testClass.resolve_device(model, xd)
    d8 = testClass.resolve_ensemble(model, x, EnsembleSpec("d8"))
    assert not torch.equal(d8, plain)                               # the network is not equivariant: the ensemble is a different image


def test_one_member_is_the_plain_path(dev):
    model = _model(dev)
    p = synth.synth_batch(2 * 64, seed=9)[0].reshape(2, 64, 22, 22, 9, 1)
    plain = testClass.evaluate_device(model, p)
    for final in ("round", "mean"):
        one = testClass.evaluate_device(model, p, ensemble=EnsembleSpec(None), final=final)
        assert len(one) == len(plain) == 2
        for a, b in zip(one, plain):
            assert a.shape == b.shape == (384, 384, 1) and a.dtype == b.dtype == np.float64
            np.testing.assert_array_equal(a, b)
    assert torch.equal(testClass.resolve_ensemble(model, p[0], EnsembleSpec(None)), testClass.resolve_device(model, p[0]))


def test_d8_ensemble_is_equivariant(dev):
    model = _model(dev)
    x = synth.synth_batch(4, seed=11)[0]
    xd = torch.as_tensor(x).to(dev)
    spec = EnsembleSpec("d8")
    E = testClass.resolve_ensemble(model, xd, spec)
    plain = testClass.resolve_device(model, xd)
    broken = 0
    for f in range(4):
        for k in range(4):
            dims = [a + 1 for a in FLIP_AXES[f]]
            A = lambda t: torch.rot90(torch.flip(t, dims) if dims else t, k, dims=(1, 2)).contiguous()
            assert torch.equal(testClass.resolve_ensemble(model, A(xd), spec), A(E)), (f, k)
            broken += not torch.equal(testClass.resolve_device(model, A(xd)), A(plain))
    assert broken >= 1                                              # ... although the network itself is not


def test_images_do_not_depend_on_the_launch_sets(dev):
    model = _model(dev)
    p = synth.synth_batch(3 * 64, seed=13)[0].reshape(3, 64, 22, 22, 9, 1)
    spec = EnsembleSpec("d8")
    V = spec.V
    ref = testClass.resolve_images(model, p, ensemble=spec)
    assert ref.shape == (3, 384, 384) and ref.dtype == torch.float32
    for lb in (V, 3 * V, 64 * V, 100 * V):                          # one patch, three, one whole image, one image and a bit (rounded down to one)
        assert torch.equal(testClass.resolve_images(model, p, ensemble=spec, launch_batch=lb), ref), lb
    patches = testClass.resolve_ensemble(model, p.reshape(-1, 22, 22, 9, 1), spec, final="round")
    assert torch.equal(testClass.stitch_device(patches, 3), ref)
    mean = testClass.resolve_images(model, p, ensemble=spec, final="mean")
    assert torch.equal(torch.round(mean), ref) and not torch.equal(mean, ref)


def test_opcheck(dev):
    rng = np.random.default_rng(2)
    lr = torch.from_numpy(rng.random((4, 22, 22, 9, 1), dtype=np.float32)).to(dev)
    spec = EnsembleSpec("d8", permute=1, seed=0)
    rec = torch.from_numpy(spec.recipe(4, 9)).to(dev)
    torch.library.opcheck(torch.ops.probav.ensemble_expand.default, (lr, rec))
    sr = torch.from_numpy(_synthetic_predictions(rng, 4 * 16, 48)).to(dev)
    torch.library.opcheck(torch.ops.probav.ensemble_reduce.default, (sr, rec, 16, 0.0, HI, False, 0, 0))
    torch.library.opcheck(torch.ops.probav.ensemble_reduce.default, (sr.unsqueeze(-1), rec, 16, 0.0, HI, True, 1, 2))


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
num_low_res_permute=0
to_flip=0
to_rotate=0
ckpt=1,2,3,4,5
"""


def _run(args, cwd):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PROBAV_FORCE_DP"):
        env.pop(k, None)
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return out


def test_test_py_ensemble_flags(dev, tmp_path):
    from probav_amd.pngio import imread_uint16
    from probav_amd.trainClass import ModelTrainer
    d = str(tmp_path)
    res = os.path.join(d, "pre", "resolverDir")
    os.makedirs(res)
    sets = 3
    test_patches = synth.synth_batch(sets * 64, seed=6)[0].reshape(sets, 64, 22, 22, 9, 1)
    np.ma.masked_array(test_patches.transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((sets, 64, 9, 1, 22, 22), bool)).dump(
        os.path.join(res, "TESTpatchesLR_NIR.npy"))
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d))
    with open(os.path.join(d, "removedTrainSetsNIR.txt"), "w") as fh:
        fh.write("1307\n1308.0\n")
    model = _model(dev)
    ck = os.path.join(d, "modelInfo", "ckpt_mini", "NIR")
    assert ModelTrainer(model, None, None, None, ck, os.path.join(d, "modelInfo", "logs_mini", "NIR")).save() == "ckpt-1.pt"

    spec = EnsembleSpec("d8", permute=1, seed=3)
    want_ens = testClass.evaluate_device(model, test_patches, ensemble=spec, final="round")
    want_plain = testClass.evaluate_device(model, test_patches)
    names = ["imgset1306.png", "imgset1309.png", "imgset1310.png"]
    for flags, want in ((["--ensemble", "d8", "--ensemble-permute", "1", "--ensemble-seed", "3"], want_ens), (["--ensemble", "none"], want_plain)):
        for f in glob.glob(os.path.join(d, "testout_mini", "*.png")):
            os.remove(f)
        out = _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
        assert "Model restored from checkpoint at step 0" in out.stdout, out.stdout[-500:]
        pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "testout_mini", "*.png")))
        assert pngs == names, pngs
        for name, w in zip(names, want):
            np.testing.assert_array_equal(imread_uint16(os.path.join(d, "testout_mini", name)), w[:, :, 0].astype(np.uint16))
    assert any(not np.array_equal(a, b) for a, b in zip(want_ens, want_plain))
