"""Overlapped-tile inference on the device (csrc/kernels_tile.hip, probav_amd/tiles.py, testClass.resolve_tiled): the blend kernel against its
numpy int64 statement bit for bit, the whole path against parts that exist without it (the builder's unfold and pickClearPatchesLR on the host,
resolve_device in batches of 16, the numpy blend), stride P against the plain path, independence of launch sets and chunks, the ensemble, the
CLIs.  Every comparison is an equality: after each tile's own rint the arithmetic is integer."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probav_amd.ops  # noqa: F401  (registers torch.ops.probav.tile_blend)
from probav_amd import _lib, prep, testClass, tiles
from probav_amd.ensemble import EnsembleSpec
from probav_amd.tiles import TileSpec, tile_blend_numpy

from tests.tiles_helpers import CONFIG, HI, cloudy_frames, synthetic_members, tile_inputs_by_the_builder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


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


BLEND_CASES = [(48, 24, 15), (48, 12, 29), (48, 21, 17), (48, 48, 8), (30, 15, 5), (90, 3, 4)]


@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("window", ["hat", "box"])
@pytest.mark.parametrize("S,hs,n", BLEND_CASES, ids=["S%dh%dn%d" % c for c in BLEND_CASES])
def test_blend_equals_numpy_bit_for_bit(dev, S, hs, n, window, n_images):
    rng = np.random.default_rng(S * 1000 + hs * 10 + n_images)
    sr = synthetic_members(rng, n_images * n * n, S)
    w = TileSpec(1, window).weights(S)
    want = tile_blend_numpy(sr, w, n, hs)
    G = (n - 1) * hs + S
    assert want.shape == (n_images, G, G)
    dsr, dw = torch.from_numpy(sr).to(dev), torch.from_numpy(w).to(dev)
    got = torch.ops.probav.tile_blend(dsr, dw, n_images, n, hs, 0.0, HI)
    _eq_bits(got, want)
    _eq_bits(torch.ops.probav.tile_blend(dsr.unsqueeze(-1), dw, n_images, n, hs, 0.0, HI), want)
    # members that are already clipped and rounded: the same image
    _eq_bits(torch.ops.probav.tile_blend(torch.ops.probav.clip_round(dsr, 0.0, HI), dw, n_images, n, hs, 0.0, HI), want)
    _eq_bits(torch.ops.probav.tile_blend(dsr, dw, n_images, n, hs, -500.0, 4000.0), tile_blend_numpy(sr, w, n, hs, lo=-500.0, hi=4000.0))
    if hs == S:
        assert torch.equal(got, testClass.stitch_device(torch.ops.probav.clip_round(dsr, 0.0, HI).unsqueeze(-1), n_images))
    else:
        assert np.any(want != np.rint(want / 2) * 2) and len(np.unique(want)) > 1000


def test_blend_with_the_largest_window_and_a_random_one(dev):
    rng = np.random.default_rng(8)
    for S, hs, n in ((90, 3, 4), (48, 24, 3), (48, 20, 3)):
        for w in (np.full(S, 1024, np.int32), rng.integers(1, 1025, S).astype(np.int32)):
            sr = synthetic_members(rng, 2 * n * n, S)
            sr[: n * n] = HI
            got = torch.ops.probav.tile_blend(torch.from_numpy(sr).to(dev), torch.from_numpy(w).to(dev), 2, n, hs, 0.0, HI)
            _eq_bits(got, tile_blend_numpy(sr, w, n, hs))
    # an unaligned view of the predictions (the scalar path)
    S, hs, n = 48, 24, 3
    buf = torch.from_numpy(synthetic_members(rng, n * n + 1, S)).to(dev).reshape(-1)
    view = buf[1:1 + n * n * S * S].reshape(n * n, S, S)
    assert view.data_ptr() % 16 != 0
    w = TileSpec(8).weights(S)
    L = _lib.lib()
    out = torch.empty(1, 96, 96, device=dev)
    assert L.probav_tile_blend(_lib.ptr(view), _lib.ptr(torch.from_numpy(w).to(dev)), 1, n, S, hs, 0.0, HI, _lib.ptr(out), _lib.current_stream()) == _lib.PROBAV_OK
    _eq_bits(out, tile_blend_numpy(view.cpu().numpy(), w, n, hs))


def test_blend_refuses_bad_arguments(dev):
    L = _lib.lib()
    S, hs, n = 48, 24, 3
    sr = torch.zeros(n * n, S, S, device=dev)
    w = torch.ones(S, dtype=torch.int32, device=dev)
    out = torch.full((1, 96, 96), -7.0, device=dev)
    P = _lib.ptr
    call = lambda sr_, w_, images, n_, S_, hs_, lo, hi, out_: L.probav_tile_blend(sr_, w_, images, n_, S_, hs_, lo, hi, out_, _lib.current_stream())
    for args in ((P(sr), P(w), 1, 0, S, hs, 0.0, HI, P(out)), (P(sr), P(w), 1, n, 0, hs, 0.0, HI, P(out)), (P(sr), P(w), 1, n, S, 0, 0.0, HI, P(out)),
                 (P(sr), P(w), 1, n, S, S + 1, 0.0, HI, P(out)), (P(sr), P(w), 1, n, S, -3, 0.0, HI, P(out)), (P(sr), P(w), 1, n, S, hs, 1.0, 0.0, P(out)),
                 (P(sr), P(w), 1, n, S, hs, float("nan"), HI, P(out)), (None, P(w), 1, n, S, hs, 0.0, HI, P(out)), (P(sr), None, 1, n, S, hs, 0.0, HI, P(out)),
                 (P(sr), P(w), 1, n, S, hs, 0.0, HI, None), (P(sr), P(w), 0, n, S, hs, 0.0, HI, P(out))):
        assert call(*args) == _lib.PROBAV_EINVAL, args[2:8]
        assert "probav_tile_blend" in L.probav_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                 # nothing was launched
    for bad in ((sr, w, 1, n, 0), (sr, w, 1, n, S + 1), (sr, w, 2, n, hs), (sr, w.long(), 1, n, hs)):
        with pytest.raises(ValueError):
            torch.ops.probav.tile_blend(bad[0], bad[1], bad[2], bad[3], bad[4], 0.0, HI)
    with pytest.raises(ValueError, match="lo"):
        torch.ops.probav.tile_blend(sr, w, 1, n, hs, 2.0, 1.0)
    assert call(P(sr), P(w), 1, n, S, hs, 0.0, HI, P(out)) == _lib.PROBAV_OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


def _frames_parts(frames, stride, config=CONFIG):
    """The tile inputs from parts that exist without the feature: the builder's device unfold copied to the host (prep._patches), its
    pickClearPatchesLR, test.py's transpose -> float32 [images, n n, 22, 22, T, 1]."""
    patches, _ = prep._patches(frames, config["patch_size"] + config["max_shift"], stride, config["max_shift"] // 2)
    return tile_inputs_by_the_builder(patches, config)


def _compose(model, x, spec, n, ensemble=None):
    """The blended images from parts: resolve_device in batches of 16 (or resolve_ensemble(final="round")), then the numpy blend on the host."""
    flat = x.reshape((-1,) + x.shape[2:])
    if ensemble is None:
        members = np.concatenate([testClass.resolve_device(model, flat[i:i + 16]).cpu().numpy() for i in range(0, len(flat), 16)])
    else:
        members = testClass.resolve_ensemble(model, flat, ensemble, final="round").cpu().numpy()
    return tile_blend_numpy(members, spec.weights(48), n, 3 * spec.stride)


@pytest.mark.parametrize("impl", [None, 2, 3], ids=["default", "impl2", "impl3"])
def test_whole_path_equals_its_parts(dev, impl):
    model = _model(dev, impl)
    frames = cloudy_frames()
    for stride, window, images in ((8, "hat", 3), (4, "hat", 1), (8, "box", 1)):
        spec = TileSpec(stride, window)
        n = spec.n(16, 128)
        x = _frames_parts(frames[:images], stride)
        assert x.shape == (images, n * n, 22, 22, 9, 1)
        want = _compose(model, x, spec, n)
        t = tiles.build_tiles(frames[:images], spec, CONFIG, dev)
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == x.shape
        np.testing.assert_array_equal(t.cpu().numpy(), x)             # the device tile builder is the builder's own steps
        got = testClass.resolve_tiled(model, t, spec)
        assert tuple(got.shape) == (images, 384, 384)
        _eq_bits(got, want)
        _eq_bits(testClass.resolve_tiled_frames(model, frames[:images], spec, CONFIG), want)
        assert float(got.min()) >= 0.0 and float(got.max()) <= HI


def test_stride_of_a_whole_patch_is_the_plain_path(dev, tmp_path):
    model = _model(dev)
    frames = cloudy_frames()
    # what prep writes to resolverDir for these frames: stage 3 and stage 4 of prep.main on a directory that holds them
    pre = str(tmp_path / "pre")
    os.makedirs(os.path.join(pre, "trimmedArrayDir"))
    config = dict(CONFIG, raw_data=str(tmp_path / "raw"), preprocessing_out=pre, patch_stride=16, high_res_threshold=0.85, ckpt=[3, 4])
    frames.dump(os.path.join(pre, "trimmedArrayDir", "TESTimgLR_NIR.npy"))
    frames[:1].dump(os.path.join(pre, "trimmedArrayDir", "TRAINimgLR_NIR.npy"))
    np.ma.masked_array(np.zeros((1, 1, 1, 384, 384)), mask=np.zeros((1, 1, 1, 384, 384), bool)).dump(os.path.join(pre, "trimmedArrayDir", "TRAINimgHR_NIR.npy"))
    prep.main(config, "NIR")
    dumped = np.load(os.path.join(pre, "resolverDir", "TESTpatchesLR_NIR.npy"), allow_pickle=True)
    patchLR = np.array(dumped).transpose((0, 1, 4, 5, 2, 3))         # test.py:67
    spec = TileSpec(16)
    t = tiles.build_tiles(frames, spec, CONFIG, dev)
    np.testing.assert_array_equal(t.cpu().numpy(), patchLR)
    plain = testClass.evaluate_device(model, patchLR)
    for window in ("hat", "box"):
        got = testClass.resolve_tiled(model, t, TileSpec(16, window))
        assert tuple(got.shape) == (3, 384, 384)
        for g, p in zip(got.cpu().numpy(), plain):
            np.testing.assert_array_equal(g.astype(np.float64), p[:, :, 0])
    via = testClass.evaluate_device(model, t, tiles=spec)
    assert len(via) == 3
    for a, b in zip(via, plain):
        assert a.shape == b.shape == (384, 384, 1) and a.dtype == b.dtype == np.float64
        np.testing.assert_array_equal(a, b)
    assert torch.equal(testClass.resolve_images(model, t, tiles=spec), testClass.resolve_images(model, patchLR))
    # overlapping tiles are a different image
    assert not torch.equal(testClass.resolve_tiled_frames(model, frames, TileSpec(8), CONFIG), testClass.resolve_images(model, patchLR))


def test_images_do_not_depend_on_launch_sets_or_chunks(dev):
    model = _model(dev)
    frames = cloudy_frames()
    spec = TileSpec(8)
    t = tiles.build_tiles(frames, spec, CONFIG, dev)
    ref = testClass.resolve_tiled(model, t, spec)
    for lb in (64, 225, 2048):
        assert torch.equal(testClass.resolve_tiled(model, t, spec, launch_batch=lb), ref), lb
    per_image = 4 * 225 * 9 * 22 * 22
    for budget in (per_image, 2 * per_image + 5):                    # chunks of one image, and of two and one
        assert tiles.images_per_chunk(spec, CONFIG, 128, 9, budget) == budget // per_image
        assert torch.equal(testClass.resolve_tiled_frames(model, frames, spec, CONFIG, budget=budget, launch_batch=225), ref), budget
    assert torch.equal(testClass.resolve_tiled_frames(model, frames, spec, CONFIG), ref)


def test_ensemble_of_tiles(dev):
    model = _model(dev)
    frames = cloudy_frames()[:1]
    spec, ens = TileSpec(8), EnsembleSpec("d8")
    x = _frames_parts(frames, 8)
    want = _compose(model, x, spec, 15, ensemble=ens)
    t = tiles.build_tiles(frames, spec, CONFIG, dev)
    got = testClass.resolve_tiled(model, t, spec, ensemble=ens)
    _eq_bits(got, want)
    assert torch.equal(testClass.resolve_tiled(model, t, spec, ensemble=ens, launch_batch=100 * ens.V), got)
    assert torch.equal(testClass.resolve_images(model, t, ensemble=ens, tiles=spec), got)
    assert not torch.equal(got, testClass.resolve_tiled(model, t, spec))


def test_opcheck(dev):
    rng = np.random.default_rng(2)
    sr = torch.from_numpy(synthetic_members(rng, 2 * 9, 48)).to(dev)
    w = torch.from_numpy(TileSpec(8).weights(48)).to(dev)
    torch.library.opcheck(torch.ops.probav.tile_blend.default, (sr, w, 2, 3, 24, 0.0, HI))
    torch.library.opcheck(torch.ops.probav.tile_blend.default, (sr.unsqueeze(-1), w, 2, 3, 21, 0.0, HI))


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


def test_cli_tile_stride(dev, tmp_path):
    from probav_amd.pngio import imread_uint16
    from probav_amd.trainClass import ModelTrainer
    d = str(tmp_path)
    res, trm = os.path.join(d, "pre", "resolverDir"), os.path.join(d, "pre", "trimmedArrayDir")
    os.makedirs(res), os.makedirs(trm)
    frames = cloudy_frames()
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d))
    for key in ("TEST", "TRAIN"):
        frames.dump(os.path.join(trm, "%simgLR_NIR.npy" % key))
        np.ma.masked_array(_frames_parts(frames, 16).transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((3, 64, 9, 1, 22, 22), bool)).dump(
            os.path.join(res, "%spatchesLR_NIR.npy" % key), protocol=4)
    rng = np.random.default_rng(4)
    hr = rng.integers(0, 2 ** 14, (4, 1, 1, 384, 384)).astype(np.float64)              # ids 594 .. 597; 595 is removed
    np.ma.masked_array(hr, mask=rng.random(hr.shape) < 0.1).dump(os.path.join(res, "TRAINimgHR_NIR.npy"))
    with open(os.path.join(d, "removedTrainSetsNIR.txt"), "w") as fh:
        fh.write("1307\n1308.0\n595\n")
    model = _model(dev)
    ck = os.path.join(d, "modelInfo", "ckpt_mini", "NIR")
    assert ModelTrainer(model, None, None, None, ck, os.path.join(d, "modelInfo", "logs_mini", "NIR")).save() == "ckpt-1.pt"

    want_tiled = testClass.resolve_tiled_frames(model, frames, TileSpec(8), CONFIG).cpu().numpy()
    want_plain = testClass.evaluate_device(model, _frames_parts(frames, 16))
    names = ["imgset1306.png", "imgset1309.png", "imgset1310.png"]
    for flags, want in ((["--tile-stride", "8"], [w[:, :, None] for w in want_tiled]), ([], want_plain)):
        for f in glob.glob(os.path.join(d, "testout_mini", "*.png")):
            os.remove(f)
        _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR"] + flags, cwd=d)
        pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "testout_mini", "*.png")))
        assert pngs == names, pngs                                   # the same names and omitted ids as the plain run
        for name, w in zip(names, want):
            np.testing.assert_array_equal(imread_uint16(os.path.join(d, "testout_mini", name)), w[:, :, 0].astype(np.uint16))
    assert any(not np.array_equal(a, b[:, :, 0]) for a, b in zip(want_tiled, want_plain))

    out = _run([os.path.join(ROOT, "evaluate.py"), "--cfg", cfg, "--band", "NIR", "--model", "--tile-stride", "8", "--out", os.path.join(d, "scores")], cwd=d)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["tiles"] == {"stride": 8, "window": "hat"} and (line["scored"], line["missing"], line["removed"]) == (3, 0, 3)
    plain = json.loads(_run([os.path.join(ROOT, "evaluate.py"), "--cfg", cfg, "--band", "NIR", "--model", "--out", os.path.join(d, "scores")],
                            cwd=d).stdout.strip().splitlines()[-1])
    assert "tiles" not in plain and set(line) - {"tiles"} == set(plain)
