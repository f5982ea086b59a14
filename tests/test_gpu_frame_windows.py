"""Frame-window ensemble on the device (csrc/kernels_windows.hip, probav_amd/frame_windows.py, testClass.resolve_windowed): the gather and the
reduce kernels against their numpy statements bit for bit, the gather with one window against the tile builder, the whole path against parts
that exist without it (the builder's unfold on the host, the numpy frame choice, resolve_device in batches of 16, the numpy mean and blend),
independence of launch sets and chunks, the ensemble, one window against the tile path, the CLIs.  Every comparison is an equality: after each
member's own rint the arithmetic is integer."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import probav_amd.ops  # noqa: F401  (registers torch.ops.probav.frame_windows_*)
from probav_amd import _lib, prep, testClass, tiles
from probav_amd.ensemble import EnsembleSpec
from probav_amd.frame_windows import (FrameWindowSpec, frame_windows_gather_numpy, frame_windows_reduce_numpy, frame_windows_select_numpy, images_per_chunk,
                                      max_masked)
from probav_amd.tiles import TileSpec, tile_blend_numpy

from tests.frame_windows_helpers import LIMIT_22, THRESHOLD, WCONFIG, distinct_frames, synthetic_counts
from tests.tiles_helpers import CONFIG, HI, cloudy_frames, synthetic_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _model(dev):
    from probav_amd.modelsTF import WDSRConv3D
    return WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)


def _eq_bits(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---- the gather kernel --------------------------------------------------------------------------------------------------------------
GATHER_CASES = [(9, 22, 9, 1, 1), (13, 22, 9, 5, 1), (19, 22, 9, 3, 5), (12, 22, 7, 6, 1), (64, 22, 9, 56, 1), (21, 44, 9, 13, 1), (2, 22, 9, 1, 1),
                (10, 5, 3, 8, 1)]


def _bit_patches(rng, N, T_pre, win):
    """fp32 of random BITS (NaNs with payloads, infinities, denormals among them) plus -0.0, +-inf and two NaNs at fixed places."""
    p = rng.integers(0, 2 ** 32, (N, T_pre, win, win), dtype=np.uint64).astype(np.uint32)
    flat = p.reshape(N, -1)
    flat[:, :5] = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffa5a5a5], np.uint32)
    return p.view(np.float32)


def _counts(N, T_pre, pixels, k, L, seed):
    names, rows = synthetic_counts(T_pre, pixels, k, L)
    assert len(rows) <= 37
    if N == 1:
        return rows[seed % len(rows)][None]
    return rows[np.arange(N) % len(rows)]                            # every synthetic row, some twice


@pytest.mark.parametrize("mode", ["clear", "uniform"])
@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("T_pre,win,k,W,step", GATHER_CASES, ids=["T%dw%dk%dW%ds%d" % c for c in GATHER_CASES])
def test_gather_equals_numpy_bit_for_bit(dev, T_pre, win, k, W, step, N, mode):
    pixels = win * win
    L = max_masked(pixels, THRESHOLD)
    rng = np.random.default_rng(T_pre * 100 + win + N)
    patches = _bit_patches(rng, N, T_pre, win)
    counts = _counts(N, T_pre, pixels, k, L, T_pre + W)
    want_sel, want_w = frame_windows_select_numpy(counts, pixels, k, L, W, step, weights=mode)
    want_x = frame_windows_gather_numpy(patches, want_sel)
    assert want_x.shape == (N, W, win, win, k, 1)
    x, weight, sel = torch.ops.probav.frame_windows_gather(torch.from_numpy(patches).to(dev), torch.from_numpy(counts).to(dev), k, L, W, step, mode)
    assert sel.dtype == torch.int32 and weight.dtype == torch.int32
    np.testing.assert_array_equal(sel.cpu().numpy(), want_sel)
    np.testing.assert_array_equal(weight.cpu().numpy(), want_w)
    _eq_bits(x, want_x)


def test_gather_from_an_unaligned_view(dev):
    T_pre, win, k, W, step, N = 13, 22, 9, 5, 1, 3
    rng = np.random.default_rng(5)
    patches = _bit_patches(rng, N, T_pre, win)
    counts = _counts(37, T_pre, 484, k, LIMIT_22, 0)[4:4 + N]
    buf = torch.zeros(patches.size + 4, device=dev)
    view = buf[1:1 + patches.size].view(N, T_pre, win, win)
    view.copy_(torch.from_numpy(patches))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()        # the scalar staging path
    want_sel, want_w = frame_windows_select_numpy(counts, 484, k, LIMIT_22, W, step)
    x, weight, sel = torch.ops.probav.frame_windows_gather(view, torch.from_numpy(counts).to(dev), k, LIMIT_22, W, step, "clear")
    np.testing.assert_array_equal(sel.cpu().numpy(), want_sel)
    np.testing.assert_array_equal(weight.cpu().numpy(), want_w)
    _eq_bits(x, frame_windows_gather_numpy(patches, want_sel))


def _device_unfold(frames, stride):
    S_, T, _, H, _ = frames.shape
    pt, _, pc = prep._device_patches(np.ma.getdata(frames).reshape(S_, T, H, H), np.ma.getmaskarray(frames).reshape(S_, T, H, H), 3, 22, stride)
    return pt, pc


@pytest.mark.parametrize("which", ["cloudy", "distinct"])
def test_one_window_on_the_real_unfold_is_the_tile_builders_choice(dev, which):
    frames = cloudy_frames(images=2, T=9, H=64) if which == "cloudy" else distinct_frames()
    pt, pc = _device_unfold(frames, 16)
    assert tuple(pt.shape) == (2, 16, 9, 22, 22)
    x, weight, sel = torch.ops.probav.frame_windows_gather(pt.reshape(32, 9, 22, 22), pc.reshape(32, 9), 9, LIMIT_22, 1, 1, "uniform")
    counts = pc.reshape(32, 9).cpu().numpy()
    choice = tiles.select_frames(counts[None], 484, 9, [THRESHOLD])[0]
    rows = np.arange(32)[:, None]
    np.testing.assert_array_equal(counts[rows, sel.cpu().numpy()[:, 0]], counts[rows, choice])      # the count sequence of every tile
    assert bool((weight == 1).all())
    built = tiles.build_tiles(frames, TileSpec(16), CONFIG, dev).reshape(32, 22, 22, 9, 1)
    elig = counts < LIMIT_22
    distinct = [n for n in range(32) if elig[n].sum() > 1 and len(set(counts[n][elig[n]].tolist())) == elig[n].sum()]
    if which == "cloudy":
        # with this seed no tile of the cloudy frames has pairwise distinct eligible counts (its clear frames tie at 0 masked pixels), so the
        # element-for-element comparison is made on the synthetic distinct-count frames, the other case of this test
        same = [n for n in range(32) if np.array_equal(sel.cpu().numpy()[n, 0], choice[n])]
        assert torch.equal(x[same, 0], built[same])
    else:
        assert len(distinct) == 32                                   # at least one such tile: here, all of them
        assert torch.equal(x[:, 0], built)


# ---- the reduce kernel --------------------------------------------------------------------------------------------------------------
def _weights(rng, N, W, kind):
    if kind == "zeros":
        w = rng.integers(0, 4357, (N, W)) * rng.integers(0, 2, (N, W))
    elif kind == "largest":
        w = np.full((N, W), 9 * 1936)
    else:
        w = rng.integers(0, 9 * 1936 + 1, (N, W))
    w[np.arange(N), rng.integers(0, W, N)] += 1                      # a positive sum per tile
    return w.astype(np.int32)


@pytest.mark.parametrize("N", [1, 19])
@pytest.mark.parametrize("W", [1, 2, 5, 64])
@pytest.mark.parametrize("S", [48, 30, 90])
def test_reduce_equals_numpy_bit_for_bit(dev, S, W, N):
    rng = np.random.default_rng(S * 100 + W + N)
    sr = synthetic_members(rng, N * W, S)
    dsr = torch.from_numpy(sr).to(dev)
    for kind in ("zeros", "largest", "random"):
        w = _weights(rng, N, W, kind)
        dw = torch.from_numpy(w).to(dev)
        want = frame_windows_reduce_numpy(sr, w)
        got = torch.ops.probav.frame_windows_reduce(dsr, dw, 0.0, HI)
        assert tuple(got.shape) == (N, S, S)
        _eq_bits(got, want)
    _eq_bits(torch.ops.probav.frame_windows_reduce(dsr.unsqueeze(-1), dw, 0.0, HI), want)                     # the [.., 1] member layout
    _eq_bits(torch.ops.probav.frame_windows_reduce(torch.ops.probav.clip_round(dsr, 0.0, HI), dw, 0.0, HI), want)
    _eq_bits(torch.ops.probav.frame_windows_reduce(dsr, dw, -500.0, 4000.0), frame_windows_reduce_numpy(sr, w, lo=-500.0, hi=4000.0))
    if W == 1:
        assert torch.equal(got, torch.ops.probav.clip_round(dsr, 0.0, HI))                                    # the identity on rounded members


def test_reduce_from_an_unaligned_view(dev):
    rng = np.random.default_rng(9)
    N, W, S = 3, 5, 48
    sr = synthetic_members(rng, N * W, S)
    w = _weights(rng, N, W, "random")
    buf = torch.zeros(sr.size + 4, device=dev)
    view = buf[1:1 + sr.size].view(N * W, S, S)
    view.copy_(torch.from_numpy(sr))
    assert view.data_ptr() % 16 != 0
    _eq_bits(torch.ops.probav.frame_windows_reduce(view, torch.from_numpy(w).to(dev), 0.0, HI), frame_windows_reduce_numpy(sr, w))


# ---- the C entry points refuse bad arguments ----------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(dev):
    L = _lib.lib()
    P = _lib.ptr
    N, T, win, k, W, step, lim = 4, 13, 22, 9, 3, 2, LIMIT_22
    patches = torch.zeros(N, T, win, win, device=dev)
    counts = torch.zeros(N, T, dtype=torch.int32, device=dev)
    x = torch.full((N, W, win, win, k, 1), -7.0, device=dev)
    weight = torch.full((N, W), -7, dtype=torch.int32, device=dev)
    sel = torch.full((N, W, k), -7, dtype=torch.int32, device=dev)
    gather = lambda pt, pc, N_, T_, win_, k_, L_, W_, step_, mode, x_, w_, s_: L.probav_frame_windows_gather(pt, pc, N_, T_, win_, k_, L_, W_, step_, mode,
                                                                                                           x_, w_, s_, _lib.current_stream())
    good = (P(patches), P(counts), N, T, win, k, lim, W, step, 0, P(x), P(weight), P(sel))
    bad = []
    for i in (0, 1, 10, 11, 12):                                     # null pointers
        bad.append(good[:i] + (None,) + good[i + 1:])
    for i, v in ((2, 0), (2, -1), (7, 0), (7, 65), (5, 0), (5, -3), (3, 0), (3, 65), (7, 4),    # N, W, k, T_pre; (W - 1) step + k = 15 > 13
                 (8, 3), (8, 0), (6, -1), (6, win * win + 2), (9, 2), (9, -1)):                   # step 3: 6 + 9 > 13; step 0; L; mode
        bad.append(good[:i] + (v,) + good[i + 1:])
    bad.append(good[:3] + (22, 44) + good[5:])                       # 22 frames of 44 x 44: 42 592 floats do not fit 160 KiB of LDS (a host check)
    for args in bad:
        assert gather(*args) == _lib.PROBAV_EINVAL, args[2:10]
        assert "probav_frame_windows_gather" in L.probav_last_error().decode()
    assert "LDS" in L.probav_last_error().decode()

    S = 48
    sr = torch.zeros(N * W, S, S, device=dev)
    rw = torch.ones(N, W, dtype=torch.int32, device=dev)
    out = torch.full((N, S, S), -7.0, device=dev)
    reduce_ = lambda sr_, w_, N_, W_, S_, lo, hi, out_: L.probav_frame_windows_reduce(sr_, w_, N_, W_, S_, lo, hi, out_, _lib.current_stream())
    for args in ((None, P(rw), N, W, S, 0.0, HI, P(out)), (P(sr), None, N, W, S, 0.0, HI, P(out)), (P(sr), P(rw), N, W, S, 0.0, HI, None),
                 (P(sr), P(rw), 0, W, S, 0.0, HI, P(out)), (P(sr), P(rw), -2, W, S, 0.0, HI, P(out)), (P(sr), P(rw), N, 0, S, 0.0, HI, P(out)),
                 (P(sr), P(rw), N, 65, S, 0.0, HI, P(out)), (P(sr), P(rw), N, W, 0, 0.0, HI, P(out)), (P(sr), P(rw), N, W, S, 1.0, 0.0, P(out)),
                 (P(sr), P(rw), N, W, S, float("nan"), HI, P(out)), (P(sr), P(rw), N, W, S, 0.0, float("nan"), P(out))):
        assert reduce_(*args) == _lib.PROBAV_EINVAL, args[2:7]
        assert "probav_frame_windows_reduce" in L.probav_last_error().decode()
    torch.cuda.synchronize()
    assert bool((x == -7.0).all()) and bool((weight == -7).all()) and bool((sel == -7).all()) and bool((out == -7.0).all())      # nothing was launched
    with pytest.raises(ValueError, match="LDS"):
        torch.ops.probav.frame_windows_gather(torch.zeros(1, 22, 44, 44, device=dev), torch.zeros(1, 22, dtype=torch.int32, device=dev), 9, 291, 2, 1, "clear")
    # then one good call of each succeeds
    assert gather(*good) == _lib.PROBAV_OK
    assert reduce_(P(sr), P(rw), N, W, S, 0.0, HI, P(out)) == _lib.PROBAV_OK
    torch.cuda.synchronize()
    assert bool((x == 0.0).all()) and bool((weight == k * win * win).all()) and bool((out == 0.0).all())
    assert sel[0].cpu().tolist() == [[j * step + i for i in range(k)] for j in range(W)]      # all counts 0: frames in index order


def test_opcheck(dev):
    rng = np.random.default_rng(2)
    patches = torch.from_numpy(rng.standard_normal((5, 13, 22, 22)).astype(np.float32)).to(dev)
    counts = torch.from_numpy(_counts(5, 13, 484, 9, LIMIT_22, 0)).to(dev)
    torch.library.opcheck(torch.ops.probav.frame_windows_gather.default, (patches, counts, 9, LIMIT_22, 3, 2, "clear"))
    sr = torch.from_numpy(synthetic_members(rng, 6, 48)).to(dev)
    w = torch.from_numpy(_weights(rng, 2, 3, "random")).to(dev)
    torch.library.opcheck(torch.ops.probav.frame_windows_reduce.default, (sr, w, 0.0, HI))
    torch.library.opcheck(torch.ops.probav.frame_windows_reduce.default, (sr.unsqueeze(-1), w, 0.0, HI))


# ---- the whole path -----------------------------------------------------------------------------------------------------------------
def _compose(model, frames, wspec, tspec, config, ensemble=None):
    """The images from parts that exist without the feature: the builder's unfold copied to the host (prep._patches), the numpy frame
    choice and gather, resolve_device in batches of 16 (or resolve_ensemble(final="round")), the numpy mean, the numpy blend."""
    patches, counts = prep._patches(frames, 22, tspec.stride, 3)
    S_, Pn, T = counts.shape
    pt = np.ma.getdata(patches).reshape(S_ * Pn, T, 22, 22)
    L = max_masked(484, config["low_res_patch_thresholds"][0])
    sel, weight = frame_windows_select_numpy(counts.reshape(S_ * Pn, T), 484, config["num_low_res_imgs"], L, wspec.windows, wspec.step, wspec.weights)
    x = frame_windows_gather_numpy(pt, sel)
    flat = x.reshape((-1,) + x.shape[2:])
    if ensemble is None:
        members = np.concatenate([testClass.resolve_device(model, flat[i:i + 16]).cpu().numpy() for i in range(0, len(flat), 16)])
    else:
        members = testClass.resolve_ensemble(model, flat, ensemble, final="round").cpu().numpy()
    per_tile = frame_windows_reduce_numpy(members, weight)
    n = int(round(Pn ** 0.5))
    return tile_blend_numpy(per_tile, tspec.weights(48), n, 3 * tspec.stride)


@pytest.fixture(scope="module")
def frames13():
    return cloudy_frames(images=2, T=13, H=64)


def test_whole_path_equals_its_parts(dev, frames13):
    model = _model(dev)
    wspec = FrameWindowSpec(3, 2)
    want = _compose(model, frames13, wspec, TileSpec(16, "box"), WCONFIG)
    assert want.shape == (2, 192, 192)
    got = testClass.resolve_windowed_frames(model, frames13, wspec, WCONFIG)
    _eq_bits(got, want)
    assert float(got.min()) >= 0.0 and float(got.max()) <= HI
    # independent of the launch sets and of the chunks
    assert torch.equal(testClass.resolve_windowed_frames(model, frames13, wspec, WCONFIG, launch_batch=16), got)
    per_image = 4 * 16 * max(13 * 484, 3 * 9 * 484, 3 * 48 * 48)
    assert images_per_chunk(wspec, TileSpec(16, "box"), WCONFIG, 64, 13, per_image) == 1 and images_per_chunk(wspec, TileSpec(16, "box"), WCONFIG, 64, 13) > 2
    assert torch.equal(testClass.resolve_windowed_frames(model, frames13, wspec, WCONFIG, budget=per_image), got)
    via = testClass.evaluate_device(model, frames13, windows=wspec, config=WCONFIG)
    assert len(via) == 2 and via[0].shape == (192, 192, 1) and via[0].dtype == np.float64
    np.testing.assert_array_equal(np.stack(via)[..., 0], want.astype(np.float64))
    # the windows show the network other frames: not the one-window image, and uniform weights are another mean
    assert not torch.equal(got, testClass.resolve_windowed_frames(model, frames13, FrameWindowSpec(1), WCONFIG))
    uni = FrameWindowSpec(3, 2, "uniform")
    _eq_bits(testClass.resolve_windowed_frames(model, frames13, uni, WCONFIG), _compose(model, frames13, uni, TileSpec(16, "box"), WCONFIG))


def test_whole_path_with_overlapping_tiles(dev, frames13):
    model = _model(dev)
    wspec, tspec = FrameWindowSpec(3, 2), TileSpec(8)
    want = _compose(model, frames13[:1], wspec, tspec, WCONFIG)
    _eq_bits(testClass.resolve_windowed_frames(model, frames13[:1], wspec, WCONFIG, tiles=tspec), want)


def test_whole_path_with_the_self_ensemble(dev, frames13):
    model = _model(dev)
    wspec, ens = FrameWindowSpec(2, 2), EnsembleSpec("d8")
    want = _compose(model, frames13[:1], wspec, TileSpec(16, "box"), WCONFIG, ensemble=ens)
    got = testClass.resolve_windowed_frames(model, frames13[:1], wspec, WCONFIG, ensemble=ens)
    _eq_bits(got, want)
    assert torch.equal(testClass.resolve_windowed_frames(model, frames13[:1], wspec, WCONFIG, ensemble=ens, launch_batch=5 * ens.V), got)
    assert not torch.equal(got, testClass.resolve_windowed_frames(model, frames13[:1], wspec, WCONFIG))


def test_one_uniform_window_is_the_tile_path(dev):
    model = _model(dev)
    frames = distinct_frames()                                       # no ties in any tile: the builder's frame choice is determined
    for tspec in (TileSpec(16, "box"), TileSpec(8)):
        want = testClass.resolve_tiled_frames(model, frames, tspec, CONFIG)
        got = testClass.resolve_windowed_frames(model, frames, FrameWindowSpec(1, 1, "uniform"), CONFIG, tiles=tspec)
        assert tuple(got.shape) == (2, 192, 192) and torch.equal(got, want)
        assert torch.equal(testClass.resolve_windowed_frames(model, frames, FrameWindowSpec(1), CONFIG, tiles=tspec), want)      # one window: any weight


# ---- the CLIs -----------------------------------------------------------------------------------------------------------------------
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
num_low_res_imgs_pre=13
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


def test_cli_frame_windows(dev, tmp_path):
    from probav_amd import scoring
    from probav_amd.parseConfig import parseConfig
    from probav_amd.pngio import imread_uint16
    from probav_amd.trainClass import ModelTrainer
    d = str(tmp_path)
    res, trm = os.path.join(d, "pre", "resolverDir"), os.path.join(d, "pre", "trimmedArrayDir")
    os.makedirs(res), os.makedirs(trm)
    frames = cloudy_frames(images=3, T=13)
    cfg = os.path.join(d, "mini.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(d=d))
    for key in ("TEST", "TRAIN"):
        frames.dump(os.path.join(trm, "%simgLR_NIR.npy" % key))
    rng = np.random.default_rng(4)
    hr = rng.integers(0, 2 ** 14, (4, 1, 1, 384, 384)).astype(np.float64)              # ids 594 .. 597; 595 is removed
    np.ma.masked_array(hr, mask=rng.random(hr.shape) < 0.1).dump(os.path.join(res, "TRAINimgHR_NIR.npy"))
    with open(os.path.join(d, "removedTrainSetsNIR.txt"), "w") as fh:
        fh.write("1307\n1308.0\n595\n")
    model = _model(dev)
    ck = os.path.join(d, "modelInfo", "ckpt_mini", "NIR")
    assert ModelTrainer(model, None, None, None, ck, os.path.join(d, "modelInfo", "logs_mini", "NIR")).save() == "ckpt-1.pt"
    config = parseConfig(cfg)

    want = testClass.evaluate_windowed_frames(model, frames, FrameWindowSpec(3, 2), config)
    _run([os.path.join(ROOT, "test.py"), "--cfg", cfg, "--band", "NIR", "--frame-windows", "3", "--frame-window-step", "2"], cwd=d)
    names = ["imgset1306.png", "imgset1309.png", "imgset1310.png"]
    pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "testout_mini", "*.png")))
    assert pngs == names, pngs                                       # the names and omitted ids of the plain run
    for name, w in zip(names, want):
        np.testing.assert_array_equal(imread_uint16(os.path.join(d, "testout_mini", name)), w[:, :, 0].astype(np.uint16))

    out = _run([os.path.join(ROOT, "evaluate.py"), "--cfg", cfg, "--band", "NIR", "--model", "--frame-windows", "3", "--out", os.path.join(d, "scores")], cwd=d)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["frame_windows"] == {"windows": 3, "step": 1, "weights": "clear"} and (line["scored"], line["missing"], line["removed"]) == (3, 0, 3)
    direct = testClass.evaluate_windowed_frames(model, frames, FrameWindowSpec(3), config)
    images = {i: img[:, :, 0].astype(np.uint16) for i, img in zip((594, 596, 597), direct)}
    rows, _ = scoring.score_images(images, {"NIR": scoring.load_hr(config, "NIR")}, removed={"NIR": {595}})
    assert line["overall"]["mean_cpsnr"] == float(np.mean([r["cpsnr"] for r in rows]))
