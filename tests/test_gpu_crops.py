"""Random crops on the device (csrc/kernels_crops.hip, probav_amd/crops.py): each kernel against its numpy statement bit for bit, the crop at the
builder's grid origins against the builder's own unfold and frame choice, the guard against recipe rows that point outside the arrays, and the
trainer fed from CropSpec("grid") against --online-aug on the patches the builder makes from the same scenes."""
import os

import numpy as np
import pytest
import torch

import probav_amd.ops  # noqa: F401  (registers torch.ops.probav.window_counts / crop_batch)
from probav_amd import _lib, crops, prep, synth
from probav_amd.augment import AugmentSpec
from tests.crops_helpers import (SHIPPED_CFG, SMALL_CFG, builder_patches, distinct_scenes, edge_scenes, eligible_counts_distinct,
                                 masked_scene_arrays)

pytestmark = pytest.mark.gpu


def _eq_bits(got, want):
    got = got.cpu().numpy()
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    as_int = {4: np.uint32, 1: np.uint8}[want.dtype.itemsize]
    np.testing.assert_array_equal(got.view(as_int), want.view(as_int))


# ---- window_counts ------------------------------------------------------------------------------------------------------------------------
WC_CASES = [(7, 7, 1, 3, 1), (9, 13, 0, 6, 3), (12, 12, 2, 12, 1), (384, 384, 0, 48, 3)]


@pytest.mark.parametrize("H,W,pad,win,stride", WC_CASES, ids=["h%dw%dp%dk%ds%d" % c for c in WC_CASES])
def test_window_counts_equal_numpy(dev, H, W, pad, win, stride):
    rng = np.random.default_rng(H * 100 + W)
    random = rng.integers(0, 256, (2, H, W)).astype(np.uint8) * (rng.random((2, H, W)) < 0.4)          # nonzero = masked, any nonzero byte
    for name, masks in (("all", np.full((2, H, W), 255, np.uint8)), ("none", np.zeros((2, H, W), np.uint8)), ("random", random.astype(np.uint8))):
        want = crops.window_counts_numpy(masks, pad, win, stride)
        assert want.shape == (2, (H + 2 * pad - win) // stride + 1, (W + 2 * pad - win) // stride + 1)
        got = torch.ops.probav.window_counts(torch.from_numpy(masks).to(dev), pad, win, stride)
        _eq_bits(got, want)
        if name == "all":
            assert (want == win * win).all()
    _eq_bits(torch.ops.probav.window_counts(torch.from_numpy(random != 0).to(dev), pad, win, stride), crops.window_counts_numpy(random, pad, win, stride))


def test_window_counts_refuses_what_it_cannot_do(dev):
    m = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev)
    for pad, win, stride in ((8, 3, 1), (0, 9, 1), (1, 11, 1), (0, 3, 0), (-1, 3, 1)):
        with pytest.raises(ValueError):
            torch.ops.probav.window_counts(m, pad, win, stride)
        out = torch.zeros((1, 8, 8), dtype=torch.int32, device=dev)
        assert _lib.lib().probav_window_counts(_lib.ptr(m), 1, 8, 8, pad, win, stride, _lib.ptr(out), _lib.current_stream()) == _lib.PROBAV_EINVAL
        assert "probav_window_counts" in _lib.lib().probav_last_error().decode()


# ---- crop_batch ---------------------------------------------------------------------------------------------------------------------------
def _rows(rng, positions, k, special):
    """Recipe rows over `positions`: the `special` position indices first, then random ones; all 16 (f, q) codes in turn; identity / reversed /
    random frame orders in turn; one row repeated."""
    n = 20
    r = np.empty((n, 3 + k), np.int32)
    j = list(special) + list(rng.integers(0, len(positions), n))
    for b in range(n):
        r[b, 0], r[b, 1], r[b, 2] = j[b], b % 4, (b // 4) % 4
        r[b, 3:] = (np.arange(k)[::-1], rng.permutation(k), np.arange(k))[b % 3]
    r[n - 1] = r[2]
    return r


def _edge_positions(H, P):
    """{scene, y, x}: both corners of the equal-count, the no-eligible-frame and the E < k scene, odd origins, and the random scene."""
    e = H - P
    return np.array([(0, 0, 0), (0, e, e), (0, 1, 3), (1, 0, 0), (1, e, e), (1, 2, 5), (2, 0, 0), (2, e, e), (2, 3, e - 1), (3, 0, e), (3, e, 0),
                     (3, 1, 1), (3, e // 2, e // 2 + 1), (3, e - 1, 2)], np.int32)


CROP_CASES = [("small", SMALL_CFG, 10, 5), ("t9", SHIPPED_CFG, 128, 9), ("t19", SHIPPED_CFG, 128, 19)]


@pytest.mark.parametrize("name,cfg,H,T_pre", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_crop_batch_equals_numpy(dev, name, cfg, H, T_pre):
    cfg = dict(cfg, num_low_res_imgs_pre=T_pre)
    g = crops.CropGeometry(cfg)
    rng = np.random.default_rng(H + T_pre)
    lr, lr_mask, hr, hr_mask = edge_scenes(cfg, H, seed=3 * H + T_pre)
    hr_clear = ~hr_mask
    pos = _edge_positions(H, g.P)
    rec = _rows(rng, pos, g.k, special=range(len(pos)))
    crops.validate_recipe(rec, len(pos), g.k)
    counts = crops.lr_window_counts_numpy(lr_mask, pos, g)
    assert (counts[3:6] >= g.L).all() and ((counts[6:9] < g.L).sum(1) == 2).all() and 2 < g.k          # no eligible frame; E = 2 < k
    assert (counts[0:3] == 0).all() and len({tuple(x) for x in rec[:, 1:3]}) == 16 and any(x % 2 for x in pos[:, 2])
    want = crops.crop_batch_numpy(lr, lr_mask, hr, hr_clear, pos, rec, g)
    np.testing.assert_array_equal(want[3][0], np.arange(g.k))                                           # equal counts: the frame index decides
    np.testing.assert_array_equal(want[3][6], np.repeat([0, 1], -(-g.k // 2))[:g.k])                    # E = 2: the list is tiled
    dv = [torch.from_numpy(a).to(dev) for a in (lr, lr_mask.view(np.uint8), hr, hr_clear, pos)]
    op = lambda rows, clear=dv[3]: torch.ops.probav.crop_batch(dv[0], dv[1], dv[2], clear, dv[4], torch.from_numpy(np.ascontiguousarray(rows)).to(dev),
                                                               g.P, g.pad, g.win, g.r, g.L)
    whole = op(rec)
    assert whole[2].dtype == torch.bool and tuple(whole[0].shape) == (20, g.win, g.win, g.k, 1) and tuple(whole[1].shape) == (20, g.side, g.side, 1)
    for a, b in zip(whole, want):
        _eq_bits(a, b)
    for lo in range(0, 20, 5):                                                                          # B = 5: the same rows in batches of five
        for a, b in zip(op(rec[lo:lo + 5]), want):
            _eq_bits(a, b[lo:lo + 5])
    for b_ in (0, 7, 19):                                                                               # a row alone equals the row inside a batch
        for a, b in zip(op(rec[b_:b_ + 1]), want):
            _eq_bits(a, b[b_:b_ + 1])
    for a, b in zip(op(rec, dv[3].view(torch.uint8))[:3], want[:2] + (want[2].view(np.uint8),)):         # the clear-mask in its own dtype
        _eq_bits(a, b)


def test_grid_origins_equal_the_builders_patches(dev):
    """probav_prep_patches + the host's clearFrameSelection on the scenes whose eligible counts are pairwise distinct (ties: frame_windows.py)."""
    for cfg, S, H in ((SMALL_CFG, 3, 10), (SHIPPED_CFG, 1, 48)):
        g = crops.CropGeometry(cfg)
        _, (lr, lr_mask, hr, hr_mask) = distinct_scenes(cfg, S, H)
        patches, _, counts = prep.device_patches(lr, lr_mask, g.pad, g.win, g.stride)                   # [S, P, T, win, win], counts [S, P, T]
        n = (H - g.P) // g.stride + 1
        assert patches.shape[1] == n * n and eligible_counts_distinct(counts.reshape(-1, counts.shape[2]), g.L)
        pos = np.array([(s, a * g.stride, c * g.stride) for s in range(S) for a in range(n) for c in range(n)], np.int32)
        rec = np.zeros((len(pos), 3 + g.k), np.int32)
        rec[:, 0], rec[:, 3:] = np.arange(len(pos)), np.arange(g.k)
        got = torch.ops.probav.crop_batch(*(torch.from_numpy(a).to(dev) for a in (lr, lr_mask.view(np.uint8), hr, ~hr_mask, pos, rec)),
                                          g.P, g.pad, g.win, g.r, g.L)
        sel = np.stack([prep.clearFrameSelection(counts[s], g.win ** 2, g.k, g.threshold)[0] for s in range(S)]).reshape(len(pos), g.k)
        _eq_bits(got[3], sel.astype(np.int32))
        flat = patches.reshape(len(pos), *patches.shape[2:])
        _eq_bits(got[0], flat[np.arange(len(pos))[:, None], sel].transpose(0, 2, 3, 1)[..., None])


def test_invalid_rows_leave_their_outputs_untouched(dev):
    """j = V, a code of 4, a permutation entry of k: the row's outputs keep their fill.  `positions` and the scene arrays are allocated with slack,
    so a missing guard shows as changed bytes and can never be an access outside an allocation."""
    cfg, H = SMALL_CFG, 10
    g = crops.CropGeometry(cfg)
    lr, lr_mask, hr, hr_mask = edge_scenes(cfg, H, seed=5)
    S, V, slack = 4, 6, 8
    pos = np.zeros((V + slack, 3), np.int32)
    pos[:V] = _edge_positions(H, g.P)[[0, 4, 8, 9, 11, 12]]
    pad_scenes = lambda a: np.concatenate([a, np.zeros((slack,) + a.shape[1:], a.dtype)])
    dv = [torch.from_numpy(pad_scenes(a)).to(dev) for a in (lr, lr_mask.view(np.uint8), hr, (~hr_mask).view(np.uint8))] + [torch.from_numpy(pos).to(dev)]
    good = np.array([[1, 1, 2, 2, 0, 1]], np.int32)
    rec = np.repeat(good, 5, 0)
    rec[1, 0], rec[2, 1], rec[3, 2], rec[4, 5] = V, 4, 4, g.k
    B = len(rec)
    outs = [torch.full((B, g.win, g.win, g.k), -7.0, device=dev), torch.full((B, g.side, g.side), -7.0, device=dev),
            torch.full((B, g.side, g.side), 9, dtype=torch.uint8, device=dev), torch.full((B, g.k), -5, dtype=torch.int32, device=dev)]
    fill = [o.clone() for o in outs]
    L = _lib.lib()
    rc = L.probav_crop_batch(_lib.ptr(dv[0]), _lib.ptr(dv[1]), _lib.ptr(dv[2]), _lib.ptr(dv[3]), S, g.T_pre, H, g.P, g.pad, g.win, g.r, g.k, g.L,
                             _lib.ptr(dv[4]), V, _lib.ptr(torch.from_numpy(rec).to(dev)), B, *(_lib.ptr(o) for o in outs), _lib.current_stream())
    assert rc == _lib.PROBAV_OK
    torch.cuda.synchronize()
    want = crops.crop_batch_numpy(lr, lr_mask, hr, (~hr_mask).view(np.uint8), pos[:V], good, g)
    for o, f, w in zip(outs, fill, want):
        _eq_bits(o[0], w[0].reshape(o[0].shape))
        for b in range(1, B):
            assert torch.equal(o[b], f[b]), b
    # a position outside the scenes (the list is device data): skipped too
    bad_pos = torch.tensor([[S, 0, 0], [0, H - g.P + 1, 0], [0, 0, H - g.P + 1]], dtype=torch.int32, device=dev)
    rec2 = np.repeat(good, 3, 0)
    rec2[:, 0] = np.arange(3)
    outs2 = [f.clone()[:3] for f in fill]
    rc = L.probav_crop_batch(_lib.ptr(dv[0]), _lib.ptr(dv[1]), _lib.ptr(dv[2]), _lib.ptr(dv[3]), S, g.T_pre, H, g.P, g.pad, g.win, g.r, g.k, g.L,
                             _lib.ptr(bad_pos), 3, _lib.ptr(torch.from_numpy(rec2).to(dev)), 3, *(_lib.ptr(o) for o in outs2), _lib.current_stream())
    assert rc == _lib.PROBAV_OK
    torch.cuda.synchronize()
    for o, f in zip(outs2, fill):
        assert torch.equal(o, f[:3])


def test_geometry_that_does_not_fit_is_refused(dev):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
    # 64 frames of 30 x 30 windows: 230 KB of staged sample
    args = (z(1, 64, 40, 40), z(1, 64, 40, 40, dt=torch.uint8), z(1, 120, 120), z(1, 120, 120, dt=torch.uint8), z(1, 3, dt=torch.int32), z(1, 67, dt=torch.int32))
    with pytest.raises(ValueError, match="LDS"):
        torch.ops.probav.crop_batch(*args, 24, 3, 30, 3, 100)
    outs = (z(1, 30, 30, 64), z(1, 72, 72), z(1, 72, 72, dt=torch.uint8), z(1, 64, dt=torch.int32))
    rc = _lib.lib().probav_crop_batch(*(_lib.ptr(a) for a in args[:4]), 1, 64, 40, 24, 3, 30, 3, 64, 100, _lib.ptr(args[4]), 1, _lib.ptr(args[5]), 1,
                                      *(_lib.ptr(o) for o in outs), _lib.current_stream())
    assert rc == _lib.PROBAV_EINVAL and "LDS" in _lib.lib().probav_last_error().decode()


def test_opcheck(dev):
    cfg, H = SMALL_CFG, 10
    g = crops.CropGeometry(cfg)
    lr, lr_mask, hr, hr_mask = edge_scenes(cfg, H, seed=1, integers=True)            # (opcheck compares values: no NaN bit patterns)
    pos = _edge_positions(H, g.P)
    rec = _rows(np.random.default_rng(0), pos, g.k, range(len(pos)))
    args = tuple(torch.from_numpy(a).to(dev) for a in (lr, lr_mask.view(np.uint8), hr, ~hr_mask, pos, rec)) + (g.P, g.pad, g.win, g.r, g.L)
    torch.library.opcheck(torch.ops.probav.crop_batch.default, args)
    torch.library.opcheck(torch.ops.probav.window_counts.default, (torch.from_numpy(hr_mask.view(np.uint8)).to(dev), 0, g.side, g.r))


# ---- the dataset and the trainer ----------------------------------------------------------------------------------------------------------
def test_dataset_table_lists_and_samplers(dev):
    cfg, H = SMALL_CFG, 10
    g = crops.CropGeometry(cfg)
    lr, lr_mask, hr, hr_mask = edge_scenes(cfg, H, seed=2)
    hr_mask[1] = True                                                                                   # a scene with no valid position
    ds = crops.CropDataset(lr, lr_mask, hr, hr_mask, cfg, dev)
    valid = crops.valid_table_numpy(hr_mask, g)
    assert not valid[1].any() and valid.any()
    _eq_bits(ds.valid, valid)
    _eq_bits(ds.positions, crops.positions_from_table(valid))
    _eq_bits(ds.grid_positions, crops.positions_from_table(valid, g.stride))
    assert len(ds) == int(valid.sum()) and ds.n_grid == len(crops.positions_from_table(valid, g.stride)) and ds.hr_clear.dtype == torch.bool
    aug = AugmentSpec.from_config(cfg, seed=4)
    pos = crops.positions_from_table(valid)
    for rec in crops.random_recipes(len(ds), g.k, aug, crops.CropSpec("all", seed=3), 0, 7, 2):
        got = ds.batch_from_recipe(rec, with_sel=True)
        for a, b in zip(got, crops.crop_batch_numpy(lr, lr_mask, hr, ~hr_mask, pos, rec, g)):
            _eq_bits(a, b)
    bad = np.zeros((1, 3 + g.k), np.int32)
    bad[0, 3:] = np.arange(g.k)
    bad[0, 0] = ds.n_grid
    with pytest.raises(ValueError):
        ds.batch_from_recipe(bad, "grid")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crops.CropDataset(lr, lr_mask, hr, hr_mask, cfg, "cpu")


def _trainer(dev, d, cls):
    from probav_amd.loss import Losses
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.trainClass import make_optimizer
    model = WDSRConv3D("t", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 2, 8, 0.8, 9, 16, True, seed=0).to(dev)
    losses = Losses(targetShape=(48, 48, 1))
    tr = cls(model, losses.shiftCompensatedL1Loss, losses.shiftCompensatedcPSNR, make_optimizer("nadam", model, 5e-4),
             os.path.join(d, "ckpt"), os.path.join(d, "logs"))
    tr.tune_side_stream = False
    return tr


def test_grid_crops_train_like_online_aug_on_the_builders_patches(dev, tmp_path):
    """The same tensors step by step over three epochs of the whole virtual set, and after two real steps (B = 4) the same parameters bit for bit."""
    from probav_amd.trainClass import ModelTrainer
    cfg, S, H = SHIPPED_CFG, 1, 48                                   # 3 x 3 grid patches
    _, (lr, lr_mask, hr, hr_mask) = distinct_scenes(cfg, S, H)
    hr_mask = np.random.default_rng(1).random(hr_mask.shape) < 0.05  # (the helper's HR density suits the small cfg's threshold, not 0.85)
    hr_mask[0, :48, 48:96] = True                                    # one grid patch fails high_res_threshold: 8 base patches
    base_lr, base_hr = builder_patches(*masked_scene_arrays(lr, lr_mask, hr, hr_mask), cfg)
    assert len(base_lr) == 8
    bX, by, bmk = np.array(base_lr), np.array(base_hr), ~np.ma.getmaskarray(base_hr)
    ds = crops.CropDataset(lr, lr_mask, hr, hr_mask, cfg, dev)
    assert ds.n_grid == 8 and len(ds) > 8
    val = [bX, by, bmk]

    class Recording(ModelTrainer):
        def trainStep(self, x, hr_, mk):
            self.__dict__.setdefault("seen", []).append((x.clone(), hr_.clone(), mk.clone()))
            self.trainLoss(torch.zeros(1, device=x.device)), self.trainPSNR(torch.zeros(1, device=x.device))

    spec = AugmentSpec(1, True, True, seed=9)                        # 8 x 2 x 4 x 4 = 256 virtual samples: 16 batches of 16 per epoch
    a, b = _trainer(dev, str(tmp_path / "rec_online"), Recording), _trainer(dev, str(tmp_path / "rec_crops"), Recording)
    a.fitTrainData(bX, [by, bmk], 16, 3, val, bufferSize=32, seed=3, augment=spec)
    b.fitTrainData(None, None, 16, 3, val, bufferSize=32, seed=3, augment=spec, crops=(ds, crops.CropSpec("grid")))
    assert len(a.seen) == len(b.seen) == 48 and a.step == b.step == 48
    for step, ((x1, h1, m1), (x2, h2, m2)) in enumerate(zip(a.seen, b.seen)):
        assert x1.dtype == x2.dtype and h1.dtype == h2.dtype and m1.dtype == m2.dtype and x1.shape == x2.shape, step
        assert torch.equal(x1.view(torch.int32), x2.view(torch.int32)) and torch.equal(h1.view(torch.int32), h2.view(torch.int32)), step
        assert torch.equal(m1, m2), step

    spec2 = AugmentSpec(0, False, False)                             # 8 samples, B = 4: two steps
    flats = []
    for name, kw in (("online", {}), ("crops", {"crops": (ds, crops.CropSpec("grid"))})):
        tr = _trainer(dev, str(tmp_path / name), ModelTrainer)
        args = (None, None) if kw else (bX, [by, bmk])
        tr.fitTrainData(*args, 4, 1, val, bufferSize=32, seed=3, augment=spec2, **kw)
        torch.cuda.synchronize()
        assert tr.step == 2
        flats.append(tr.model.flat.detach().clone())
    assert torch.isfinite(flats[0]).all() and torch.equal(flats[0].view(torch.int32), flats[1].view(torch.int32))
