"""Host side of the random crops (probav_amd/crops.py), no GPU: the numpy statement at grid origins against the dataset builder's own functions, the
window counts against a double loop, the validity rule against pickClearPatches, the samplers, recipe validation, the scene split and the
command-line flags.  The device unfold is replaced by numpy's (tests/tiles_helpers.numpy_unfold)."""
import importlib.util
import os

import numpy as np
import pytest

from probav_amd import augment, crops, prep
from probav_amd.augment import AugmentSpec
from probav_amd.frame_windows import max_masked
from tests.crops_helpers import (SMALL_CFG, builder_patches, distinct_scenes, eligible_counts_distinct, masked_scene_arrays,
                                 numpy_device_patches, scenes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 10


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def numpy_unfold(monkeypatch):
    monkeypatch.setattr(prep, "device_patches", numpy_device_patches)


def test_geometry_of_the_small_scene():
    g = crops.CropGeometry(SMALL_CFG)
    assert (g.P, g.pad, g.win, g.r, g.k, g.T_pre, g.side, g.stride) == (4, 1, 6, 3, 3, 5, 12, 4)
    assert g.L == max_masked(36, 0.5) == 18 and g.L_hr == max_masked(144, 0.6)
    with pytest.raises(ValueError):
        crops.CropGeometry(dict(SMALL_CFG, low_res_patch_thresholds=[0.5, 0.6]))
    with pytest.raises(ValueError):
        crops.CropGeometry(dict(SMALL_CFG, max_shift=3))
    with pytest.raises(ValueError):
        crops.CropSpec("random")


def test_crops_at_grid_origins_equal_the_builders_patches(numpy_unfold):
    """crop_batch_numpy with the identity recipe over the grid list == prep._patches -> pickClearPatchesLR -> pickClearPatches on the same scenes,
    element for element and in order."""
    g = crops.CropGeometry(SMALL_CFG)
    seeds, (lr, lr_mask, hr, hr_mask) = distinct_scenes(SMALL_CFG, 4, H)
    hr_mask[1] = True                                                # a scene without a clear HR patch: removeCorruptedTrainPatchSets drops it
    hr_mask[2, :12, 12:24] = True                                    # one patch of a scene: pickClearPatches drops it
    grid = crops.positions_from_table(np.ones((4, H - g.P + 1, H - g.P + 1), bool), g.stride)
    assert len(grid) == 16
    # the fixture's eligible counts are pairwise distinct per patch: np.argsort's tie order in the builder is unspecified otherwise
    assert eligible_counts_distinct(crops.lr_window_counts_numpy(lr_mask, grid, g), g.L), seeds
    base_lr, base_hr = builder_patches(*masked_scene_arrays(lr, lr_mask, hr, hr_mask), SMALL_CFG)
    pos = crops.positions_from_table(crops.valid_table_numpy(hr_mask, g), g.stride)
    assert 4 < len(pos) == len(base_lr) < 16 and not (pos[:, 0] == 1).any()
    rec = np.zeros((len(pos), 3 + g.k), np.int32)
    rec[:, 0], rec[:, 3:] = np.arange(len(pos)), np.arange(g.k)
    x, y, m, sel = crops.crop_batch_numpy(lr, lr_mask, hr, ~hr_mask, pos, rec, g)
    assert x.dtype == y.dtype == np.float32 and m.dtype == np.bool_ and sel.dtype == np.int32
    np.testing.assert_array_equal(x, np.array(base_lr).astype(np.float32))
    np.testing.assert_array_equal(y, np.array(base_hr).astype(np.float32))
    np.testing.assert_array_equal(m, ~np.ma.getmaskarray(base_hr))
    # prep.gridPatches (what --scene-split runs) is the same composition
    g_lr, g_hr = prep.gridPatches(*masked_scene_arrays(lr, lr_mask, hr, hr_mask), SMALL_CFG)
    np.testing.assert_array_equal(np.array(g_lr), np.array(base_lr))
    np.testing.assert_array_equal(np.ma.getmaskarray(g_hr), np.ma.getmaskarray(base_hr))
    # and with codes: the recipe applied to the builder's patches (what --online-aug does)
    rec2 = augment.make_recipe(np.arange(len(pos) * 48), len(pos), g.k, AugmentSpec(2, True, True, seed=3))
    got = crops.crop_batch_numpy(lr, lr_mask, hr, ~hr_mask, pos, rec2, g)[:3]
    want = augment.apply_recipe_numpy(np.array(base_lr).astype(np.float32), np.array(base_hr).astype(np.float32), ~np.ma.getmaskarray(base_hr), rec2)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_window_counts_numpy_against_a_double_loop():
    rng = np.random.default_rng(0)
    for Hh, W, pad, win, stride in ((7, 7, 1, 3, 1), (9, 13, 0, 6, 3), (12, 12, 2, 12, 1), (10, 8, 3, 5, 2)):
        m = (rng.random((2, Hh, W)) < 0.4) * rng.integers(1, 256, (2, Hh, W))
        p = np.pad(m != 0, ((0, 0), (pad, pad), (pad, pad)), "reflect")
        ny, nx = (Hh + 2 * pad - win) // stride + 1, (W + 2 * pad - win) // stride + 1
        want = np.zeros((2, ny, nx), np.int32)
        for i in range(2):
            for a in range(ny):
                for c in range(nx):
                    want[i, a, c] = p[i, a * stride:a * stride + win, c * stride:c * stride + win].sum()
        got = crops.window_counts_numpy(m, pad, win, stride)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    for bad in ((7, 3, 1), (0, 8, 1), (0, 3, 0)):
        with pytest.raises(ValueError):
            crops.window_counts_numpy(np.zeros((1, 7, 7)), *bad)


def test_validity_rule_is_pick_clear_patches_on_every_count():
    g = crops.CropGeometry(SMALL_CFG)
    px = g.side ** 2
    hr = np.ma.masked_array(np.zeros((px + 1, 1, 1, 1, g.side, g.side)), mask=False)
    for c in range(px + 1):
        hr.mask[c].reshape(-1)[:c] = True
    lr = np.ma.masked_array(np.zeros((px + 1, 1, 2, 1, g.win, g.win)), mask=False)
    kept = prep.pickClearPatches(lr, hr, SMALL_CFG["high_res_threshold"])[1]
    want = np.zeros(px + 1, bool)
    want[:len(kept)] = True                                          # pickClearPatches keeps a prefix of the counts
    assert [int(np.ma.getmaskarray(p).sum()) for p in kept] == list(range(len(kept)))
    np.testing.assert_array_equal(np.arange(px + 1) < g.L_hr, want)
    # and through the table: one scene whose HR window at (0, 0) has exactly c masked pixels
    for c in (g.L_hr - 1, g.L_hr):
        m = np.zeros((1, g.r * H, g.r * H), bool)
        idx = np.unravel_index(np.arange(c), (g.side, g.side))
        m[0][idx] = True
        assert crops.valid_table_numpy(m, g)[0, 0, 0] == (c < g.L_hr)


def test_all_sampler_streams_differ_per_rank_and_repeat_per_seed():
    aug = AugmentSpec(2, True, True)
    draw = lambda seed, rank, a=aug: np.stack(list(crops.random_recipes(1000, 3, a, crops.CropSpec("all", seed=seed), rank, 16, 5)))
    a, b, c, d = draw(1, 0), draw(1, 0), draw(1, 1), draw(2, 0)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c) and not np.array_equal(a, d)
    assert a.shape == (5, 16, 6) and a.dtype == np.int32
    for r in a:
        crops.validate_recipe(r, 1000, 3)
    assert len(np.unique(a[..., 1])) == 4 and len(np.unique(a[..., 2])) == 4 and (a[..., 0].max() > 500)
    plain = draw(1, 0, AugmentSpec(0, False, False))                 # codes are drawn only where the cfg enables them
    assert (plain[..., 1:3] == 0).all() and (plain[..., 3:] == np.arange(3)).all()
    assert crops.steps_per_epoch(64, aug, 32) == 64 * 48 // 32 and crops.steps_per_epoch(64, aug, 32, world=2) == 48
    assert crops.steps_per_epoch(64, aug, 32, crops_per_epoch=1000) == 31


def test_validate_recipe_errors():
    ok = np.array([[4, 3, 3, 2, 0, 1], [0, 0, 0, 0, 1, 2]], np.int32)
    crops.validate_recipe(ok, 5, 3)
    for col, val in ((0, 5), (0, -1), (1, 4), (2, -1), (3, 3), (3, 0)):
        bad = ok.copy()
        bad[0, col] = val
        with pytest.raises(ValueError):
            crops.validate_recipe(bad, 5, 3)
    with pytest.raises(ValueError):
        crops.validate_recipe(ok[:, :5], 5, 3)
    with pytest.raises(ValueError):
        crops.validate_recipe(ok.astype(np.float32), 5, 3)


def test_scene_split_dumps_contain_no_training_scene(numpy_unfold, tmp_path):
    cfg = dict(SMALL_CFG, preprocessing_out=str(tmp_path), raw_data=str(tmp_path / "raw"), ckpt=[5])
    S = 8
    lr, lr_mask, hr, hr_mask = scenes(cfg, S, H, seed=11, integers=True)
    lr += (np.arange(S, dtype=np.float32) * 2 ** 14)[:, None, None, None]          # every value names its scene
    hr += (np.arange(S, dtype=np.float32) * 2 ** 14)[:, None, None]
    d = tmp_path / "trimmedArrayDir"
    d.mkdir()
    lr_m, hr_m = masked_scene_arrays(lr, lr_mask, hr, hr_mask)
    lr_m.dump(str(d / "TRAINimgLR_NIR.npy")), hr_m.dump(str(d / "TRAINimgHR_NIR.npy"))
    prep.main(cfg, "NIR", np.random.RandomState(0), scene_split=True)
    out = tmp_path / "augmentedPatchesDir"
    assert sorted(os.listdir(out)) == ["TRAINVALpatchesHR_NIR.npy", "TRAINVALpatchesLR_NIR.npy", "TRAINscenes_NIR.npy"]
    train = np.load(out / "TRAINscenes_NIR.npy")
    perm = np.random.RandomState(17).permutation(S)
    np.testing.assert_array_equal(train, np.sort(perm[2:]))                        # ceil(0.25 * 8) = 2 validation scenes
    vl = np.load(out / "TRAINVALpatchesLR_NIR.npy", allow_pickle=True)
    vh = np.load(out / "TRAINVALpatchesHR_NIR.npy", allow_pickle=True)
    assert len(vl) == len(vh) > 0 and vl.shape[1:] == (6, 6, 3, 1) and vh.shape[1:] == (12, 12, 1)
    assert set(np.unique(np.ma.getdata(vl) // 2 ** 14)) == set(perm[:2]) == set(np.unique(np.ma.getdata(vh) // 2 ** 14))
    assert not set(train) & set(perm[:2])
    # the loader hands train.py exactly the training scenes
    got = crops.load_scenes(cfg, "NIR", train)
    np.testing.assert_array_equal(got[0], lr[train])
    np.testing.assert_array_equal(got[1], lr_mask[train])
    np.testing.assert_array_equal(got[2], hr[train])
    np.testing.assert_array_equal(got[3], hr_mask[train])


def test_stage5_without_the_flag_is_what_it_was(tmp_path):
    """prep.main's default stage 5 does not read trimmedArrayDir and writes the files it wrote."""
    cfg = dict(SMALL_CFG, preprocessing_out=str(tmp_path), raw_data=str(tmp_path / "raw"), ckpt=[5], num_low_res_permute=1)
    rng = np.random.default_rng(0)
    lr = np.ma.masked_array(rng.random((6, 6, 6, 3, 1)), mask=rng.random((6, 6, 6, 3, 1)) < 0.1)
    hr = np.ma.masked_array(rng.random((6, 12, 12, 1)), mask=rng.random((6, 12, 12, 1)) < 0.1)
    d = tmp_path / "trimmedPatchesDir"
    d.mkdir()
    lr.dump(str(d / "TRAINpatchesLR_NIR.npy")), hr.dump(str(d / "TRAINpatchesHR_NIR.npy"))
    prep.main(cfg, "NIR", np.random.RandomState(0))
    assert sorted(os.listdir(tmp_path / "augmentedPatchesDir")) == ["TRAINVALpatchesHR_NIR.npy", "TRAINVALpatchesLR_NIR.npy", "TRAINpatchesHR_NIR.npy",
                                                                     "TRAINpatchesLR_NIR.npy"]


def test_cli_flag_exclusions(capsys):
    train = _load("train_cli_for_crops", "train.py")
    gen = _load("datagen_cli_for_crops", os.path.join("utils", "dataGenerator.py"))
    o = train.parser(["--random-crops"])
    assert o.random_crops and o.crop_positions == "all" and o.crop_seed == 0 and o.crops_per_epoch is None and not o.online_aug
    o = train.parser(["--random-crops", "--crop-positions", "grid", "--crop-seed", "5"])
    assert o.crop_positions == "grid" and o.crop_seed == 5
    assert train.parser(["--random-crops", "--crops-per-epoch", "4096"]).crops_per_epoch == 4096
    assert not train.parser([]).random_crops
    for bad in (["--random-crops", "--online-aug"], ["--crop-positions", "grid"], ["--crop-seed", "1"], ["--crops-per-epoch", "10"],
                ["--random-crops", "--crop-positions", "grid", "--crops-per-epoch", "10"], ["--random-crops", "--crops-per-epoch", "0"],
                ["--random-crops", "--crop-positions", "some"]):
        with pytest.raises(SystemExit):
            train.parser(bad)
    assert gen.parser(["--scene-split"]).scene_split is True and gen.parser([]).scene_split is False
    with pytest.raises(SystemExit):
        gen.parser(["--scene-split", "--online-aug"])
    capsys.readouterr()


def test_train_py_says_what_random_crops_needs(tmp_path):
    train = _load("train_cli_for_crops2", "train.py")
    with pytest.raises(SystemExit, match="--scene-split"):
        train.training_scenes(str(tmp_path), "NIR")
    np.save(tmp_path / "TRAINscenes_NIR.npy", np.array([0, 2, 3]))
    np.testing.assert_array_equal(train.training_scenes(str(tmp_path), "NIR"), [0, 2, 3])


# ---- the ops, without a device --------------------------------------------------------------------------------------------------------------
def test_ops_on_fake_tensors_and_cpu_tensors():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import probav_amd.ops  # noqa: F401
    with FakeTensorMode():
        out = torch.ops.probav.window_counts(torch.empty(4, 384, 384, dtype=torch.uint8), 0, 48, 3)
        assert tuple(out.shape) == (4, 113, 113) and out.dtype == torch.int32
        assert tuple(torch.ops.probav.window_counts(torch.empty(2, 9, 13, dtype=torch.bool), 0, 6, 3).shape) == (2, 2, 3)
        for bad in ((384, 3, 1), (0, 385, 1), (0, 3, 0)):
            with pytest.raises(ValueError):
                torch.ops.probav.window_counts(torch.empty(4, 384, 384, dtype=torch.uint8), *bad)
        sc = (torch.empty(3, 19, 128, 128), torch.empty(3, 19, 128, 128, dtype=torch.uint8), torch.empty(3, 384, 384), torch.empty(3, 384, 384, dtype=torch.bool))
        pos, rec = torch.empty(50, 3, dtype=torch.int32), torch.empty(5, 12, dtype=torch.int32)
        x, y, m, sel = torch.ops.probav.crop_batch(*sc, pos, rec, 16, 3, 22, 3, 73)
        assert tuple(x.shape) == (5, 22, 22, 9, 1) and tuple(y.shape) == tuple(m.shape) == (5, 48, 48, 1) and tuple(sel.shape) == (5, 9)
        assert x.dtype == y.dtype == torch.float32 and m.dtype == torch.bool and sel.dtype == torch.int32
        for args in ((16, 3, 23, 3, 73), (16, 3, 22, 2, 73), (16, 3, 22, 3, 486), (129, 3, 135, 3, 73), (16, 128, 22, 3, 73)):
            with pytest.raises(ValueError):
                torch.ops.probav.crop_batch(*sc, pos, rec, *args)
        with pytest.raises(ValueError):
            torch.ops.probav.crop_batch(*sc, pos.long(), rec, 16, 3, 22, 3, 73)
    with pytest.raises(NotImplementedError, match="CPU"):            # real CPU tensors: no CPU kernel, the dispatcher refuses
        torch.ops.probav.window_counts(torch.zeros(1, 8, 8, dtype=torch.uint8), 0, 3, 1)
