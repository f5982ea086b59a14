"""Host side of the online augmentation (probav_amd/augment.py), no GPU: the virtual data set decoded element by element equals what the
builder's three augmentation functions materialise; stage 5 with online_aug saves what the normal run applies; recipes are validated
before anything is launched; and the trainer walks the same index stream over the virtual set as over the materialised arrays."""
import os

import numpy as np
import pytest
import torch

from probav_amd import augment, prep
from probav_amd.augment import AugmentSpec, apply_recipe_numpy, decode, make_recipe, validate_recipe
from probav_amd.modelsTF import WDSRModel
from probav_amd.trainClass import ModelTrainer, shuffle_repeat_batch


def _base(n, H=6, T=9, S=9, seed=1, C=1):
    r = np.random.RandomState(seed)
    lr = np.ma.masked_array(r.rand(n, H, H, T, C).astype(np.float32), mask=r.rand(n, H, H, T, C) > 0.5)
    hr = np.ma.masked_array(r.rand(n, S, S, 1).astype(np.float32), mask=r.rand(n, S, S, 1) > 0.5)
    return lr, hr


def _materialise(lr, hr, numPermute, flip, rotate, rng):
    """Stage 5 of prep.main, restated with the builder's own functions."""
    a = prep.augmentByShufflingLRImgs(lr, numPermute=numPermute, rng=rng)
    h = np.tile(hr, (numPermute + 1, 1, 1, 1))
    if flip:
        a, h = prep.augmentByFlipping(a), prep.augmentByFlipping(h)
    if rotate:
        a, h = prep.augmentByRotating(a), prep.augmentByRotating(h)
    return a, h


def _expand(lr, hr, spec):
    """decode + the numpy statement of a recipe over the whole virtual set: (LR data, LR mask, HR data, HR mask)."""
    N, T = len(lr), lr.shape[3]
    rec = make_recipe(np.arange(N * spec.multiplicity), N, T, spec)
    validate_recipe(rec, N, T)
    d, hd, hm = apply_recipe_numpy(np.ma.getdata(lr), np.ma.getdata(hr), np.ma.getmaskarray(hr), rec)
    m = apply_recipe_numpy(np.ma.getmaskarray(lr), np.ma.getdata(hr), np.ma.getmaskarray(hr), rec)[0]
    return d, m, hd, hm


@pytest.mark.parametrize("numPermute", [0, 3, 19])
@pytest.mark.parametrize("flip,rotate", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_virtual_set_equals_the_materialised_one(numPermute, flip, rotate):
    lr, hr = _base(5)
    a, h = _materialise(lr, hr, numPermute, flip, rotate, np.random.RandomState(3))
    spec = AugmentSpec(numPermute, flip, rotate, seed=3)
    assert spec.multiplicity == (numPermute + 1) * (4 if flip else 1) * (4 if rotate else 1) == len(a) // len(lr)
    d, m, hd, hm = _expand(lr, hr, spec)
    np.testing.assert_array_equal(spec.table(9)[0], np.arange(9))
    assert spec.table(9).shape == (numPermute + 1, 9)
    for got, want in ((d, np.ma.getdata(a)), (m, np.ma.getmaskarray(a)), (hd, np.ma.getdata(h)), (hm, np.ma.getmaskarray(h))):
        assert got.shape == want.shape and got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    # decode alone, on scattered indices
    v = np.array([0, len(a) - 1, len(lr), 7 % len(a)])
    i, p, f, k = decode(v, len(lr), spec)
    assert i.tolist() == (v % 5).tolist() and p.max() <= numPermute and f.max() <= (3 if flip else 0) and k.max() <= (3 if rotate else 0)


def test_a_given_table_is_used_and_checked():
    lr, hr = _base(4, T=4)
    perms = augment.draw_perms(2, 4, np.random.RandomState(11))
    a, h = _materialise(lr, hr, 2, 1, 1, np.random.RandomState(11))
    spec = AugmentSpec.from_config({"num_low_res_permute": 2, "to_flip": 1, "to_rotate": 1}, perms)
    d, m, hd, hm = _expand(lr, hr, spec)
    np.testing.assert_array_equal(d, np.ma.getdata(a))
    np.testing.assert_array_equal(hm, np.ma.getmaskarray(h))
    with pytest.raises(ValueError):
        AugmentSpec(2, 1, 1, perms=perms[:2])                      # one row short
    with pytest.raises(ValueError):
        AugmentSpec(2, 1, 1, perms=np.array([[0, 1, 2, 3], [0, 0, 2, 3], [3, 2, 1, 0]]))
    with pytest.raises(ValueError):
        AugmentSpec(2, 1, 1, perms=perms[::-1])                    # the identity is not first
    with pytest.raises(ValueError):
        spec.table(9)                                              # a table for 4 frames, data with 9
    fresh = AugmentSpec(2, 1, 1, perms=perms, seed=5, permute="fresh")
    rec = make_recipe(np.arange(4 * fresh.multiplicity), 4, 4, fresh)
    validate_recipe(rec, 4, 4)
    assert len({tuple(r) for r in rec[:, 3:]}) > 3                 # more orders than the table's three rows
    np.testing.assert_array_equal(rec[:, :3], make_recipe(np.arange(4 * spec.multiplicity), 4, 4, spec)[:, :3])


def _stage5(tmp_path, name, lr, hr, online_aug, cfg):
    out = tmp_path / name
    os.makedirs(out / "trimmedPatchesDir")
    lr.dump(str(out / "trimmedPatchesDir" / "TRAINpatchesLR_NIR.npy"), protocol=4)
    hr.dump(str(out / "trimmedPatchesDir" / "TRAINpatchesHR_NIR.npy"), protocol=4)
    config = dict(cfg, raw_data=str(tmp_path / "raw"), preprocessing_out=str(out), ckpt=[5])
    if online_aug:
        prep.main(config, "NIR", np.random.RandomState(4), online_aug=True)
    else:
        prep.main(config, "NIR", np.random.RandomState(4))
    return out / "augmentedPatchesDir"


@pytest.mark.parametrize("numPermute,flip,rotate", [(3, 1, 1), (2, 0, 1), (0, 0, 0)])
def test_builder_stage5_saves_what_the_normal_run_applies(tmp_path, numPermute, flip, rotate):
    lr, hr = _base(23, seed=9)
    cfg = {"split": 0.2, "num_low_res_permute": numPermute, "to_flip": flip, "to_rotate": rotate}
    normal = _stage5(tmp_path, "normal", lr, hr, False, cfg)
    online = _stage5(tmp_path, "online", lr, hr, True, cfg)
    for n in ("TRAINVALpatchesLR_NIR.npy", "TRAINVALpatchesHR_NIR.npy"):
        assert open(normal / n, "rb").read() == open(online / n, "rb").read(), n
    assert sorted(os.listdir(normal)) == ["TRAINVALpatchesHR_NIR.npy", "TRAINVALpatchesLR_NIR.npy", "TRAINpatchesHR_NIR.npy", "TRAINpatchesLR_NIR.npy"]
    assert sorted(os.listdir(online)) == ["TRAINVALpatchesHR_NIR.npy", "TRAINVALpatchesLR_NIR.npy", "TRAINaugperms_NIR.npy", "TRAINbasepatchesHR_NIR.npy",
                                          "TRAINbasepatchesLR_NIR.npy"]
    load = lambda d, n: np.load(d / n, allow_pickle=True)
    a, h = load(normal, "TRAINpatchesLR_NIR.npy"), load(normal, "TRAINpatchesHR_NIR.npy")
    blr, bhr, perms = load(online, "TRAINbasepatchesLR_NIR.npy"), load(online, "TRAINbasepatchesHR_NIR.npy"), load(online, "TRAINaugperms_NIR.npy")
    assert perms.shape == (numPermute + 1, 9) and len(blr) == 23 - 5
    d, m, hd, hm = _expand(blr, bhr, AugmentSpec.from_config(cfg, perms))
    for got, want in ((d, np.ma.getdata(a)), (m, np.ma.getmaskarray(a)), (hd, np.ma.getdata(h)), (hm, np.ma.getmaskarray(h))):
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)
    from utils import dataGenerator
    assert dataGenerator.parser(["--online-aug"]).online_aug is True and dataGenerator.parser([]).online_aug is False


def test_recipes_are_validated_on_the_host():
    spec = AugmentSpec(3, 1, 1, seed=0)
    N, T = 5, 9
    V = N * spec.multiplicity
    good = make_recipe(np.arange(V), N, T, spec)
    validate_recipe(good, N, T)
    for bad_v in ([V], [-1], [0, V + 3]):
        with pytest.raises(ValueError, match="out of range"):
            make_recipe(bad_v, N, T, spec)
    for col, val in ((0, N), (0, -1), (1, 4), (2, 4), (2, -1), (3, T), (4, 0 if good[0, 4] != 0 else 1)):
        r = good[:8].copy()
        r[5, col] = val
        if col == 4:                                               # a repeated frame: entries in range, not a permutation
            r[5, 3:] = good[5, 3:]
            r[5, 4] = r[5, 3]
        with pytest.raises(ValueError):
            validate_recipe(r, N, T)
    with pytest.raises(ValueError):
        validate_recipe(good[:, :-1], N, T)
    # non-square patches, wrong ranks, a CPU device
    X, y, mk = np.zeros((3, 6, 6, 9, 1), np.float32), np.zeros((3, 9, 9, 1), np.float32), np.ones((3, 9, 9, 1), bool)
    augment.DeviceDataset._host_arrays(X, y, mk)
    with pytest.raises(ValueError, match="square"):
        augment.DeviceDataset._host_arrays(np.zeros((3, 6, 5, 9, 1), np.float32), y, mk)
    with pytest.raises(ValueError, match="square"):
        augment.DeviceDataset._host_arrays(X, np.zeros((3, 9, 8, 1), np.float32), np.ones((3, 9, 8, 1), bool))
    with pytest.raises(ValueError):
        augment.DeviceDataset._host_arrays(X, y, mk.astype(np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment.DeviceDataset(X, y, mk, "cpu")


def test_op_traces_on_fake_tensors(built_lib):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import probav_amd.ops  # noqa: F401
    schema = str(torch.ops.probav.augment_batch.default._schema)
    assert schema.endswith("(Tensor lr, Tensor hr, Tensor mask, Tensor recipe) -> (Tensor, Tensor, Tensor)"), schema
    with FakeTensorMode():
        for mdt in (torch.bool, torch.uint8):
            lr, hr = torch.empty(7, 22, 22, 13, 1), torch.empty(7, 48, 48, 1)
            mask, rec = torch.empty(7, 48, 48, 1, dtype=mdt), torch.empty(128, 16, dtype=torch.int32)
            a, b, c = torch.ops.probav.augment_batch(lr, hr, mask, rec)
            assert a.shape == (128, 22, 22, 13, 1) and b.shape == c.shape == (128, 48, 48, 1)
            assert (a.dtype, b.dtype, c.dtype) == (torch.float32, torch.float32, mdt)
        for bad in ((torch.empty(7, 22, 21, 13, 1), hr, mask, rec), (lr, torch.empty(7, 48, 47, 1), torch.empty(7, 48, 47, 1, dtype=torch.bool), rec),
                    (lr, hr, mask, torch.empty(128, 12, dtype=torch.int32)), (lr, hr, mask, torch.empty(128, 16, dtype=torch.int64)),
                    (lr.double(), hr, mask, rec)):
            with pytest.raises(ValueError):
                torch.ops.probav.augment_batch(*bad)
    with pytest.raises(NotImplementedError, match="CPU"):            # real CPU tensors: the op has no CPU kernel, the dispatcher refuses
        torch.ops.probav.augment_batch(torch.zeros(2, 6, 6, 4, 1), torch.zeros(2, 9, 9, 1), torch.ones(2, 9, 9, 1, dtype=torch.bool),
                                       torch.zeros(1, 7, dtype=torch.int32))


@pytest.mark.parametrize("world", [1, 2])
def test_index_stream_equals_the_materialised_path(world):
    """fitTrainData shards materialised arrays as X[rank::world][:len(X) // world] and walks shuffle_repeat_batch over the shard with
    default_rng(seed + rank); the online path must draw the same ELEMENTS of the augmented set, batch by batch."""
    spec = AugmentSpec(3, 1, 0, seed=2)
    N, batch, epochs, buf, seed = 5, 14, 3, 8, 6
    V = N * spec.multiplicity                                      # 80 (40 per rank at world 2): neither an epoch nor the run is whole batches
    for rank in range(world):
        shard = np.arange(V)[rank::world][:V // world]
        want = [shard[idx] for idx in shuffle_repeat_batch(len(shard), epochs, batch, buf, np.random.default_rng(seed + rank))]
        per, stream = augment.virtual_index_batches(V, rank, world, epochs, batch, buf, np.random.default_rng(seed + rank))
        got = list(stream)
        assert per == len(shard) and len(got) == len(want)
        assert len(want[-1]) == (epochs * per) % batch != 0                          # the partial last batch
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        # a batch that straddles an epoch: the stream's first `per` elements are one permutation of the shard, and `per` is not a multiple of the batch
        flat = np.concatenate(got)
        assert per % batch != 0 and sorted(flat[:per].tolist()) == shard.tolist() and sorted(flat[per:2 * per].tolist()) == shard.tolist()


class _Stub(WDSRModel):
    def forward(self, x, training=False):
        return x.mean(dim=(1, 2, 3, 4)).view(-1, 1, 1, 1) * 0 + self.flat[:81].view(1, 9, 9, 1)


_host_arrays = augment.DeviceDataset._host_arrays


class _HostDataset:
    """Test-only stand-in for augment.DeviceDataset on a machine without a GPU: same surface, the recipe applied by its numpy statement
    (the kernel itself is held to that statement bit for bit in tests/test_gpu_augment.py)."""

    def __init__(self, X, yHR, yMask, device):
        self.a = _host_arrays(X, yHR, yMask)
        self.N, self.T, self.nbytes = len(self.a[0]), self.a[0].shape[3], sum(x.nbytes for x in self.a)

    def __len__(self):
        return self.N

    def batches(self, index_batches, spec):
        for v in index_batches:
            rec = make_recipe(v, self.N, self.T, spec)
            validate_recipe(rec, self.N, self.T)
            yield tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in apply_recipe_numpy(*self.a, rec))


def _recording_trainer(tmp_path, name, rank, world):
    class Rec(ModelTrainer):
        seen = []
        _rank = staticmethod(lambda: rank)
        _world = staticmethod(lambda: world)

        def trainStep(self, x, hr, mk):
            self.seen.append((x.clone(), hr.clone(), mk.clone()))

        def save(self):
            return None
    model = _Stub("stub", "NIR", 0.0, 1.0, 6, 3, 32, 12, 8, 0.8, 9, 16, seed=0)
    tr = Rec(model, None, None, None, str(tmp_path / name / "c"), str(tmp_path / name / "l"), evalStep=10 ** 9)
    tr.trainLoss(torch.zeros(1)), tr.trainPSNR(torch.zeros(1))
    return tr


@pytest.mark.parametrize("world", [1, 2])
def test_trainer_hands_the_same_batches_to_train_step(tmp_path, monkeypatch, world):
    monkeypatch.setattr(augment, "DeviceDataset", _HostDataset)
    lr, hr = _base(5, seed=21)
    spec = AugmentSpec(3, 1, 0, seed=8)
    a, h = _materialise(lr, hr, 3, 1, 0, np.random.RandomState(8))
    X, y, mk = np.array(a), np.array(h), ~np.ma.getmaskarray(h)
    bX, by, bmk = np.array(lr), np.array(hr), ~np.ma.getmaskarray(hr)
    val = [bX, by, bmk]
    for rank in range(world):
        host = _recording_trainer(tmp_path, "host%d" % rank, rank, world)
        host.fitTrainData(X, [y, mk], 16, 3, val, bufferSize=8, seed=6)
        online = _recording_trainer(tmp_path, "online%d" % rank, rank, world)
        online.fitTrainData(bX, [by, bmk], 16, 3, val, bufferSize=8, seed=6, augment=spec)
        per = 80 // world
        assert host.step == online.step == len(host.seen) == len(online.seen) == -(-3 * per // 16)
        for (x1, h1, m1), (x2, h2, m2) in zip(host.seen, online.seen):
            assert x1.dtype == x2.dtype and h1.dtype == h2.dtype and m1.dtype == m2.dtype == torch.bool
            assert torch.equal(x1, x2) and torch.equal(h1, h2) and torch.equal(m1, m2)
