"""Refined quality masks on the device (csrc/kernels_refine.hip via probav_amd.prep): the two kernels against the numpy statement
(prep.refine_masks_numpy) bit for bit -- masks, counts and flagged -- over set lengths, frame sizes that straddle the 4 x 64 pixel tile, ties,
clear fractions, dilation at corners, edges and tile seams, saturation and the extreme values; ragged sets in one launch and split over
several; refused arguments; and the feature through registerImages and prep.main on a tiny raw tree."""
import os

import numpy as np
import pytest

from tests.prep_helpers import encode_png
from tests.refine_helpers import ragged, scene_set

pytestmark = pytest.mark.gpu
N = 128
TILE_H, TILE_W = 4, 64                                      # RT_H x RT_W of csrc/kernels_refine.hip: one workgroup's pixels
SIZES = [(1, 1), (5, 7), (16, 16), (37, 150), (7, 70)]      # (7, 70): both dimensions exceed the 4 x 64 tile and are no multiples of it


def _same(got, want):
    for g, w, name in zip(got, want, ("masks", "counts", "flagged")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


def _check(prep, frames, clear, off, spec):
    keep = frames.copy(), clear.copy()
    got = prep.device_refine_masks(frames, clear, off, spec)
    _same(got, prep.refine_masks_numpy(frames, clear, off, spec))
    np.testing.assert_array_equal(frames, keep[0])
    np.testing.assert_array_equal(clear, keep[1])
    return got


def _specs(prep):
    S = prep.RefineSpec
    return [S(k=5, floor=32, min_clear=3, dilate=0), S(k=1, floor=0, min_clear=5, dilate=1, saturation=0),
            S(k=0.5, floor=100, min_clear=4, dilate=2, saturation=16383), S(k=2.0625, floor=3, min_clear=3, dilate=3)]


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 9, 35, 64])
def test_kernel_equals_the_statement(dev, T, hw):
    """One set of T frames (n = T where every look is clear: even and odd n), a neighbour set of 3; a 3-symbol alphabet, all-equal values and
    the whole uint16 range; clear probability 0, 0.5 and 1; every dilate and every saturation setting."""
    from probav_amd import prep
    rng = np.random.default_rng(1000 * T + hw[0] * hw[1])
    flagged_any = 0
    for alphabet in ((0, 300, 20000), (300,), None):
        for p_clear in (0.0, 0.5, 1.0):
            frames, clear, off = ragged(rng, [T, 3], *hw, alphabet=alphabet, p_clear=p_clear)
            for spec in _specs(prep):
                flagged_any += int(_check(prep, frames, clear, off, spec)[2].sum())
    assert flagged_any > 0 or T < 3


@pytest.mark.parametrize("hw", [(7, 70), (37, 150), (1, 1), (2, 65)], ids=lambda s: "%dx%d" % s)
def test_dilation_at_corners_edges_and_tile_seams(dev, hw):
    """Flags planted (as saturated pixels, and as outliers) on the four corners, on every edge and on both sides of the tile seams at
    row 4 and column 64: they grow by `dilate` across the seams and stop at the frame."""
    from probav_amd import prep
    H, W = hw
    rng = np.random.default_rng(7)
    pts = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)}
    for y in (TILE_H - 1, TILE_H, 2 * TILE_H - 1, 2 * TILE_H):
        for x in (TILE_W - 1, TILE_W, 2 * TILE_W - 1, 2 * TILE_W, 5):
            if y < H and x < W:
                pts.add((y, x))
    pts = sorted(pts)
    for dilate in (0, 1, 2, 3):
        frames, _ = scene_set(rng, 6, H, W, noise=10)
        clear = rng.random(frames.shape) < 0.9
        want = np.zeros(frames.shape, bool)
        for i, (y, x) in enumerate(pts):
            t = i % 6
            frames[t, y, x] = 40000 if i % 2 else frames[t, y, x] + 4000          # saturated / an outlier
            clear[:, y, x] = True
            want[t, max(0, y - dilate):y + dilate + 1, max(0, x - dilate):x + dilate + 1] = True
        spec = prep.RefineSpec(k=5, floor=16, min_clear=3, dilate=dilate, saturation=30000)
        out, counts, flagged = _check(prep, frames, clear, [0, 6], spec)
        np.testing.assert_array_equal(clear & ~out, clear & want)               # noise 10 < 5 * 16: nothing else is flagged
        assert flagged.sum() == len(pts) and flagged[:, 0].sum() == len(pts) // 2


def test_extreme_values_with_the_largest_k(dev):
    """0 and 65535 with k16 = 1024: 16 * 65535 = 1048560 lies between 1024 * 1023 and 1024 * 1024, nothing overflows."""
    from probav_amd import prep
    rng = np.random.default_rng(3)
    for T in (5, 8, 64):
        frames, clear, off = ragged(rng, [T, 4], 9, 70, alphabet=(0, 65535), p_clear=0.8)
        frames[:T, 0] = 0
        frames[0, 0] = 65535                                # med = 0, mad = 0 and one look at 65535 wherever it is clear
        frames[:T, 1] = 65535
        frames[1, 1] = 0
        clear[:T, :2] = True
        res = {}
        for floor in (0, 1023, 1024, 65535):
            res[floor] = _check(prep, frames, clear, off, prep.RefineSpec(k=64, floor=floor, min_clear=3, dilate=0, saturation=None))[0]
        assert not res[1023][0, 0].any() and res[1024][0, 0].all() and not res[1023][1, 1].any() and res[1024][1, 1].all()
        _check(prep, frames, clear, off, prep.RefineSpec(k=0, floor=0, min_clear=3, dilate=1, saturation=65534))


def test_ragged_sets_in_one_launch_and_split_over_several(dev):
    """Sets of 1 .. 64 frames side by side, a set of one frame next to a set of 64, sets without a clear pixel: every set gets what it gets
    alone, and the corpus cut into several launches gives the same bytes."""
    from probav_amd import prep
    rng = np.random.default_rng(5)
    sizes = [9, 1, 64, 2, 35, 5, 3, 1, 4, 12]
    H, W = 6, 67
    parts = []
    for i, T in enumerate(sizes):
        fr, _ = scene_set(rng, T, H, W, noise=60)
        fr[rng.random(fr.shape) < 0.03] += 5000
        parts.append(fr)
    frames = np.concatenate(parts)
    clear = rng.random(frames.shape) < 0.85
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    clear[off[4]:off[5]] = False                            # a set of 35 frames without a clear pixel
    clear[off[7]] = True
    for spec in (prep.RefineSpec(k=3, floor=24, min_clear=3, dilate=1, saturation=9000), prep.RefineSpec()):
        whole = _check(prep, frames, clear, off, spec)
        assert whole[2][:, 1].sum() > 0 and (whole[2][:, 0].sum() > 0) == (spec.saturation is not None)
        assert whole[1][off[4]:off[5]].sum() == 0 and not whole[2][off[1]:off[2], 1].any()
        for cut in ([0, 1, 3, 10], [0, 2, 3, 4, 9, 10], list(range(11))):
            for a, b in zip(cut[:-1], cut[1:]):
                sl = slice(off[a], off[b])
                part = prep.device_refine_masks(frames[sl], clear[sl], off[a:b + 1] - off[a], spec)
                _same(part, [w[sl] for w in whole])


SENTINEL64 = np.uint64(0xABABABABABABABAB)


def _raw_call(prep, frames, clear, off, n_sets, n_frames, H, W, max_len, k16, floor, min_clear, dilate, sat, null=None):
    """The C entry itself on sentinel-filled outputs -> (rc, pixel_masks [sets][3][H * W] uint64, out_masks, counts, flagged) as numpy."""
    import torch
    from probav_amd import _lib
    d = torch.device("cuda")
    fr, mk = torch.from_numpy(frames).to(d), torch.from_numpy(clear.view(np.uint8)).to(d)
    od = torch.from_numpy(np.asarray(off, np.int64)).to(d)
    out = torch.full_like(mk, 0xAB)
    flags = torch.full(((len(off) - 1) * 3 * frames.shape[1] * frames.shape[2] * 8,), 0xAB, dtype=torch.uint8, device=d)
    counts = torch.full((len(frames),), -77, dtype=torch.int32, device=d)
    flagged = torch.full((len(frames), 2), -77, dtype=torch.int32, device=d)
    ptrs = {"frames": fr, "masks": mk, "off": od, "flags": flags, "out": out, "counts": counts, "flagged": flagged}
    p = {k: (None if k == null else _lib.ptr(v)) for k, v in ptrs.items()}
    rc = _lib.lib().probav_prep_refine_masks(p["frames"], p["masks"], p["off"], n_sets, n_frames, H, W, max_len, k16, floor, min_clear, dilate, sat,
                                             p["flags"], p["out"], p["counts"], p["flagged"], _lib.current_stream())
    torch.cuda.synchronize()
    planes = flags.cpu().numpy().view(np.uint64).reshape(len(off) - 1, 3, -1)
    return rc, planes, out.cpu().numpy(), counts.cpu().numpy(), flagged.cpu().numpy()


def test_bad_arguments_are_refused_and_nothing_is_written(dev):
    from probav_amd import _lib, prep
    rng = np.random.default_rng(9)
    frames, clear, off = ragged(rng, [3, 7, 2], 5, 70, alphabet=(0, 300, 20000), p_clear=0.9)
    good = dict(n_sets=3, n_frames=12, H=5, W=70, max_len=7, k16=80, floor=32, min_clear=3, dilate=1, sat=-1)
    rc, flags, out, counts, flagged = _raw_call(prep, frames, clear, off, **good)
    assert rc == _lib.PROBAV_OK
    want = prep.refine_masks_numpy(frames, clear, off, prep.RefineSpec(k=5, floor=32, min_clear=3, dilate=1))
    _same((out.astype(bool), counts, flagged), want)
    for i in range(3):                                      # pixel_masks: bit t of plane 0 / 1 / 2 = clear / saturated / outlier of the set's frame t
        bits = lambda k: np.stack([(flags[i, k] >> np.uint64(t)) & np.uint64(1) for t in range(int(off[i + 1] - off[i]))]).astype(bool)
        np.testing.assert_array_equal(bits(0), clear[off[i]:off[i + 1]].reshape(-1, 5 * 70))
        assert not flags[i, 1].any() and (bits(2).sum(1) == want[2][off[i]:off[i + 1], 1]).all()
        assert not (flags[i] >> np.uint64(int(off[i + 1] - off[i]))).any()
    bad = [dict(k16=-1), dict(k16=1025), dict(floor=-1), dict(floor=65536), dict(min_clear=2), dict(min_clear=65), dict(dilate=-1), dict(dilate=4),
           dict(sat=-2), dict(sat=65536), dict(max_len=0), dict(max_len=65), dict(H=0), dict(W=0), dict(n_sets=0), dict(n_frames=0), dict(n_sets=13),
           dict(null="frames"), dict(null="masks"), dict(null="off"), dict(null="flags"), dict(null="out"), dict(null="counts"), dict(null="flagged")]
    for b in bad:
        rc, flags, out, counts, flagged = _raw_call(prep, frames, clear, off, **{**good, **b})
        assert rc == _lib.PROBAV_EINVAL, b
        assert (flags == SENTINEL64).all() and (out == 0xAB).all() and (counts == -77).all() and (flagged == -77).all(), b
    # a precondition that lives in the device array: the set of 7 is longer than the max_set_len the launch was sized for.  It is neither
    # read nor written and its frames are marked; its neighbours are refined as ever
    rc, flags, out, counts, flagged = _raw_call(prep, frames, clear, off, **{**good, "max_len": 3})
    assert rc == _lib.PROBAV_OK
    mid = slice(3, 10)
    assert (flags[1] == SENTINEL64).all() and (out[mid] == 0xAB).all() and (counts[mid] == prep.PREP_BAD_COUNT).all() and (flagged[mid] == prep.PREP_BAD_COUNT).all()
    for sl in (slice(0, 3), slice(10, 12)):
        _same((out[sl].astype(bool), counts[sl], flagged[sl]), [w[sl] for w in want])
    # set_offsets that do not start at 0 or end at n_frames: every frame is marked, nothing else written
    for o in ([1, 3, 10, 12], [0, 3, 10, 11], [0, 10, 3, 12]):
        rc, flags, out, counts, flagged = _raw_call(prep, frames, clear, o, **good)
        assert rc == _lib.PROBAV_OK
        marked = counts == prep.PREP_BAD_COUNT
        assert marked.any() and (out[marked] == 0xAB).all(), o
        if o[1] != 10:
            assert marked.all() and (flags == SENTINEL64).all(), o
    # the Python entry refuses on the host what it can see there
    for o in ([0, 3, 3, 12], [0, 3, 10], [1, 3, 10, 12]):
        with pytest.raises(ValueError):
            prep.device_refine_masks(frames, clear, o, prep.RefineSpec())
    with pytest.raises(ValueError):
        prep.device_refine_masks(np.zeros((65, 2, 2), np.uint16), np.ones((65, 2, 2), bool), [0, 65], prep.RefineSpec())


# ---- through the builder ------------------------------------------------------------------------------------------------------------------
def _texture(rng, lo=2000, hi=20000):
    f = np.fft.fft2(rng.standard_normal((N, N)))
    k = np.fft.fftfreq(N)
    f *= 1.0 / (1e-3 + np.hypot(k[:, None], k[None, :]) ** 1.5)
    t = np.fft.ifft2(f).real
    t = (t - t.min()) / (t.max() - t.min())
    return (lo + t * (hi - lo)).astype(np.int64)


def _sets(rng, n_sets, strip=False):
    """Sets of 9 .. frames of one texture rolled by small shifts plus noise; every set gets a bright blob (an undetected cloud) in one
    frame under a mask that says clear.  strip: frame 3 of every set is rolled by (0, 5) and the 5 columns that wrapped round are given
    other content, as a real shifted acquisition has there."""
    imgs, msks = [], []
    for k in range(n_sets):
        base = _texture(rng)
        T = 9 + k
        fr = []
        for i in range(T):
            s = (0, 0) if i == 0 else (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
            if strip:
                s = (0, 5) if i == 3 else (0, 0)
            f = np.roll(base, s, axis=(0, 1)) + rng.integers(-20, 21, (N, N))
            if strip and i == 3:                            # +-(600 .. 1200) per pixel: far from the scene, yet no pull on the correlation's argmax
                f[:, :5] += rng.integers(600, 1201, (N, 5)) * rng.choice([-1, 1], (N, 5))
            fr.append(f)
        if not strip:
            fr[2][40:52, 60:75] += 5000
        qm = rng.random((T, N, N)) < 0.97
        qm[0] = True                                        # the clearest frame: the reference, unshifted
        imgs.append(np.clip(np.stack(fr), 0, 65535).astype(np.uint16)[:, None])
        msks.append(qm[:, None])
    return imgs, msks


def _flatten(reg):
    data = np.concatenate([np.ma.getdata(a)[:, 0] for a in reg])
    clear = ~np.concatenate([np.ma.getmaskarray(a)[:, 0] for a in reg])
    off = np.concatenate([[0], np.cumsum([len(a) for a in reg])]).astype(np.int64)
    assert (data == np.rint(data)).all()
    return data, clear, off


@pytest.mark.parametrize("tech", ["freq", "time"])
def test_register_images_with_refine_is_registration_then_the_statement(dev, tech):
    from probav_amd import prep
    imgs, msks = _sets(np.random.default_rng(21), 3)
    spec = prep.RefineSpec(k=5, floor=32, min_clear=5, dilate=1, saturation=24000)
    plain = prep.registerImages(imgs, msks, tech, 4)
    got = prep.registerImages(imgs, msks, tech, 4, refine=spec)
    data, clear, off = _flatten(plain)
    gdata, gclear, goff = _flatten(got)
    np.testing.assert_array_equal(gdata, data)              # the data are identical
    np.testing.assert_array_equal(goff, off)
    want, counts, flagged = prep.refine_masks_numpy(data.astype(np.uint16), clear, off, spec)
    np.testing.assert_array_equal(gclear, want)
    assert got[0].dtype == np.float64 and got[0].shape == plain[0].shape
    assert flagged.sum() >= 3 * 12 * 15 * 0.9 and clear.sum() > want.sum()            # the planted blobs, at least


def test_the_strip_that_circular_registration_rolls_in_is_flagged(dev):
    from probav_amd import prep
    imgs, msks = _sets(np.random.default_rng(22), 2, strip=True)
    spec = prep.RefineSpec(k=5, floor=32, min_clear=5, dilate=0)
    plain = prep.registerImages(imgs, msks, "freq")
    got = prep.registerImages(imgs, msks, "freq", refine=spec)
    for k in range(2):
        src = imgs[k][:, 0]
        cnt = msks[k][:, 0].reshape(len(src), -1).sum(1)
        order = np.argsort(-cnt)
        j = int(np.nonzero(order == 3)[0][0])               # where the shifted frame went
        np.testing.assert_array_equal(np.ma.getdata(got[k])[j, 0], np.roll(src[3], (0, -5), axis=(0, 1)))    # registered by (0, -5): the strip is now columns 123 .. 127
        before, after = ~np.ma.getmaskarray(plain[k])[j, 0], ~np.ma.getmaskarray(got[k])[j, 0]
        assert before[:, 123:].sum() > 0.9 * 5 * N and not after[:, 123:].any()
        assert after[:, :123].sum() == before[:, :123].sum()            # noise 20 against 5 * 32: nothing else of the frame


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
num_low_res_permute=0
to_flip=0
to_rotate=0
ckpt=1,2,3,4,5
"""


def _write_tree(root, rng):
    raw = {}
    for split, n_sets in (("train", 3), ("test", 2)):
        imgs, msks = _sets(rng, n_sets)
        for k in range(n_sets):
            d = os.path.join(root, "raw", split, "NIR", "imgset%04d" % (k + (0 if split == "train" else 1160)))
            os.makedirs(d)
            for i in range(len(imgs[k])):
                open(os.path.join(d, "LR%03d.png" % i), "wb").write(encode_png(imgs[k][i, 0].astype(np.int64), 16))
                open(os.path.join(d, "QM%03d.png" % i), "wb").write(encode_png(msks[k][i, 0], 1))
            if split == "train":
                open(os.path.join(d, "HR.png"), "wb").write(encode_png(np.kron(imgs[k][0, 0].astype(np.int64), np.ones((3, 3), np.int64)), 16))
                open(os.path.join(d, "SM.png"), "wb").write(encode_png(rng.random((3 * N, 3 * N)) < 0.97, 1))
        raw[split] = (imgs, msks)
    return raw


def _run_main(prep, raw_root, root, refine, monkeypatch):
    """prep.main, stages 1 to 5, from the raw tree under raw_root into root -> (cfg, {relative path: bytes} of everything it wrote)."""
    from probav_amd.parseConfig import parseConfig
    os.makedirs(root)
    cfgp = os.path.join(root, "t.cfg")
    open(cfgp, "w").write(CFG.format(d=root).replace("raw_data=" + root, "raw_data=" + raw_root))
    monkeypatch.chdir(root)                                 # removedTrainSets<band>.txt goes to the working directory
    cfg = parseConfig(cfgp)
    prep.main(cfg, "NIR", np.random.RandomState(3), refine=refine)
    files = {}
    for dirpath, _, names in os.walk(os.path.join(root, "pre")):
        for n in names:
            p = os.path.join(dirpath, n)
            files[os.path.relpath(p, root)] = open(p, "rb").read()
    return cfg, files


def test_main_runs_its_stages_on_the_refined_dumps_and_the_default_is_unchanged(dev, tmp_path, monkeypatch):
    from probav_amd import prep
    spec = prep.RefineSpec(k=5, floor=32, min_clear=5, dilate=1)
    raw = _write_tree(str(tmp_path / "src"), np.random.default_rng(31))
    _, first = _run_main(prep, str(tmp_path / "src"), str(tmp_path / "a"), None, monkeypatch)
    _, second = _run_main(prep, str(tmp_path / "src"), str(tmp_path / "b"), None, monkeypatch)
    assert sorted(first) == sorted(second) and len(first) >= 20
    for name in first:
        assert first[name] == second[name], name           # a default run writes the bytes it wrote
    cfg, refined = _run_main(prep, str(tmp_path / "src"), str(tmp_path / "c"), spec, monkeypatch)
    assert sorted(refined) == sorted(first)                 # stages 2 to 5 ran and wrote every dump
    for name in first:                                      # stage 1 and the HR side do not depend on it
        if "arrayDir" + os.sep in name and "trimmedArrayDir" not in name or name.endswith("imgHR_NIR.npy") or "patchesHR" in name:
            assert refined[name] == first[name], name
    load = lambda sub, n: np.load(os.path.join(str(tmp_path / "c"), "pre", sub, n + "_NIR.npy"), allow_pickle=True)

    # stage 2 against registration (default) + the numpy statement + the same host bookkeeping under the same seed
    def refined_sets(imgs, msks):
        reg = prep.registerImages(imgs, msks)
        data, clear, off = _flatten(reg)
        want = prep.refine_masks_numpy(data.astype(np.uint16), clear, off, spec)[0]
        return prep._objects([np.ma.masked_array(data[off[i]:off[i + 1], None], mask=~want[off[i]:off[i + 1], None]) for i in range(len(reg))])
    rng = np.random.RandomState(3)
    hr = prep.convertToMaskedArray(load("arrayDir", "TRAINimgHR"), load("arrayDir", "TRAINmskHR"))
    tl, th, removed = prep.removeCorruptedTrainImageSets(refined_sets(*raw["train"]), hr, cfg["low_res_threshold"])
    assert len(removed) == 0
    tl = prep.pickClearLRImgsPerImgSet(tl, 9, cfg["low_res_threshold"], rng)
    tt = prep.pickClearLRImgsPerImgSet(prep.removeCorruptedTestImageSets(refined_sets(*raw["test"]), cfg["low_res_threshold"]), 9,
                                       cfg["low_res_threshold"], rng)
    for name, want in (("TRAINimgLR", tl), ("TESTimgLR", tt)):
        got = load("trimmedArrayDir", name)
        assert got.shape == want.shape and got.dtype == want.dtype
        np.testing.assert_array_equal(np.ma.getdata(got), np.ma.getdata(want))
        np.testing.assert_array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(want))
    base = np.load(os.path.join(str(tmp_path / "a"), "pre", "trimmedArrayDir", "TRAINimgLR_NIR.npy"), allow_pickle=True)
    assert np.ma.getmaskarray(load("trimmedArrayDir", "TRAINimgLR")).sum() > np.ma.getmaskarray(base).sum()      # the blobs are masked now
    # the later stages read those dumps: the patches' masks carry the refinement on
    p3 = load("patchesDir", "TRAINpatchesLR")
    assert p3.shape[:3] == (3, 64, 9) and p3.shape[-2:] == (22, 22)
    assert np.ma.getmaskarray(p3).sum() > np.ma.getmaskarray(np.load(os.path.join(str(tmp_path / "a"), "pre", "patchesDir", "TRAINpatchesLR_NIR.npy"),
                                                                     allow_pickle=True)).sum()
    assert load("augmentedPatchesDir", "TRAINpatchesLR").shape[1:] == (22, 22, 9, 1)
    assert load("trimmedPatchesDir", "TRAINpatchesHR").shape[1:] == (48, 48, 1)
