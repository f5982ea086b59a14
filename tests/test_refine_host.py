"""The statement of the mask refinement, probav_amd.prep.refine_masks_numpy, on the host: against an independent per-pixel restatement,
planted defects found exactly with zero false flags, every boundary of the definition, refusals, defaults and the CLI's flags."""
import inspect

import numpy as np
import pytest

from probav_amd import prep
from tests.refine_helpers import ragged, refine_plain, scene_set

Spec = prep.RefineSpec


def _plain(frames, clear, off, spec):
    return refine_plain(frames, clear, off, spec.k16, spec.floor, spec.min_clear, spec.dilate, spec.saturation)


def _agree(frames, clear, off, spec):
    keep = frames.copy(), np.array(clear).copy()
    got = prep.refine_masks_numpy(frames, clear, off, spec)
    want = _plain(frames, clear, off, spec)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(frames, keep[0])         # data are returned untouched
    np.testing.assert_array_equal(clear, keep[1])
    assert got[0].dtype == np.bool_ and got[1].dtype == np.int32 and got[2].dtype == np.int32
    np.testing.assert_array_equal(got[1], got[0].reshape(len(frames), -1).sum(1))
    return got


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (9, 4)])
@pytest.mark.parametrize("alphabet", [(7, 300, 9000), None])
@pytest.mark.parametrize("p_clear", [0.0, 0.5, 1.0])
def test_statement_equals_the_plain_per_pixel_loop(hw, alphabet, p_clear):
    rng = np.random.default_rng(hash((hw, alphabet is None, p_clear)) % 2 ** 32)
    sizes = [int(t) for t in rng.permutation([1, 2, 3, 4, 5, 8])]
    frames, clear, off = ragged(rng, sizes, *hw, alphabet=alphabet, p_clear=p_clear)
    for spec in (Spec(k=5, floor=32, min_clear=3, dilate=1), Spec(k=0.5, floor=0, min_clear=4, dilate=0, saturation=300),
                 Spec(k=1.0625, floor=5, min_clear=5, dilate=2, saturation=40000), Spec(k=0, floor=0, min_clear=3, dilate=3, saturation=0)):
        _agree(frames, clear, off, spec)


def _planted():
    rng = np.random.default_rng(4)
    frames, _ = scene_set(rng, 9, 32, 32, noise=40)
    frames = frames.astype(np.int64)
    clear = np.ones(frames.shape, bool)
    clear[2, 11:16] = False                                # five rows of frame 2
    frames[4, 10:16, 12:20] += 3000
    frames[6, 20:23, 3:6] -= 1500
    blocks = np.zeros(frames.shape, bool)
    blocks[4, 10:16, 12:20] = True
    blocks[6, 20:23, 3:6] = True
    return frames.astype(np.uint16), clear, blocks


def test_planted_defects_are_flagged_exactly():
    """Every clean |x - med| <= 80 = 5 * 16 is not strictly above the threshold; both planted offsets exceed 5 * 80 + 80."""
    frames, clear, blocks = _planted()
    out, counts, flagged = _agree(frames, clear, [0, 9], Spec(k=5, floor=16, min_clear=3, dilate=0))
    np.testing.assert_array_equal(clear & ~out, blocks & clear)
    assert (blocks & clear).sum() == 48 + 9 and flagged[:, 1].sum() == 57 and not flagged[:, 0].any()
    np.testing.assert_array_equal(flagged[:, 1], (blocks & clear).reshape(9, -1).sum(1))
    out1, _, flagged1 = _agree(frames, clear, [0, 9], Spec(k=5, floor=16, min_clear=3, dilate=1))
    grown = np.zeros_like(blocks)
    grown[4, 9:17, 11:21] = True
    grown[6, 19:24, 2:7] = True                            # column 3 grows to column 2, inside the frame
    np.testing.assert_array_equal(clear & ~out1, grown & clear)
    np.testing.assert_array_equal(flagged1, flagged)       # counted before the dilation
    out3, _, _ = _agree(frames, clear, [0, 9], Spec(k=5, floor=16, min_clear=3, dilate=3))
    grown[:] = False
    grown[4, 7:19, 9:23] = True
    grown[6, 17:26, 0:9] = True                            # column 3 less 3: stops at the frame, nothing wraps to column 31
    np.testing.assert_array_equal(clear & ~out3, grown & clear)


def _one(values, clear=None, **kw):
    x = np.array(values, np.uint16).reshape(-1, 1, 1)
    c = np.ones(len(values), bool) if clear is None else np.array(clear, bool)
    out, counts, flagged = _agree(x, c.reshape(-1, 1, 1), [0, len(values)], Spec(**kw))
    return list(c & ~out[:, 0, 0]), flagged


def test_boundaries_of_the_definition():
    # n = min_clear - 1 judges nothing, n = min_clear does
    v = [100, 100, 100, 100, 9000]
    assert _one(v, [0, 1, 1, 1, 1], min_clear=5, dilate=0)[0] == [False] * 5
    assert _one(v, min_clear=5, dilate=0)[0] == [False] * 4 + [True]
    assert _one(v[1:], min_clear=5, dilate=0)[0] == [False] * 4                # T < min_clear
    # 16 d == k16 s is not flagged, one DN more is; mad = 0 uses the floor
    assert _one([1000] * 6 + [1160], k=5, floor=32, dilate=0)[0] == [False] * 7
    assert _one([1000] * 6 + [1161], k=5, floor=32, dilate=0)[0] == [False] * 6 + [True]
    assert _one([1000] * 6 + [840], k=5, floor=32, dilate=0)[0] == [False] * 7
    assert _one([1000] * 6 + [839], k=5, floor=32, dilate=0)[0] == [False] * 6 + [True]
    # mad above the floor: values 0 10 20 30 40 50 x -> med 30, d 30 20 10 0 10 20 |x - 30|, mad 20: 16 d > 80 * 20 from d = 101
    assert _one([0, 10, 20, 30, 40, 50, 130], floor=3, dilate=0)[0] == [False] * 7
    assert _one([0, 10, 20, 30, 40, 50, 131], floor=3, dilate=0)[0] == [False] * 6 + [True]
    # floor = 0 with mad = 0 flags every d > 0
    assert _one([5, 5, 5, 5, 6, 4], floor=0, dilate=0)[0] == [False] * 4 + [True, True]
    assert _one([5, 5, 5, 5, 6, 4], k=0, floor=500, dilate=0)[0] == [False] * 4 + [True, True]      # k = 0: the same
    # x == saturation is not flagged, saturation + 1 is
    f, flagged = _one([16383] * 5 + [16384], saturation=16383, k=64, dilate=0)
    assert f == [False] * 5 + [True] and flagged.tolist() == [[0, 0]] * 5 + [[1, 0]]
    assert _one([0] * 5 + [1], [1, 1, 1, 1, 0, 0], saturation=0, k=64, dilate=0)[0] == [False] * 6   # an unclear look is not saturated
    # saturated looks are excluded from med and mad: with them the median would be 60000 and the three 10s the outliers
    f, flagged = _one([10, 10, 10, 60000, 60000, 60000, 60000], saturation=50000, min_clear=3, dilate=0)
    assert f == [False] * 3 + [True] * 4 and flagged.tolist() == [[0, 0]] * 3 + [[1, 0]] * 4
    f, _ = _one([10, 10, 10, 60000, 60000, 60000, 60000], min_clear=3, dilate=0)
    assert f == [True] * 3 + [False] * 4
    # med = 0 with x = 65535 and k16 = 1024: 16 * 65535 = 1048560 against 1024 * 1023 = 1047552 and 1024 * 1024 = 1048576
    assert _one([0, 0, 0, 0, 65535], k=64, floor=1023, dilate=0)[0] == [False] * 4 + [True]
    assert _one([0, 0, 0, 0, 65535], k=64, floor=1024, dilate=0)[0] == [False] * 5
    assert _one([65535, 65535, 65535, 65535, 0], k=64, floor=1023, dilate=0)[0] == [False] * 4 + [True]
    # even n takes the LOWER median: 0 0 100 100 -> med 0, d 0 0 100 100, mad 0
    assert _one([0, 0, 100, 100], min_clear=4, floor=1, dilate=0)[0] == [False, False, True, True]


def test_default_spec_and_refusals():
    s = Spec()
    assert (s.k, s.floor, s.min_clear, s.dilate, s.saturation, s.k16) == (5.0, 32, 5, 1, None, 80)
    assert Spec(k=64).k16 == 1024 and Spec(k=0.0625).k16 == 1 and Spec(min_clear=64, dilate=3, floor=65535, saturation=65535)
    for bad in (dict(k=5.01), dict(k=-0.0625), dict(k=64.0625), dict(k=float("nan")), dict(k="5"), dict(k=True), dict(floor=-1),
                dict(floor=65536), dict(floor=1.5), dict(min_clear=2), dict(min_clear=65), dict(dilate=-1), dict(dilate=4), dict(dilate=True),
                dict(saturation=-1), dict(saturation=65536), dict(saturation=1.0)):
        with pytest.raises(ValueError):
            Spec(**bad)
    x, c = np.zeros((65, 2, 2), np.uint16), np.ones((65, 2, 2), bool)
    with pytest.raises(ValueError):
        prep.refine_masks_numpy(x, c, [0, 65], Spec())                           # T > 64
    prep.refine_masks_numpy(x, c, [0, 64, 65], Spec())
    for off in ([0, 3, 3, 65], [1, 65], [0, 64], [0]):
        with pytest.raises(ValueError):
            prep.refine_masks_numpy(x, c, off, Spec())
    with pytest.raises(ValueError):
        prep.refine_masks_numpy(x, c[:, :1], [0, 64, 65], Spec())
    with pytest.raises(ValueError):
        prep.refine_masks_numpy(x, c, [0, 64, 65], (5.0, 32, 5, 1, None))
    for fn in (prep.registerImages, prep.main):
        with pytest.raises(ValueError):
            fn(*(([x[:2, None]], [c[:2, None]]) if fn is prep.registerImages else ({}, "NIR")), refine=(5.0, 32, 5, 1, None))


def test_the_feature_is_off_by_default():
    assert inspect.signature(prep.registerImages).parameters["refine"].default is None
    assert inspect.signature(prep.main).parameters["refine"].default is None
    assert list(inspect.signature(prep.registerImages).parameters) == ["allImgLR", "allMskLR", "tech", "window", "refine"]
    from utils import dataGenerator
    opt = dataGenerator.parser([])
    assert opt.refine is None and not opt.refine_masks
    opt = dataGenerator.parser(["--refine-masks"])
    assert opt.refine == Spec()
    opt = dataGenerator.parser(["--refine-masks", "--refine-k", "3.5", "--refine-floor", "8", "--refine-min-clear", "4", "--refine-dilate", "2",
                                "--refine-saturation", "16383"])
    assert opt.refine == Spec(k=3.5, floor=8, min_clear=4, dilate=2, saturation=16383)
    for flag, val in (("--refine-k", "5"), ("--refine-floor", "32"), ("--refine-min-clear", "5"), ("--refine-dilate", "1"),
                      ("--refine-saturation", "16383")):
        with pytest.raises(SystemExit):
            dataGenerator.parser([flag, val])                # not without --refine-masks
    for flag, val in (("--refine-k", "5.01"), ("--refine-dilate", "4"), ("--refine-min-clear", "2")):
        with pytest.raises(SystemExit):
            dataGenerator.parser(["--refine-masks", flag, val])
