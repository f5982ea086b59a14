"""The statement of the masked (cloud-aware) registration, probav_amd.prep.register_masked_numpy, on the host: planted shifts under
clouds that mislead the plain circular argmax, the shift against scipy.ndimage.shift, refusals, options and the no-candidate cases."""
import numpy as np
import pytest

from probav_amd import prep
from tests.prep_masked_helpers import N, clouded_pair, cut, plain_circular_argmax, scene


@pytest.mark.parametrize("s", [(2, -3), (-4, 1), (0, 3)])
def test_planted_shift_is_recovered_where_the_plain_argmax_aligns_the_clouds(s):
    ref, img, rc, ic = clouded_pair(21, s)
    shift, registered, out, clear = prep.register_masked_numpy(ref, img, rc, ic, 5)
    assert tuple(shift) == s and registered == 1
    both = clear & rc                                       # clear in the reference and in the shifted frame: the same ground
    assert both.sum() > 0.5 * N * N
    np.testing.assert_array_equal(out[both], ref[both])
    plain = plain_circular_argmax(ref, img)
    print("planted", s, "masked", tuple(shift), "plain circular argmax", plain)
    assert plain != s                                       # recorded: the raw-pixel correlation aligns the two clouds instead
    assert max(abs(plain[0]), abs(plain[1])) > 5


def test_shift_application_is_scipy_reflect_and_a_mask_without_wrap():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (N, N)).astype(np.uint16)
    img[0, 0], img[-1, -1] = 65535, 65535
    clear = rng.random((N, N)) < 0.9
    for s in [(0, 0), (3, -2), (-5, 7), (32, -32), (-1, 0)]:
        out, cl = prep.shift_masked_numpy(img, clear, s)
        assert out.dtype == np.uint16 and cl.dtype == np.bool_
        want = ndi.shift(img.astype(np.float64), s, mode="reflect")
        assert np.abs(want - out).max() <= 1e-9 * 65535, s
        inside = np.zeros((N, N), bool)
        inside[max(0, s[0]):N + min(0, s[0]), max(0, s[1]):N + min(0, s[1])] = True
        assert not cl[~inside].any()                       # nothing wraps in, nothing rings
        src = np.zeros((N, N), bool)
        src[max(0, -s[0]):N + min(0, -s[0]), max(0, -s[1]):N + min(0, -s[1])] = True
        np.testing.assert_array_equal(cl[inside], clear[src])


def test_refusals_and_options():
    ref, img, rc, ic = clouded_pair(21, (1, 1))
    for w in (0, 33, -1, 2.5):
        with pytest.raises(ValueError):
            prep.register_masked_numpy(ref, img, rc, ic, w)
        with pytest.raises(ValueError):
            prep.registerFrame(img[None], ic[None], ref[None], rc[None], tech="time", window=w)
        with pytest.raises(ValueError):
            prep.registerImages([np.stack([ref, img])[:, None]], [np.stack([rc, ic])[:, None]], tech="time", window=w)
        with pytest.raises(ValueError):
            prep.device_register_masked(np.stack([ref, img]), np.stack([rc, ic]), [0, 2], [0], w)
        with pytest.raises(ValueError):
            prep.main({}, "NIR", register="masked", register_window=w)
    for tech in ("masked", "TIME", None, ""):
        with pytest.raises(ValueError):
            prep.registerFrame(img[None], ic[None], ref[None], rc[None], tech=tech)
        with pytest.raises(ValueError):
            prep.registerImages([np.stack([ref, img])[:, None]], [np.stack([rc, ic])[:, None]], tech=tech)
    with pytest.raises(ValueError):
        prep.main({}, "NIR", register="time")              # main and the CLI speak of freq / masked

    import inspect
    for fn in (prep.registerFrame, prep.registerImages):
        p = inspect.signature(fn).parameters
        assert p["tech"].default == "freq" and p["window"].default == 8
    p = inspect.signature(prep.main).parameters
    assert p["register"].default == "freq" and p["register_window"].default == 8
    assert list(inspect.signature(prep.registerFrame).parameters)[:5] == ["img", "msk", "referenceImg", "referenceMsk", "tech"]

    from utils import dataGenerator
    opt = dataGenerator.parser([])
    assert opt.register == "freq" and opt.register_window == 8
    opt = dataGenerator.parser(["--register", "masked", "--register-window", "5"])
    assert opt.register == "masked" and opt.register_window == 5
    with pytest.raises(SystemExit):
        dataGenerator.parser(["--register", "time"])


def test_no_candidate_shift_leaves_the_frame_where_it_is():
    sc = scene(np.random.default_rng(8))
    ref, img = cut(sc), cut(sc, (1, -2))
    rc = np.ones((N, N), bool)
    # an all-cloud frame: n = 0 at every shift
    shift, registered, out, clear = prep.register_masked_numpy(ref, img, rc, np.zeros((N, N), bool), 4)
    assert tuple(shift) == (0, 0) and registered == 0 and not clear.any()
    np.testing.assert_array_equal(out, img)
    # a constant frame: db = 0 at every shift
    const = np.full((N, N), 777, np.uint16)
    ic = np.random.default_rng(9).random((N, N)) < 0.9
    shift, registered, out, clear = prep.register_masked_numpy(ref, const, rc, ic, 4)
    assert tuple(shift) == (0, 0) and registered == 0
    np.testing.assert_array_equal(out, const)
    np.testing.assert_array_equal(clear, ic)
    # a reference without a clear pixel does the same
    shift, registered, _, _ = prep.register_masked_numpy(ref, img, np.zeros((N, N), bool), rc, 4)
    assert tuple(shift) == (0, 0) and registered == 0
