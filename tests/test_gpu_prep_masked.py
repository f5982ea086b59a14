"""Masked (cloud-aware) registration on the device (csrc/kernels_prep_masked.hip via probav_amd.prep): bit for bit against the numpy
statement prep.register_masked_numpy -- shifts, registered flags, shifted frames, shifted masks and clear counts, no element excluded --
on clouded sets, exact ties, shifts at the window's edge, degenerate rows, through registerImages, and the C entry's argument checks."""
import functools

import numpy as np
import pytest

from tests.prep_masked_helpers import N, cloud, clouded_pair, cut, random_clouds, scene

pytestmark = pytest.mark.gpu
NAMES = ("shifts", "registered", "frames", "masks", "counts")


def _equal(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


@functools.lru_cache(maxsize=None)
def _clouded_sets():
    """3 sets of 2, 3 and 4 frames: one smooth scene per set, planted shifts within +-3, random cloud blocks over 10-40 % of each frame."""
    rng = np.random.default_rng(17)
    frames, clear, planted = [], [], []
    for size in (2, 3, 4):
        sc = scene(rng)
        for k in range(size):
            s = (0, 0) if k == 0 else tuple(int(v) for v in rng.integers(-3, 4, 2))
            f, c = cut(sc, s), np.ones((N, N), bool)
            random_clouds(rng, f, c)
            frames.append(f)
            clear.append(c)
            planted.append(s)
    return np.stack(frames), np.stack(clear), np.array([0, 2, 5, 9], np.int64), np.array(planted)


@functools.lru_cache(maxsize=None)
def _statement(R):
    from probav_amd import prep
    F, C, off, _ = _clouded_sets()
    return prep.register_masked_sets_numpy(F, C, off, off[:-1], R)


@pytest.mark.parametrize("R", [1, 3, 8])
def test_kernel_equals_the_statement_bit_for_bit(dev, R):
    from probav_amd import prep
    F, C, off, planted = _clouded_sets()
    want = _statement(R)
    got = prep.device_register_masked(F, C, off, off[:-1], R)
    _equal(got, want, "R=%d" % R)
    assert got[1].all()
    if R >= 3:                                              # the planted shifts lie inside the window: they are what both find
        np.testing.assert_array_equal(got[0], planted)
    # the plain path on the same frames does not find them: it correlates the clouds
    plain = prep.device_register(F, C, off, off[:-1])[0]
    assert (plain != planted).any(axis=1).sum() >= 3, plain


def test_split_into_launches_changes_nothing(dev):
    from probav_amd import prep
    F, C, off, _ = _clouded_sets()
    want = _statement(8)
    parts = []
    for s in range(3):
        sl = slice(off[s], off[s + 1])
        parts.append(prep.device_register_masked(F[sl], C[sl], [0, off[s + 1] - off[s]], [0], 8))
    _equal(tuple(np.concatenate([p[k] for p in parts]) for k in range(5)), want, "one set per launch")
    # and with another frame of each set as its reference, against the statement for that choice
    ref = off[:-1] + 1
    _equal(prep.device_register_masked(F, C, off, ref, 3), prep.register_masked_sets_numpy(F, C, off, ref, 3), "second frame as reference")


def test_widest_window(dev):
    from probav_amd import prep
    ref, img, rc, ic = clouded_pair(23, (-29, 31))
    F, C = np.stack([ref, img]), np.stack([rc, ic])
    want = prep.register_masked_sets_numpy(F, C, [0, 2], [0], 32)
    got = prep.device_register_masked(F, C, [0, 2], [0], 32)
    _equal(got, want, "R=32")
    assert tuple(got[0][1]) == (-29, 31) and got[1][1] == 1


@pytest.mark.parametrize("R", [2, 7])
def test_exact_tie_goes_to_the_first_shift_visited(dev, R):
    """A frame constant along x, fully clear, against a reference that is clear only on columns [R, 128 - R): every dx reads the same
    pixels' values, so all 2R + 1 shifts of one dy share their integer moments exactly and the first, dx = -R, must win."""
    from probav_amd import prep
    rng = np.random.default_rng(31)
    g = scene(rng)[:, 5].astype(np.int64)                   # a smooth profile along y, longer than the frame
    img = np.repeat(g[40:40 + N, None], N, axis=1).astype(np.uint16)
    ref = (np.repeat(g[40 + 2:40 + 2 + N, None], N, axis=1) + rng.integers(0, 30, (1, N))).astype(np.uint16)   # the frame's rows 2 further on
    rc = np.zeros((N, N), bool)
    rc[:, R:N - R] = True
    F, C = np.stack([ref, img]), np.stack([rc, np.ones((N, N), bool)])
    want = prep.register_masked_sets_numpy(F, C, [0, 2], [0], R)
    got = prep.device_register_masked(F, C, [0, 2], [0], R)
    _equal(got, want, "tie R=%d" % R)
    assert tuple(got[0][1]) == (-2, -R) and got[1][1] == 1


@pytest.mark.parametrize("sign", [(1, 1), (-1, -1), (1, -1)])
def test_shift_at_the_edge_of_the_window_reflects_the_frame_and_clears_the_band(dev, sign):
    from probav_amd import prep
    R = 6
    s = (sign[0] * R, sign[1] * R)
    sc = scene(np.random.default_rng(41))
    ref, img = cut(sc), cut(sc, s)
    rc, ic = np.ones((N, N), bool), np.ones((N, N), bool)
    cloud(img, ic, N - 8, N - 8, 8, 8)                      # the bottom-right 8 x 8 of the frame is the only flagged region
    F, C = np.stack([ref, img]), np.stack([rc, ic])
    want = prep.register_masked_sets_numpy(F, C, [0, 2], [0], R)
    got = prep.device_register_masked(F, C, [0, 2], [0], R)
    _equal(got, want, "edge %r" % (s,))
    assert tuple(got[0][1]) == s
    out, msk = got[2][1], got[3][1]
    band = np.ones((N, N), bool)                            # the band that was shifted in: no source pixel inside the frame
    band[max(0, s[0]):N + min(0, s[0]), max(0, s[1]):N + min(0, s[1])] = False
    assert band.sum() == N * N - (N - R) ** 2 and not msk[band].any()
    fold = lambda i: np.where(i < 0, -i - 1, np.where(i >= N, 2 * N - 1 - i, i))
    np.testing.assert_array_equal(out, img[fold(np.arange(N) - s[0])[:, None], fold(np.arange(N) - s[1])[None, :]])
    assert got[4][1] == msk.sum()


def test_degenerate_rows_do_not_disturb_their_neighbours(dev):
    from probav_amd import prep
    rng = np.random.default_rng(51)
    fr, cl = [], []
    for shifts in (((0, 0), (2, -1)), ((0, 0), (-3, 3), (1, 4))):
        sc = scene(rng)
        for s in shifts:
            f, c = cut(sc, s), np.ones((N, N), bool)
            random_clouds(rng, f, c)
            fr.append(f)
            cl.append(c)
    cloudy, const = cut(sc, (1, 1)), np.full((N, N), 4242, np.uint16)
    # set 0: its own reference, a neighbour, an all-cloud frame and a constant frame; set 1: three sound frames
    F = np.stack([fr[0], fr[1], cloudy, const, fr[2], fr[3], fr[4]])
    C = np.stack([cl[0], cl[1], np.zeros((N, N), bool), rng.random((N, N)) < 0.9, cl[2], cl[3], cl[4]])
    got = prep.device_register_masked(F, C, [0, 4, 7], [0, 4], 4)
    _equal(got, prep.register_masked_sets_numpy(F, C, [0, 4, 7], [0, 4], 4), "with degenerate rows")
    assert got[1].tolist() == [1, 1, 0, 0, 1, 1, 1]
    assert got[0].tolist() == [[0, 0], [2, -1], [0, 0], [0, 0], [0, 0], [-3, 3], [1, 4]]
    np.testing.assert_array_equal(got[2][[0, 2, 3, 4]], F[[0, 2, 3, 4]])   # references and frames without a candidate stay where they are
    np.testing.assert_array_equal(got[3][[0, 2, 3, 4]], C[[0, 2, 3, 4]])
    keep = [0, 1, 4, 5, 6]
    alone = prep.device_register_masked(F[keep], C[keep], [0, 2, 5], [0, 2], 4)
    _equal(tuple(g[keep] for g in got), alone, "neighbours")


def test_through_register_images(dev):
    from probav_amd import prep
    sets_img, sets_msk, planted = [], [], []
    for seed, blocks in ((61, [(60, 70, 30, 40), (70, 10, 45, 50), (20, 30, 50, 60)]), (62, [(5, 5, 20, 30), (40, 40, 60, 50)])):
        sc = scene(np.random.default_rng(seed))
        shifts = [(0, 0), (-1, 2), (2, -3)][:len(blocks)]
        fs, cs = [], []
        for s, b in zip(shifts, blocks):                    # blocks grow along a set: the clear-count order keeps the frames where they are
            f, c = cut(sc, s), np.ones((N, N), bool)
            cloud(f, c, *b)
            fs.append(f)
            cs.append(c)
        sets_img.append(np.stack(fs)[:, None])
        sets_msk.append(np.stack(cs)[:, None])
        planted.append(shifts)
    img, msk = prep._objects(sets_img), prep._objects(sets_msk)
    plain = prep.registerImages(img, msk)
    freq = prep.registerImages(img, msk, tech="freq")
    time = prep.registerImages(img, msk, tech="time", window=5)
    assert plain.dtype == freq.dtype == time.dtype == object and len(plain) == len(freq) == len(time) == 2
    for a, b, c in zip(plain, freq, time):
        assert isinstance(c, np.ma.MaskedArray) and c.dtype == a.dtype == np.float64 and c.shape == a.shape and c.mask.shape == a.mask.shape
        assert c.mask.dtype == a.mask.dtype == np.bool_
        np.testing.assert_array_equal(np.ma.getdata(a), np.ma.getdata(b))            # tech='freq' is the call without the argument
        np.testing.assert_array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b))
    # the clouded frames are aligned by the masked path: wherever a frame and the reference are both clear they show the same ground
    for k, (a, c) in enumerate(zip(plain, time)):
        ref_clear = ~np.ma.getmaskarray(c)[0]
        np.testing.assert_array_equal(np.ma.getdata(c)[0], sets_img[k][0].astype(np.float64))
        for t in range(1, len(c)):
            both = ref_clear & ~np.ma.getmaskarray(c)[t]
            assert both.sum() > 0.4 * N * N
            np.testing.assert_array_equal(np.ma.getdata(c)[t][both], np.ma.getdata(c)[0][both])
    # ... and not by the plain one: its first set's large-cloud frame is aligned cloud to cloud
    a = plain[0]
    both = ~np.ma.getmaskarray(a)[0] & ~np.ma.getmaskarray(a)[2]
    assert (np.ma.getdata(a)[2][both] != np.ma.getdata(a)[0][both]).mean() > 0.5
    # registerFrame, one pair, both names
    f, m = prep.registerFrame(sets_img[0][1], sets_msk[0][1], sets_img[0][0], sets_msk[0][0], tech="time", window=5)
    assert f.dtype == np.float64 and f.shape == (1, N, N) and m.dtype == np.bool_ and m.shape == (1, N, N)
    np.testing.assert_array_equal(f, np.ma.getdata(time[0])[1])
    np.testing.assert_array_equal(m, ~np.ma.getmaskarray(time[0])[1])
    f, m = prep.registerFrame(sets_img[0][1], sets_msk[0][1], sets_img[0][0], sets_msk[0][0])
    np.testing.assert_array_equal(f, np.ma.getdata(plain[0])[1])
    np.testing.assert_array_equal(m, ~np.ma.getmaskarray(plain[0])[1])


def test_argument_checks_launch_nothing(dev):
    import torch
    from probav_amd import _lib, prep
    F, C, off, _ = _clouded_sets()
    L = _lib.lib()
    fr, mk = torch.from_numpy(F[:5]).to(dev), torch.from_numpy(C[:5].view(np.uint8)).to(dev)
    od = torch.tensor([0, 2, 5], dtype=torch.int64, device=dev)
    rd = torch.tensor([0, 2], dtype=torch.int32, device=dev)

    def call(window, n_sets=2, n_frames=5, offsets=od, refs=rd):
        out = (torch.full((5, 2), 77, dtype=torch.int32, device=dev), torch.full((5,), 77, dtype=torch.uint8, device=dev),
               torch.full_like(fr, 77), torch.full_like(mk, 77), torch.full((5,), 77, dtype=torch.int32, device=dev))
        rc = L.probav_prep_register_masked(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(offsets), n_sets, n_frames, _lib.ptr(refs), window,
                                           *[_lib.ptr(o) for o in out], _lib.current_stream())
        torch.cuda.synchronize()
        return rc, [o.cpu().numpy() for o in out]

    untouched = lambda outs: all((o == 77).all() for o in outs)
    for window in (0, 33, -1, 1 << 20):
        rc, outs = call(window)
        assert rc == _lib.PROBAV_EINVAL and untouched(outs), window
        assert b"window" in L.probav_last_error()
    for kw in (dict(n_sets=0), dict(n_frames=0), dict(offsets=None), dict(refs=None)):      # a set table the host can see is bad
        rc, outs = call(3, **kw)
        assert rc == _lib.PROBAV_EINVAL and untouched(outs), kw
    # a set table that is bad on the device (a reference outside its set): marked like probav_prep_register's, the set's frames not written
    rc, outs = call(3, refs=torch.tensor([0, 1], dtype=torch.int32, device=dev))
    assert rc == _lib.PROBAV_OK
    assert (outs[0][2:] == prep.PREP_BAD_SHIFT).all() and all((o[2:] == 77).all() for o in outs[1:])
    _equal(tuple(o[:2] if i != 3 else o[:2].astype(bool) for i, o in enumerate(outs)), prep.register_masked_sets_numpy(F[:2], C[:2], [0, 2], [0], 3),
           "the sound set")
    rc, outs = call(3)                                      # and the same arguments with a good table do launch
    assert rc == _lib.PROBAV_OK and not any((o == 77).all() for o in outs)
    # the Python entry refuses what it can see before it launches
    with pytest.raises(ValueError):
        prep.device_register_masked(F[:5], C[:5], [0, 2, 2, 5], [0, 2, 2], 3)                # an empty set
    with pytest.raises(ValueError):
        prep.device_register_masked(F[:5], C[:5], [0, 2, 5], [0, 1], 3)                      # a reference outside its set
    with pytest.raises(ValueError):
        prep.device_register_masked(F[:5], C[:5], [0, 2, 5], [0, 2], 0)
