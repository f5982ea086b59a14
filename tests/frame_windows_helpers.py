"""Shared pieces of the frame-window tests: synthetic masked-pixel counts that reach every branch of the frame choice, and the unfold of the
seeded cloudy frames (tests/tiles_helpers.py) the host and the device tests both read."""
import numpy as np

from probav_amd.frame_windows import max_masked

from tests.tiles_helpers import CONFIG, cloudy_frames, numpy_unfold

THRESHOLD = 0.85
WCONFIG = dict(CONFIG, num_low_res_imgs_pre=13)


def synthetic_counts(T_pre, pixels, k, L, seed=0):
    """({name: row index}, int32 [rows, T_pre]): one row of masked-pixel counts per case of the frame choice that T_pre, k and L admit --
    all distinct, all zero, all equal to `pixels`, E = 0, E = 1, 1 < E < k with m = 2 and with m > 2, E = k, E = T_pre (with ties), counts
    exactly L - 1 and L -- and two random rows with ties.  E counts the eligible frames (count < L), m = ceil(k / E)."""
    rng = np.random.default_rng(seed + 1000 * T_pre + k)
    assert 1 <= L <= pixels, (L, pixels)                                # both sides of the limit exist
    rows, names = [], {}

    def add(name, row):
        names[name] = len(rows)
        rows.append(np.asarray(row, np.int64))

    def with_eligible(E):
        """E frames below L (ties among them when L is small), the rest at or above it, at random positions."""
        row = rng.integers(L, pixels + 1, T_pre)
        row[rng.permutation(T_pre)[:E]] = rng.integers(0, L, E)
        return row

    if T_pre <= L:
        add("distinct", rng.permutation(L)[:T_pre])
    add("zero", np.zeros(T_pre))
    add("full", np.full(T_pre, pixels))
    add("E=0", rng.integers(L, pixels + 1, T_pre))
    add("E=1", with_eligible(1))
    for E in range(2, min(k, T_pre + 1)):
        m = -(-k // E)
        name = "m=2" if m == 2 else "m>2"
        if name not in names:
            add(name, with_eligible(E))
    if k <= T_pre:
        add("E=k", with_eligible(k))
    add("E=T_pre", rng.integers(0, max(1, min(L, 3)), T_pre))           # everything eligible, many ties
    edge = np.where(rng.integers(0, 2, T_pre) == 1, L - 1, L)
    edge[0], edge[-1] = L, L - 1
    add("edge", edge)
    add("random-a", rng.integers(0, pixels + 1, T_pre))
    add("random-b", rng.integers(max(0, L - 3), min(pixels, L + 2) + 1, T_pre))
    return names, np.stack(rows).astype(np.int32)


def eligible(counts, L):
    """E per row, with the statement's rule that a row without an eligible frame takes them all."""
    E = (np.asarray(counts) < L).sum(-1)
    return np.where(E == 0, np.asarray(counts).shape[-1], E)


def distinct_frames(images=2, T=9, H=64, seed=7):
    """Masked float64 [images, T, 1, H, H] whose tiles (22 x 22 windows at LR stride 16 or 8, reflect pad 3) all have pairwise distinct
    masked-pixel counts below the 0.85 limit of 73, so the builder's frame choice has no ties: frame t masks c_t = 2 perm[t] + (t % 2) cells
    (distinct, at most 17) of a lattice of period 16, at offsets 5 .. 10 of the period.  A window starts at offset 13 or 5 of the period and
    holds 22 rows, so it sees each of those offsets once or twice per axis and the reflected border (offsets 1 .. 3 and 12 .. 14) never:
    its counts are c_t, 2 c_t or 4 c_t, distinct and at most 68.  perm differs per image."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2 ** 14, (images, T, 1, H, H)).astype(np.float64)
    mask = np.zeros((images, T, 1, H, H), bool)
    cells = [(y, x) for y in (5, 6, 7, 8, 9, 10) for x in (5, 6, 7, 8, 9, 10)]              # offsets within a 16-pixel period: once per window
    for i in range(images):
        perm = rng.permutation(T)
        for t in range(T):
            for y, x in cells[:2 * perm[t] + (1 if t % 2 else 0)]:
                mask[i, t, 0, y::16, x::16] = True
    return np.ma.masked_array(data, mask=mask)


_UNFOLDS = {}


def unfolded_cloudy(T, images=2, H=64, stride=16):
    """(frames, patches float32 [images n n, T, 22, 22], counts int32 [images n n, T]) of cloudy_frames(images, T, H) at the stride; computed
    once per shape and shared (do not write into it)."""
    key = (images, T, H, stride)
    if key not in _UNFOLDS:
        frames = cloudy_frames(images=images, T=T, H=H)
        data, mask = np.ma.getdata(frames).reshape(images, T, H, H), np.ma.getmaskarray(frames).reshape(images, T, H, H)
        pt, _, pc = numpy_unfold(data, mask, 3, 22, stride)
        _UNFOLDS[key] = (frames, pt.reshape(-1, T, 22, 22), pc.reshape(-1, T))
    return _UNFOLDS[key]


LIMIT_22 = max_masked(22 * 22, THRESHOLD)
