"""Test-time self-ensemble: the variant tables and the numpy statement of what the device computes (csrc/kernels_ensemble.hip;
testClass.resolve_ensemble / resolve_images(..., ensemble=spec) drive it).

It is the geometric self-ensemble of the EDSR / WDSR papers in the form the reference's resolveBySampleAveraging averages
its predictions (test.py:137-146: every member goes through `resolve`, i.e. is clipped and rounded, before the mean).  A variant is
v = (f, k, perm) in the recipe convention of augment.py: flip code f (0 none, 1 axis 0, 2 axis 1, 3 both), k counter-clockwise quarter
turns, frame order perm.  For an LR patch x [H, H, T, C] and an HR-side patch q [S, S]

    A_v(x)    = rot90(flip(x[:, :, perm], FL[f]), k)          what the network is fed           (augment.apply_recipe_numpy's LR tensor)
    G_v(q)    = rot90(flip(q, FL[f]), k)                      how its answer is turned
    G_v^-1(q) = flip(rot90(q, -k), FL[f])
    E(x)      = (1 / V) sum_v G_v^-1( round_half_even( clip( net(A_v(x)), 0, 2**16 ) ) )

The inference patches are the 16-pixel core plus a symmetric 3-pixel border and the network returns the 48 x 48 core, so turning the LR
patch about its centre turns the HR patch the same way: the pairing the training augmentation relies on.  Every member is an integer in
[0, 65536], so for V <= 256 the fp32 sum is exact (<= 2**24) in any order and E is that sum divided once by V in fp32; more members
are refused.  final = "mean": the fp32 mean (what the reference's helper returns); final = "round": the mean rounded half to even once
more, the uint16-range image a PNG needs (test.py truncates with astype(uint16), so it must be fed this form).

Variant tables (`EnsembleSpec.table`): geometry "d8" = the eight rows f in {0, 1} x k in {0, 1, 2, 3}, the eight distinct elements of the
square's symmetry group in flip-then-turn form; permute = P adds P frame orders drawn by augment.draw_perms(P, T, RandomState(seed))
(row 0 the identity) and crosses them with the geometric rows.  Row order: frame order outermost, then f, then k --
v = 8 p + 4 f + k with the geometry on (V = 8 (P + 1)), v = p without (V = P + 1).  V = 1 is the plain prediction.
"""
import numpy as np

from .augment import FLIP_AXES, draw_perms, validate_recipe
from .intmath import clip_rint_numpy

MAX_MEMBERS = 256
GEOMETRIES = {None: ((0, 0),), "d8": tuple((f, k) for f in (0, 1) for k in (0, 1, 2, 3))}


def _check_members(V):
    if not 1 <= V <= MAX_MEMBERS:
        raise ValueError("an ensemble of %d members: 1 <= V <= %d.  Every member is an integer in [0, 2**16]; %d of them sum to at most 2**24, "
                         "which fp32 holds exactly in any order -- more need not, and the result would depend on the order of the sum"
                         % (V, MAX_MEMBERS, MAX_MEMBERS))


class EnsembleSpec:
    """Which variants of a patch are predicted and averaged: `geometry` "d8" (flips x quarter turns) or None, beside `permute` extra frame
    orders drawn from `seed` (the same seed gives the same table, hence the same image; seed None draws from fresh entropy, once per spec)."""

    def __init__(self, geometry="d8", permute=0, seed=None):
        if geometry in ("none", "None"):
            geometry = None
        if geometry not in GEOMETRIES:
            raise ValueError("geometry must be 'd8' or None, got %r" % (geometry,))
        if int(permute) < 0:
            raise ValueError("permute must be >= 0, got %r" % (permute,))
        self.geometry, self.permute, self.seed = geometry, int(permute), seed
        _check_members(self.V)
        self._tables = {}

    @property
    def V(self):
        return len(GEOMETRIES[self.geometry]) * (self.permute + 1)

    def table(self, T):
        """int32 [V, 2 + T], rows {f, k, perm[0..T)}; frame order outermost (row 8 p + 4 f + k for "d8")."""
        T = int(T)
        if T not in self._tables:
            perms = draw_perms(self.permute, T, np.random.RandomState(self.seed))
            geo = GEOMETRIES[self.geometry]
            tab = np.empty((self.V, 2 + T), np.int32)
            for p, perm in enumerate(perms):
                for g, (f, k) in enumerate(geo):
                    tab[p * len(geo) + g, :2] = f, k
                    tab[p * len(geo) + g, 2:] = perm
            self._tables[T] = tab
        return self._tables[T].copy()

    def recipe(self, N, T):
        """int32 [N V, 3 + T]: row n V + v = {n, f_v, k_v, perm_v}, the recipe both kernels take for N base patches."""
        tab, V = self.table(T), self.V
        rec = np.empty((int(N) * V, 3 + T), np.int32)
        rec[:, 0] = np.repeat(np.arange(int(N), dtype=np.int32), V)
        rec[:, 1:] = np.tile(tab, (int(N), 1))
        return rec


def validate_ensemble_recipe(recipe, N, V, T):
    """ValueError unless `recipe` is [N V, 3 + T] with 1 <= V <= 256, every row applicable (augment.validate_recipe) and row n V + v a variant
    of base patch n -- the grouping the reduction relies on (it never reads the base index)."""
    _check_members(int(V))
    r = np.asarray(recipe)
    validate_recipe(r, N, T)
    if r.shape[0] != N * V:
        raise ValueError("an ensemble recipe for %d patches x %d members has %d rows, got %d" % (N, V, N * V, r.shape[0]))
    if not np.array_equal(r[:, 0], np.repeat(np.arange(N), V)):
        raise ValueError("an ensemble recipe is grouped by base patch: row n V + v must carry base index n")


def inverse_geometry(q, f, k):
    """G^-1 of one member [S, S, ...]: flip(rot90(q, -k), FL[f])."""
    return np.flip(np.rot90(q, -int(k), axes=(0, 1)), FLIP_AXES[int(f)])


def ensemble_reduce_numpy(sr, recipe, V, lo=0.0, hi=float(2 ** 16), final="mean", sets=0, grid=0):
    """The definition, member by member (the statement the kernel is tested against): sr [N V, S, S] (or [N V, S, S, 1]) raw predictions ->
    float32 [N, S, S], or with sets * grid * grid == N the stitched [sets, grid S, grid S] (row-major blocks, test.py:149-160)."""
    if final not in ("mean", "round"):
        raise ValueError("final must be 'mean' or 'round', got %r" % (final,))
    sr = np.asarray(sr, dtype=np.float32)
    if sr.ndim == 4 and sr.shape[3] == 1:
        sr = sr[..., 0]
    V = int(V)
    _check_members(V)
    if sr.ndim != 3 or sr.shape[1] != sr.shape[2] or sr.shape[0] % V or not sr.shape[0]:
        raise ValueError("sr must be [N V, S, S] with V = %d; got %s" % (V, sr.shape))
    N, S = sr.shape[0] // V, sr.shape[1]
    r = np.asarray(recipe)
    validate_ensemble_recipe(r, N, V, r.shape[1] - 3)
    out = np.empty((N, S, S), np.float32)
    for n in range(N):
        acc = np.zeros((S, S), np.float32)
        for v in range(V):
            member = clip_rint_numpy(sr[n * V + v], lo, hi)
            acc += inverse_geometry(member, r[n * V + v, 1], r[n * V + v, 2])
        out[n] = acc / np.float32(V)
    if final == "round":
        out = np.rint(out)
    if not grid and not sets:
        return out
    if sets * grid * grid != N:
        raise ValueError("sets * grid * grid must be N = %d; got sets %d, grid %d" % (N, sets, grid))
    return out.reshape(sets, grid, grid, S, S).transpose(0, 1, 3, 2, 4).reshape(sets, grid * S, grid * S)
