"""Training from UN-augmented patches: every batch is augmented on the device (torch.ops.probav.augment_batch, csrc/kernels_augment.hip).

The reference materialises its augmentation (utils/dataGenerator.py:227-273; here prep.augmentByShufflingLRImgs / augmentByFlipping /
augmentByRotating, stage 5 of prep.main): (numPermute + 1) frame-shuffled copies of the training set, 4 flipped copies of that, 4 rotated
copies of that -- 20 x the base set for the shipped cfg, 320 x with flips and rotations -- dumped to disk and loaded into host memory.
Each of those samples is a re-arrangement of ONE base sample, so the augmented set is kept VIRTUAL here: element v of it is described by

    i = v % N                                base sample                            N = len(base set), P1 = numPermute + 1
    p = (v // N) % P1                        row of the frame-permutation table     (row 0 is the identity)
    f = (v // (N P1)) % 4   if flip          flip code: 0 none, 1 axis 0, 2 axis 1, 3 both (of one sample's axes)
    k =  v // (N P1 (4 if flip else 1))  if rotate     counter-clockwise quarter turns
    element v = rot90(flip(x[i][:, :, perms[p]] if LR else x[i], FL[f]), k)            flip first, then rotate

which is the order in which stage 5 concatenates its copies: the virtual set equals the materialised one element for element
(tests/test_augment_host.py).  The base arrays live on the device (`DeviceDataset`), a batch is one kernel launch over a recipe
[B, 3 + T] int32 = rows {i, f, k, perm}, and the trainer walks the same shuffled index stream it would walk over the materialised arrays
(`ModelTrainer.fitTrainData(..., augment=spec)`), so both ways of training consume the same tensors step by step.

`AugmentSpec.permute`: "fixed" (default) takes the permutation of row p -- one permutation for the whole set per copy, what the reference
does; "fresh" draws a new permutation for every sample drawn, from the spec's own seeded generator (more variety than a data set on disk
can hold; not comparable with the materialised path).
"""
import numpy as np

FLIP_AXES = [(), (0,), (1,), (0, 1)]                      # flip code -> axes of ONE sample [H, W, ...]


def draw_perms(numPermute, T, rng=None):
    """The table stage 5 applies: identity, then `numPermute` draws of rng.permutation(np.arange(T)), in that order
    (prep.augmentByShufflingLRImgs).  rng: a numpy RandomState / Generator, or None for numpy's global state, as there."""
    rng = np.random if rng is None else rng
    return np.stack([np.arange(T)] + [rng.permutation(np.arange(T)) for _ in range(int(numPermute))]).astype(np.int64)


def _check_table(perms, numPermute):
    perms = np.asarray(perms)
    if perms.ndim != 2 or perms.shape[0] != numPermute + 1 or not np.issubdtype(perms.dtype, np.integer):
        raise ValueError("perms must be an integer table [numPermute + 1 = %d, T]; got shape %s dtype %s" % (numPermute + 1, perms.shape, perms.dtype))
    T = perms.shape[1]
    if not np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(T), perms.shape)):
        raise ValueError("every row of perms must be a permutation of 0..%d" % (T - 1))
    if not np.array_equal(perms[0], np.arange(T)):
        raise ValueError("row 0 of perms must be the identity (the un-shuffled copy comes first)")
    return perms.astype(np.int64)


class AugmentSpec:
    """What stage 5 of the dataset builder would have materialised: `numPermute` frame-shuffled copies beside the original, x 4 flips if
    `flip`, x 4 quarter turns if `rotate`.  `perms`: the [(numPermute + 1), T] table (row 0 the identity) -- the one the builder saved
    with --online-aug; without it the table is drawn from RandomState(seed) as stage 5 draws it, once the frame count is known."""

    def __init__(self, numPermute, flip, rotate, perms=None, seed=None, permute="fixed"):
        if int(numPermute) < 0:
            raise ValueError("numPermute must be >= 0, got %r" % (numPermute,))
        if permute not in ("fixed", "fresh"):
            raise ValueError("permute must be 'fixed' or 'fresh', got %r" % (permute,))
        self.numPermute, self.flip, self.rotate = int(numPermute), bool(flip), bool(rotate)
        self.seed, self.permute = seed, permute
        self.perms = None if perms is None else _check_table(perms, self.numPermute)
        self._fresh = None

    @classmethod
    def from_config(cls, config, perms=None, seed=None, permute="fixed"):
        return cls(config["num_low_res_permute"], config["to_flip"], config["to_rotate"], perms=perms, seed=seed, permute=permute)

    @property
    def multiplicity(self):
        return (self.numPermute + 1) * (4 if self.flip else 1) * (4 if self.rotate else 1)

    def table(self, T):
        """The permutation table for T frames (drawn on first use when the spec was made without one)."""
        if self.perms is None:
            self.perms = draw_perms(self.numPermute, T, np.random.RandomState(self.seed))
        if self.perms.shape[1] != T:
            raise ValueError("the permutation table is for %d frames, the data has %d" % (self.perms.shape[1], T))
        return self.perms

    def fresh_perms(self, B, T):
        if self._fresh is None:
            self._fresh = np.random.default_rng(self.seed)
        return self._fresh.permuted(np.broadcast_to(np.arange(T), (B, T)), axis=1)


def decode(v, N, spec):
    """Virtual indices -> (i, p, f, k) arrays (int64): base sample, permutation-table row, flip code, quarter turns."""
    v = np.asarray(v, dtype=np.int64)
    P1 = spec.numPermute + 1
    i = v % N
    p = (v // N) % P1
    f = (v // (N * P1)) % 4 if spec.flip else np.zeros_like(v)
    k = v // (N * P1 * (4 if spec.flip else 1)) if spec.rotate else np.zeros_like(v)
    return i, p, f, k


def make_recipe(v, N, T, spec):
    """Recipe rows {i, f, k, perm[0..T)} (int32 [B, 3 + T]) of the virtual elements `v` of a base set of N samples with T frames."""
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    V = N * spec.multiplicity
    if len(v) and (v.min() < 0 or v.max() >= V):
        raise ValueError("virtual index out of range: the augmented set has %d x %d = %d elements, got [%d, %d]"
                         % (N, spec.multiplicity, V, v.min(), v.max()))
    i, p, f, k = decode(v, N, spec)
    out = np.empty((len(v), 3 + T), np.int32)
    out[:, 0], out[:, 1], out[:, 2] = i, f, k
    out[:, 3:] = spec.fresh_perms(len(v), T) if spec.permute == "fresh" else spec.table(T)[p]
    return out


def validate_recipe(recipe, N, T):
    """ValueError unless every row can be applied to a base set of N samples with T frames."""
    r = np.asarray(recipe)
    if r.ndim != 2 or r.shape[1] != 3 + T or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("a recipe is an integer array [B, 3 + T = %d]; got shape %s dtype %s" % (3 + T, r.shape, r.dtype))
    if not len(r):
        return
    if r[:, 0].min() < 0 or r[:, 0].max() >= N:
        raise ValueError("recipe: base index out of range [0, %d): [%d, %d]" % (N, r[:, 0].min(), r[:, 0].max()))
    for col, name in ((1, "flip code"), (2, "rotation count")):
        if r[:, col].min() < 0 or r[:, col].max() > 3:
            raise ValueError("recipe: %s outside 0..3: [%d, %d]" % (name, r[:, col].min(), r[:, col].max()))
    if not np.array_equal(np.sort(r[:, 3:], axis=1), np.broadcast_to(np.arange(T), (len(r), T))):
        raise ValueError("recipe: a frame order that is not a permutation of 0..%d" % (T - 1))


def apply_recipe_numpy(lr, hr, mask, recipe):
    """The recipe's meaning in numpy, sample by sample (the statement the kernel is tested against; nothing on the training path calls
    it): out[b] = rot90(flip(x[i][:, :, perm] if LR else x[i], FL[f]), k)."""
    outs = ([], [], [])
    for row in np.asarray(recipe):
        i, f, k, perm = int(row[0]), int(row[1]), int(row[2]), row[3:]
        for o, x in zip(outs, (np.asarray(lr)[i][:, :, perm], np.asarray(hr)[i], np.asarray(mask)[i])):
            o.append(np.rot90(np.flip(x, FLIP_AXES[f]), k, axes=(0, 1)))
    return tuple(np.stack(o) for o in outs)


def virtual_index_batches(V, rank, world, epochs, batchSize, bufferSize, rng):
    """The index stream of one rank over the virtual set: this rank's shard is arange(V)[rank::world][:V // world] -- element for element
    the shard ModelTrainer.fitTrainData takes of materialised arrays -- walked by the same shuffle / repeat / batch stream.  The shard's
    j-th element is rank + world j, so it is never built.  -> (shard length, iterator of int64 index batches)."""
    from .trainClass import shuffle_repeat_batch
    per = V // world
    return per, (rank + world * idx for idx in shuffle_repeat_batch(per, epochs, batchSize, bufferSize, rng))


class RecipeUploader:
    """Host recipes -> device, through pinned slots, asynchronously on the current stream: no pageable copy, no host synchronisation (a
    slot is reused only after its upload has left the host; its event is `slots` batches old when the slot comes round again)."""

    def __init__(self, device, slots=4):
        self.device, self.slots = device, int(slots)
        self._pinned = [None] * self.slots
        self._events = [None] * self.slots
        self._k = 0

    def __call__(self, recipe):
        import torch
        k, B = self._k, len(recipe)
        self._k = (k + 1) % self.slots
        if self._events[k] is not None:
            self._events[k].synchronize()
        if self._pinned[k] is None or self._pinned[k].shape[0] < B or self._pinned[k].shape[1] != recipe.shape[1]:
            self._pinned[k] = torch.empty((B, recipe.shape[1]), dtype=torch.int32, pin_memory=True)
        pin = self._pinned[k][:B]
        pin.numpy()[...] = recipe
        dev = pin.to(self.device, non_blocking=True)
        self._events[k] = torch.cuda.Event()
        self._events[k].record(torch.cuda.current_stream(self.device))
        return dev


class DeviceDataset:
    """The base arrays on the device, uploaded once (cast like trainClass.BatchPrefetcher casts its batches: LR and HR to fp32, the mask in
    its own dtype), and batches of the virtual augmented set made from them by one kernel launch each.  There is no host path: a device
    that is not a HIP device is refused, and a base set that does not fit raises with the number of bytes asked for."""
    SLOTS = 4

    def __init__(self, X, yHR, yMask, device):
        import torch
        from . import ops                                 # noqa: F401  (registers torch.ops.probav.augment_batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceDataset lives on %s: batches are augmented by a HIP kernel on a gfx950 device (no CPU fallback)" % self.device)
        host = self._host_arrays(X, yHR, yMask)
        self.N, self.H, self.T = host[0].shape[0], host[0].shape[1], host[0].shape[3]
        self.nbytes = sum(a.nbytes for a in host)
        try:
            self.lr, self.hr, self.mask = (torch.from_numpy(a).to(self.device) for a in host)
        except torch.OutOfMemoryError as exc:
            raise MemoryError("the un-augmented training set does not fit on %s: %d bytes were asked for (%d samples; LR %d, HR %d, mask %d bytes). "
                              "There is no host-memory fallback: train from the materialised arrays, or on fewer samples."
                              % (self.device, self.nbytes, self.N, host[0].nbytes, host[1].nbytes, host[2].nbytes)) from exc
        self._upload = RecipeUploader(self.device, self.SLOTS)

    @staticmethod
    def _host_arrays(X, yHR, yMask):
        X, yHR, yMask = np.asarray(X), np.asarray(yHR), np.asarray(yMask)
        if X.ndim != 5 or yHR.ndim != 4 or yMask.shape != yHR.shape or yHR.shape[3] != 1 or not (len(X) == len(yHR) >= 1):
            raise ValueError("expected LR [N, H, H, T, C], HR and mask [N, S, S, 1] with N >= 1; got %s %s %s" % (X.shape, yHR.shape, yMask.shape))
        if X.shape[1] != X.shape[2] or yHR.shape[1] != yHR.shape[2]:
            raise ValueError("square patches only (a quarter turn needs them); got LR %s, HR %s" % (X.shape, yHR.shape))
        if yMask.dtype not in (np.bool_, np.uint8):
            raise ValueError("the HR mask must be bool or uint8, got %s" % yMask.dtype)
        return (np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(yHR, dtype=np.float32), np.ascontiguousarray(yMask))

    def __len__(self):
        return self.N

    def batch_from_recipe(self, recipe):
        """(lr_b, hr_b, mask_b) device tensors of a host recipe [B, 3 + T]; validated here, before anything is launched."""
        import torch
        validate_recipe(recipe, self.N, self.T)
        with torch.cuda.device(self.device):
            return torch.ops.probav.augment_batch(self.lr, self.hr, self.mask, self._upload(np.asarray(recipe, dtype=np.int32)))

    def batch(self, v_indices, spec):
        """The virtual elements `v_indices` of the augmented set `spec` describes, as device tensors."""
        return self.batch_from_recipe(make_recipe(v_indices, self.N, self.T, spec))

    def batches(self, index_batches, spec):
        for v in index_batches:
            yield self.batch(v, spec)
