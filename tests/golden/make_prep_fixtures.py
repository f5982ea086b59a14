#!/usr/bin/env python3
"""Reference-EXECUTED fixtures for the dataset builder's host bookkeeping (build container only: reads /root/reference).

The numpy-only helpers of the reference's utils/dataGenerator.py run as they are once lifted out of their module (whose imports of
skimage / scipy would fail).  As in make_ref_fixtures.py, this script parses the file with `ast`, compiles ONLY the named function nodes
(sha256-pinned: a changed reference is refused, not run), executes them on seeded small inputs (16 x 16 frames: the helpers are
shape-generic) with np.random.seed set before every call that draws, and stores inputs + outputs in tests/golden/prep_ref.npz.
No text of the reference is written anywhere.  sklearn's train_test_split (present in the build container) backs splitPatches.
Manual tool: nothing in tests/ or the build invokes it.
    python tests/golden/make_prep_fixtures.py
"""
import ast
import hashlib
import os
import sys

import numpy as np

REF = "/root/reference"
REL = "utils/dataGenerator.py"
HERE = os.path.dirname(os.path.abspath(__file__))

NAMES = ["removeAndReplaceDirtyFrames", "pickClearPatchesLR", "pickClearPatches", "isPatchNotCorrupted", "removeCorruptedTrainPatchSets",
         "isPatchSetNotCorrupted", "removeCorruptedTrainImageSets", "removeCorruptedTestImageSets", "isImageSetNotCorrupted",
         "filterImgMskSet", "pickClearImg", "pickClearLRImgsPerImgSet", "augmentByShufflingLRImgs", "augmentByFlipping",
         "augmentByRotating", "convertToMaskedArray", "splitPatches"]
PIN = "0ec5c093bf448018d30a45ef8c96a0ff9820d36ea39cc0a61d89334f6562cba4"


def _lift():
    import math
    from typing import Dict, List, Tuple
    from sklearn.model_selection import train_test_split
    with open(os.path.join(REF, REL)) as fh:
        tree = ast.parse(fh.read(), filename=REL)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in nodes) == sorted(NAMES), [n.name for n in nodes]
    digest = hashlib.sha256("\n".join(ast.dump(n, include_attributes=False) for n in nodes).encode()).hexdigest()
    if "--print-pins" in sys.argv:
        print(digest)
        raise SystemExit(0)
    if digest != PIN:
        raise SystemExit("make_prep_fixtures: the reference code behind %s is not the reviewed one (sha256 %s): read it, then update PIN" % (REL, digest))
    ns = {"np": np, "math": math, "List": List, "Tuple": Tuple, "Dict": Dict, "train_test_split": train_test_split,
          "tqdm": lambda it, **kw: it, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), os.path.join(REF, REL), "exec"), ns)
    return ns


def _ma(rng, shape, frac_hi=0.6, dtype=np.float32):
    data = rng.integers(0, 16, shape).astype(dtype)                       # small values: the fixture stays small; gathers are pinned by the masks too
    lead = shape[:-3] if len(shape) > 3 else shape[:1]
    p = rng.choice([0.0, 0.02, 0.1, 0.3, frac_hi], lead + (1,) * (len(shape) - len(lead)))
    return np.ma.masked_array(data, mask=rng.random(shape) < p)


def _put(out, key, a):
    out[key + "_data"] = np.ma.getdata(a)
    out[key + "_mask"] = np.ma.getmaskarray(a)


def main():
    R = _lift()
    rng = np.random.default_rng(20261016)
    out = {}

    # removeAndReplaceDirtyFrames / pickClearPatchesLR: [S, P, T, 1, 16, 16], two passes as main() runs them (T 9 -> k 9)
    x = _ma(rng, (3, 5, 9, 1, 16, 16))
    x.mask[0, 0] = True                                                    # one patch where no frame passes
    _put(out, "rrd_in", x)
    y, c, n = R["removeAndReplaceDirtyFrames"](x[1], 9, 0.85)
    _put(out, "rrd_out", y)
    out["rrd_counts"] = np.array([c, n])
    p1 = R["pickClearPatchesLR"](x, k=9, clarityThreshold=0.85)
    _put(out, "pcl_pass1", p1)
    _put(out, "pcl_pass2", R["pickClearPatchesLR"](p1, k=7, clarityThreshold=0.7))

    # removeCorruptedTrainPatchSets + pickClearPatches
    lr = _ma(rng, (4, 5, 9, 1, 16, 16))
    hr = _ma(rng, (4, 5, 1, 1, 16, 16))
    hr.mask[2] = rng.random(hr.mask[2].shape) < 0.5                        # every HR patch of set 2 too dirty
    _put(out, "rcp_lr", lr)
    _put(out, "rcp_hr", hr)
    a, b = R["removeCorruptedTrainPatchSets"](lr, hr, clarityThreshold=0.85)
    _put(out, "rcp_out_lr", a)
    _put(out, "rcp_out_hr", b)
    a, b = R["pickClearPatches"](a, b, clarityThreshold=0.85)
    _put(out, "pcp_out_lr", a)
    _put(out, "pcp_out_hr", b)

    # image sets (ragged, object arrays of per-set masked arrays): corrupted-set removal, frame filter, picking with random fill
    sizes = [12, 5, 9, 3, 10]
    sets = [_ma(rng, (t, 1, 16, 16), dtype=np.float64) for t in sizes]
    sets[3].mask[:] = rng.random(sets[3].shape) < 0.8                      # corrupted
    obj = np.empty(len(sets), dtype=object)
    for i, s in enumerate(sets):
        obj[i] = s
        _put(out, "set%d" % i, s)
    out["set_sizes"] = np.array(sizes)
    hrs = _ma(rng, (len(sizes), 1, 1, 16, 16))
    _put(out, "sets_hr", hrs)
    lr_kept, hr_kept, removed = R["removeCorruptedTrainImageSets"](obj, hrs, clarityThreshold=0.3)
    out["rci_removed"] = removed
    _put(out, "rci_hr", hr_kept)
    out["rci_test_kept"] = np.array([len(s) for s in R["removeCorruptedTestImageSets"](obj, clarityThreshold=0.3)])
    out["isc"] = np.array([R["isImageSetNotCorrupted"](s, 0.3) for s in sets])
    for i, s in enumerate(sets):
        _put(out, "filt%d" % i, R["filterImgMskSet"](s, 0.3))
        np.random.seed(100 + i)
        pk, cnt = R["pickClearImg"](s, numImgToPick=9)
        _put(out, "pick%d" % i, pk)
        out["pick%d_count" % i] = np.array(cnt)
    np.random.seed(7)
    _put(out, "pcl_sets", R["pickClearLRImgsPerImgSet"](lr_kept, numImgToPick=9, clarityThreshold=0.3))

    # augmentation on [N, H, W, T, C] / [N, H, W, C]
    aug = _ma(rng, (3, 16, 16, 4, 1))
    augh = _ma(rng, (3, 16, 16, 1))
    _put(out, "aug_in", aug)
    _put(out, "augh_in", augh)
    np.random.seed(3)
    _put(out, "aug_shuffle", R["augmentByShufflingLRImgs"](aug, numPermute=2))
    _put(out, "aug_flip", R["augmentByFlipping"](aug))
    _put(out, "aug_rot", R["augmentByRotating"](aug))
    _put(out, "augh_flip", R["augmentByFlipping"](augh))
    _put(out, "augh_rot", R["augmentByRotating"](augh))

    # convertToMaskedArray: uint16 frames, boolean masks (nonzero = clear)
    img = rng.integers(0, 65536, (4, 1, 1, 16, 16)).astype(np.uint16)
    msk = rng.random((4, 1, 1, 16, 16)) < 0.8
    out["cma_img"], out["cma_msk"] = img, msk
    _put(out, "cma_out", R["convertToMaskedArray"](img, msk))

    # splitPatches (sklearn train_test_split, random_state=17)
    sl, sh = _ma(rng, (23, 16, 16, 4, 1)), _ma(rng, (23, 16, 16, 1))
    _put(out, "split_lr", sl)
    _put(out, "split_hr", sh)
    for k, v in zip(("split_a", "split_av", "split_b", "split_bv"), R["splitPatches"](sl, sh, {"split": 0.2})):
        _put(out, k, v)

    out["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "prep_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
