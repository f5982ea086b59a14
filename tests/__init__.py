import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(stem):
    """The arrays of the fixture tests/golden/<stem>.npz, or of the parts <stem>.part0.npz, <stem>.part1.npz, ... it is stored in
    (no committed file exceeds 1 MiB): the parts' arrays merged, an array that several parts hold concatenated along its first
    axis in part order."""
    whole = os.path.join(GOLD, stem + ".npz")
    if os.path.exists(whole):
        return dict(np.load(whole))
    parts = sorted(glob.glob(os.path.join(GOLD, stem + ".part*.npz")), key=lambda p: int(p.rsplit(".part", 1)[1][:-4]))
    if not parts:
        raise FileNotFoundError("no golden fixture %s(.partK).npz under %s" % (stem, GOLD))
    out = {}
    for p in parts:
        for k, v in np.load(p).items():
            out[k] = np.concatenate([out[k], v]) if k in out else v
    return out
