#!/usr/bin/env python3
"""Frame attribution of a trained network over the patches train.py reads: each frame position's share of |d loss / d LR frames|.

    python tools/frame_attribution.py --cfg cfg/p16t9c85r12.cfg --band NIR [--split val] [--max-patches 4096] [--out attribution.csv]

Reads <preprocessing_out>/augmentedPatchesDir/{TRAIN,TRAINVAL}patches{LR,HR}_<band>.npy (--split train | val), restores the cfg's latest
checkpoint (none: the initial weights, said so on stderr), runs forward + the cfg's loss + backward with the LR frames requiring grad
(probav_amd/attribution.py) and writes a CSV: one row per patch with the T shares (they sum to 1), and a last row `mean` of their column
means.  The patches hold their frames from clearest to dirtiest, so the file says whether the network leans on the clear frames or on
positions.  evaluate.py and test.py are not involved.
"""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def parser(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", default="cfg/yourcfg.cfg", type=str)
    p.add_argument("--band", type=str, default="NIR")
    p.add_argument("--split", type=str, default="val", choices=("train", "val"))
    p.add_argument("--max-patches", dest="max_patches", type=int, default=4096, help="the first N patches of the split (0: all)")
    p.add_argument("--micro-batch", dest="micro_batch", type=int, default=128)
    p.add_argument("--weights", type=str, default="raw", choices=("raw", "ema"))
    p.add_argument("--out", type=str, default=None, help="CSV path (default: frame_attribution_<split>_<band>.csv)")
    opt = p.parse_args(argv)
    if opt.max_patches < 0 or opt.micro_batch < 1:
        p.error("--max-patches must be >= 0 and --micro-batch positive")
    return opt


def write_csv(path, shares):
    """shares [N, T] -> rows `patch, frame_0 .. frame_{T-1}` and a last row `mean` (NaN rows, patches with a non-finite gradient, stay out of it)."""
    shares = np.asarray(shares, dtype=np.float64)
    T = shares.shape[1]
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["patch"] + ["frame_%d" % t for t in range(T)])
        for i, row in enumerate(shares):
            w.writerow([i] + ["%.9f" % v for v in row])
        ok = np.isfinite(shares).all(axis=1)
        mean = shares[ok].mean(axis=0) if ok.any() else np.full(T, np.nan)
        w.writerow(["mean"] + ["%.9f" % v for v in mean])
    return mean


def main(argv=None):
    opt = parser(argv)
    from probav_amd.attribution import frame_shares, input_gradient
    from probav_amd.inference import load_model
    from probav_amd.loss import Losses
    from probav_amd.parseConfig import parseConfig
    config = parseConfig(opt.cfg)
    dataDir = os.path.join(config["preprocessing_out"], "augmentedPatchesDir")
    prefix = "TRAIN" if opt.split == "train" else "TRAINVAL"
    load = lambda n: np.load(os.path.join(dataDir, n % (prefix, opt.band)), allow_pickle=True)
    X, y = load("%spatchesLR_%s.npy"), load("%spatchesHR_%s.npy")
    n = len(X) if opt.max_patches == 0 else min(len(X), opt.max_patches)
    mask = ~np.ma.getmaskarray(y)[:n]                                            # True = clear pixel
    X, y = np.array(X)[:n], np.array(y)[:n]
    model, trainer = load_model(config, opt.cfg, opt.band, opt.weights, "tools/frame_attribution.py")
    if trainer.latest_checkpoint is None and trainer._tf_latest() is None:
        print("[ WARN ] no checkpoint under %s: attributing the INITIAL weights" % trainer.ckptDir, file=sys.stderr)
    target = config["scale"] * config["patch_size"]
    losses = Losses(targetShape=(target, target, 1))
    loss_fn = {"l1": losses.shiftCompensatedL1Loss, "l2": losses.shiftCompensatedL2Loss,
               "sobel_l1_mix": losses.shiftCompensatedL1EdgeLoss, "l1msssim": losses.shiftCompensatedRevSSIM}[config["loss"]]
    dx = input_gradient(model, loss_fn, X, y, mask, micro_batch=opt.micro_batch)
    shares = frame_shares(dx).cpu().numpy()
    out = opt.out or "frame_attribution_%s_%s.csv" % (opt.split, opt.band)
    mean = write_csv(out, shares)
    print("[ SUCCESS ] %d patches -> %s ; mean share per frame position (clearest first): %s" % (n, out, " ".join("%.4f" % v for v in mean)))


if __name__ == "__main__":
    main()
