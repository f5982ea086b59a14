"""Dataset builder CLI at the reference's path (utils/dataGenerator.py): raw ESA PROBA-V image sets -> the numpy.ma dumps that
train.py and test.py read.  Runs on the GPU (probav_amd.prep); the same cfg keys, `ckpt=` stage selection and output layout as the
reference.  --seed N seeds the frame picking and LR shuffling (equal to the reference after np.random.seed(N)); without it the run is
unseeded, as the reference's is.

    python utils/dataGenerator.py --cfg cfg/p16t9c85r12.cfg --band NIR [--seed 0] [--online-aug | --scene-split] [--register masked [--register-window 8]]
                                     [--refine-masks [--refine-k 5] ...]

--online-aug: stage 5 writes the un-augmented training patches and the frame permutations it drew (TRAINbasepatches{LR,HR}_<band>.npy,
TRAINaugperms_<band>.npy) instead of the augmented set; `train.py --online-aug` augments every batch on the GPU from them.

--scene-split: stage 5 holds out whole scenes instead of patches and writes the TRAINVAL dumps from their grid patches and the training
scenes' indices (TRAINscenes_<band>.npy); `train.py --random-crops` cuts its samples out of those scenes of trimmedArrayDir on the GPU.
Validation scores under a scene split are not comparable with the patch split's.

--register masked: stage 2 registers every LR frame by the cloud-aware masked correlation over a window of +-R integer shifts
(--register-window R, 1..32) and shifts it without wrap-around (the reference's registerFrame(tech='time')); the default, freq, is the
plain circular registration.

--refine-masks [--refine-k 5 --refine-floor 32 --refine-min-clear 5 --refine-dilate 1 --refine-saturation N]: stage 2 takes out of the
quality masks the clear pixels of the registered frames that lie more than k median absolute deviations (at least `floor` DN) from the
temporal median of their set's clear looks, and those above the saturation value; the flags grow by `dilate` pixels (INTEGRATION.md,
'Refined quality masks').  Off by default: without it the run is what it was.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from probav_amd import prep  # noqa: E402
from probav_amd.parseConfig import parseConfig  # noqa: E402


def parser(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--cfg', default='cfg/FINALv2.cfg', type=str)
    p.add_argument('--band', default='NIR', type=str, choices=['NIR', 'RED'])
    p.add_argument('--seed', default=None, type=int)
    p.add_argument('--online-aug', dest='online_aug', action='store_true',
                   help='stage 5 saves the un-augmented training patches and the frame permutations instead of the augmented set '
                        '(for train.py --online-aug)')
    p.add_argument('--scene-split', dest='scene_split', action='store_true',
                   help='stage 5 holds out whole scenes instead of patches: TRAINVAL dumps from their grid patches, TRAINscenes_<band>.npy for the '
                        'rest (for train.py --random-crops)')
    p.add_argument('--register', default='freq', choices=['freq', 'masked'],
                   help="stage 2's registration: freq = plain circular cross-correlation (default); masked = cloud-aware masked "
                        "normalised correlation over a bounded window, shifted without wrap-around")
    p.add_argument('--register-window', dest='register_window', default=8, type=int,
                   help='largest integer shift, per axis, that --register masked tries (1..32)')
    p.add_argument('--refine-masks', dest='refine_masks', action='store_true',
                   help='stage 2 takes temporal outliers (and, with --refine-saturation, saturated pixels) of the registered frames out of '
                        'their quality masks (prep.refine_masks_numpy); off by default')
    p.add_argument('--refine-k', dest='refine_k', default=None, type=float, help='outlier threshold in MADs, a multiple of 1/16 (default 5)')
    p.add_argument('--refine-floor', dest='refine_floor', default=None, type=int, help='smallest scale in DN (default 32)')
    p.add_argument('--refine-min-clear', dest='refine_min_clear', default=None, type=int,
                   help='clear looks a pixel needs before it is judged, 3..64 (default 5)')
    p.add_argument('--refine-dilate', dest='refine_dilate', default=None, type=int, help='radius by which the flags grow, 0..3 (default 1)')
    p.add_argument('--refine-saturation', dest='refine_saturation', default=None, type=int,
                   help='flag clear pixels above this value, e.g. 16383 for the 14-bit depth (default: no saturation test)')
    opt = p.parse_args(argv)
    if opt.scene_split and opt.online_aug:
        p.error('--scene-split and --online-aug are mutually exclusive: a scene split writes no training patches to augment')
    given = {k: getattr(opt, 'refine_' + k) for k in ('k', 'floor', 'min_clear', 'dilate', 'saturation')}
    given = {k: v for k, v in given.items() if v is not None}
    if given and not opt.refine_masks:
        p.error('--refine-%s needs --refine-masks' % sorted(given)[0].replace('_', '-'))
    opt.refine = None
    if opt.refine_masks:
        try:
            opt.refine = prep.RefineSpec(**given)
        except ValueError as e:
            p.error(str(e))
    return opt


if __name__ == '__main__':
    logging.basicConfig(format='%(asctime)s - %(message)s', level=logging.INFO)
    opt = parser()
    logging.info(f'[ CFG - INFO ] Using {opt.cfg} as config file...')
    rng = None if opt.seed is None else np.random.RandomState(opt.seed)
    prep.main(parseConfig(opt.cfg), opt.band, rng, online_aug=opt.online_aug, register=opt.register,
              register_window=opt.register_window, scene_split=opt.scene_split, refine=opt.refine)
