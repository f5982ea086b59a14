#!/usr/bin/env python3
"""Inference CLI with the reference's flags and flow (test.py:25-100): --cfg --band --totest.

Loads <preprocessing_out>/resolverDir/<TEST|TRAIN>patchesLR_<band>.npy ([sets, 64, T, 1, 22, 22]), restores the latest
checkpoint, resolves every image set patch-wise on the MI355X engine (all sets in micro-batches of --micro-batch patches; forward, clip to
[0, 2**16], round half to even and the 8 x 8 stitch into 384 x 384 stay on the device) and writes uint16 PNGs named imgsetNNNN.png, skipping the ids in
removedTrainSets<band>.txt exactly as the reference does.

--ensemble d8 [--ensemble-permute P --ensemble-seed s] writes the test-time self-ensemble instead (probav_amd/ensemble.py): every
patch predicted in 8 (P + 1) flipped / turned / frame-shuffled variants, the clipped and rounded predictions turned back and averaged on the
device, the mean rounded half to even for the PNG.  It costs that many forward passes.  --ensemble none (default) is the path above, byte for byte.

--tile-stride s [--tile-window hat|box] writes the blend of overlapping tiles instead (probav_amd/tiles.py): the registered frames
of <preprocessing_out>/trimmedArrayDir/<TEST|TRAIN>imgLR_<band>.npy are unfolded at LR stride s, the frames of every tile chosen as the dataset
builder chooses them, every tile predicted, and the predictions blended by an integer window in exact arithmetic on the device.  The set order,
hence the PNG names and the omitted ids, is the same.  ((128 - P) / s + 1)^2 / 64 times the forward passes (3.5 x at s = 8); combines with
--ensemble.  --tile-stride 0 (default) is the path above, byte for byte.

--frame-windows W [--frame-window-step s --frame-window-weights clear|uniform] writes the frame-window ensemble instead (probav_amd/frame_windows.py,
INTEGRATION.md): per tile, W windows of num_low_res_imgs frames slid over the frames of trimmedArrayDir/<TEST|TRAIN>imgLR_<band>.npy sorted from
clearest to dirtiest, one prediction per window, their mean weighted by clear pixels in exact integer arithmetic on the device.  W times the forward
passes; it needs num_low_res_imgs_pre >= (W - 1) s + num_low_res_imgs; combines with --tile-stride, --ensemble and --weights ema.
--frame-windows 0 (default) is the path above, byte for byte.

--weights ema predicts with the moving average of the weights that `train.py --ema-momentum M` keeps and saves beside the raw weights (the
checkpoint's "ema" entry); --weights raw (default) is the path above.  A checkpoint without an "ema" entry is refused, not silently read raw.

--method baseline [--baseline-mode esa|clear] [--baseline-frames raw|registered] writes the competition's bicubic-mean baseline instead
(probav_amd/baseline.py): every LR frame upscaled by the Keys cubic and the frames of maximum clearance averaged, in exact
integer arithmetic on the device.  It reads <preprocessing_out>/arrayDir (raw: every set, unregistered) or trimmedArrayDir (registered) and
needs no checkpoint; it does not combine with --ensemble, --tile-stride, --frame-windows or --weights ema.  --method network (default) is the path above.
"""
import argparse
import logging
import os

import numpy as np
import torch

from probav_amd.modelsTF import WDSRConv3D
from probav_amd.parseConfig import parseConfig
from probav_amd.pngio import imsave_uint16
from probav_amd.frame_windows import add_cli_args as add_window_args, cli_window_args
from probav_amd.testClass import evaluate, evaluate_device, evaluate_tiled_frames, evaluate_windowed_frames
from probav_amd.tiles import cli_tile_args
from probav_amd.trainClass import ModelTrainer

logging.basicConfig(format="%(asctime)s - %(message)s", level=logging.INFO)
logger = logging.getLogger("probav_amd")

BAND_STATS = {"NIR": (8075.2045, 3160.7272), "RED": (5266.2245, 3431.8614)}
FIRST_ID = {("TEST", "NIR"): 1306, ("TEST", "RED"): 1160, ("TRAIN", "NIR"): 594, ("TRAIN", "RED"): 0}    # test.py:79-90


def parser(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", default="cfg/FINAL.cfg", type=str)
    p.add_argument("--band", type=str, default="RED")
    p.add_argument("--totest", type=str, default="TEST")
    p.add_argument("--micro-batch", type=int, default=2048, help="patches per forward launch; 16 = the reference's resolveByBatch (test.py:125). "
                   "Samples are independent, so the images do not depend on it")
    p.add_argument("--reference-loop", action="store_true", help="launch every micro-batch of 16 patches on its own, as the reference's loop does "
                   "(test.py:125-134; 3x slower, same pixels); by default the micro-batches are coalesced into launch sets")
    p.add_argument("--ensemble", type=str, default="none", choices=("none", "d8"), help="test-time self-ensemble: d8 = the mean over the 4 quarter "
                   "turns x 2 flips of every patch (8 forward passes per patch); none = the plain prediction")
    p.add_argument("--ensemble-permute", type=int, default=0, help="with --ensemble d8: P further frame orders, crossed with the 8 geometric variants "
                   "(8 (P + 1) members, at most 256)")
    p.add_argument("--ensemble-seed", type=int, default=0, help="seed of the frame orders: the same seed gives the same images")
    p.add_argument("--tile-stride", type=int, default=0, help="predict overlapping tiles at this LR stride and blend them on the device "
                   "(it must divide 128 - patch_size and be at most patch_size; 8 = 3.5 x the forward passes); 0 = disjoint patches placed side by side")
    p.add_argument("--tile-window", type=str, default=None, choices=("hat", "box"), help="with --tile-stride: the blend window (default hat)")
    p.add_argument("--weights", type=str, default="raw", choices=("raw", "ema"), help="which weights of the checkpoint to predict with: raw (default) or "
                   "the moving average a run with train.py --ema-momentum saved; ema on a checkpoint without one is an error")
    p.add_argument("--method", type=str, default="network", choices=("network", "baseline"), help="network (default): the cfg's latest checkpoint; "
                   "baseline: the competition's bicubic-mean baseline of the LR frames, which needs no checkpoint")
    add_window_args(p)
    from probav_amd.baseline import add_cli_args, cli_spec
    add_cli_args(p)
    opt = p.parse_args(argv)
    if opt.method == "baseline":
        for given, flag in ((opt.ensemble != "none", "--ensemble"), (opt.tile_stride != 0, "--tile-stride"), (opt.weights == "ema", "--weights ema"),
                            (opt.frame_windows != 0, "--frame-windows")):
            if given:
                p.error("%s predicts with the network: it cannot be combined with --method baseline" % flag)
    opt.baseline = cli_spec(p, opt, opt.method == "baseline", "--method baseline")
    if opt.ensemble == "none" and opt.ensemble_permute:
        p.error("--ensemble-permute needs --ensemble d8")
    if opt.ensemble != "none" and opt.reference_loop:
        p.error("--reference-loop is the reference's plain loop: it cannot be combined with --ensemble")
    if opt.tile_stride and opt.reference_loop:
        p.error("--reference-loop is the reference's plain loop: it cannot be combined with --tile-stride")
    cli_tile_args(p, opt)
    if opt.frame_windows and opt.reference_loop:
        p.error("--reference-loop is the reference's plain loop: it cannot be combined with --frame-windows")
    opt.windows = cli_window_args(p, opt)
    return opt


def tile_spec(opt):
    """The TileSpec the two --tile flags ask for (None: disjoint patches)."""
    if not opt.tile_stride:
        return None
    from probav_amd.tiles import TileSpec
    return TileSpec(opt.tile_stride, opt.tile_window)


def ensemble_spec(opt):
    """The EnsembleSpec the three --ensemble flags ask for (None: the plain path)."""
    if opt.ensemble == "none":
        return None
    from probav_amd.ensemble import EnsembleSpec
    return EnsembleSpec(opt.ensemble, permute=opt.ensemble_permute, seed=opt.ensemble_seed)


def main_baseline(config, opt):
    """--method baseline: the bicubic-mean baseline of every image set (probav_amd/baseline.py), named as the network's PNGs are."""
    from probav_amd.baseline import baseline_images
    logger.info("[ INFO ] Bicubic-mean baseline (%s frames, %s mode)..." % (opt.baseline.frames, opt.baseline.mode))
    imgs, ids = baseline_images(config, opt.band.upper(), "TEST" if opt.totest == "TEST" else "TRAIN", opt.baseline)
    outDir = (config["test_out"] if opt.totest == "TEST" else config["train_out"]) + "_" + os.path.basename(opt.cfg).split(".")[0]
    os.makedirs(outDir, exist_ok=True)
    logger.info("[ SAVE ] Saving baseline images to %s..." % outDir)
    for i, img in zip(ids, imgs):
        imsave_uint16(os.path.join(outDir, "imgset%04d.png" % i), img)


def main(config, opt):
    if getattr(opt, "baseline", None) is not None:
        return main_baseline(config, opt)
    logger.info("[ INFO ] Loading data...")
    tiles = tile_spec(opt)
    windows = getattr(opt, "windows", None)
    if tiles is not None or windows is not None:
        framesLR = np.load(os.path.join(config["preprocessing_out"], "trimmedArrayDir", "%simgLR_%s.npy" % (opt.totest, opt.band)), allow_pickle=True)
    else:
        dataDir = os.path.join(config["preprocessing_out"], "resolverDir")
        patchLR = np.load(os.path.join(dataDir, "%spatchesLR_%s.npy" % (opt.totest, opt.band)), allow_pickle=True)
        patchLR = np.array(patchLR).transpose((0, 1, 4, 5, 2, 3))                    # -> [sets, 64, 22, 22, T, 1] (test.py:38)
    mean, std = BAND_STATS["NIR" if opt.band == "NIR" else "RED"]
    k = config["kernel_size"]
    model = WDSRConv3D(name="superResolutionNet", band=opt.band, mean=mean, std=std, maxShift=config["max_shift"]).build(
        scale=config["scale"], numFilters=config["num_filters"], kernelSize=(k, k, k), numResBlocks=config["num_res_blocks"],
        expRate=config["exp_rate"], decayRate=config["decay_rate"], numImgLR=config["num_low_res_imgs"],
        patchSizeLR=config["patch_size"], isGrayScale=config["is_grayscale"]).to("cuda")
    basename = os.path.basename(opt.cfg).split(".")[0]
    ckptDir = os.path.join(config["model_out"], "ckpt_%s" % basename, opt.band)
    try:
        ModelTrainer(model, None, None, None, ckptDir, os.path.join(config["model_out"], "logs_%s" % basename, opt.band), weights=opt.weights)   # restores the latest checkpoint
    except ValueError as exc:
        if opt.weights != "ema":
            raise
        raise SystemExit("test.py --weights ema: %s" % exc)
    logger.info("[ INFO ] Generating predictions...")
    spec = ensemble_spec(opt)
    if windows is not None:
        logger.info("[ INFO ] %d frame windows at step %d, %s weights%s%s" % (windows.windows, windows.step, windows.weights,
                                                                           "" if tiles is None else ", overlapping tiles at stride %d (%s window)" % (tiles.stride, tiles.window),
                                                                           "" if spec is None else ", self-ensemble of %d members per window" % spec.V))
        y_preds = evaluate_windowed_frames(model, framesLR, windows, config, tiles=tiles, ensemble=spec)
    elif tiles is not None:
        logger.info("[ INFO ] Overlapping tiles at stride %d, %s window%s" % (tiles.stride, tiles.window, "" if spec is None else ", self-ensemble of %d members per tile" % spec.V))
        y_preds = evaluate_tiled_frames(model, framesLR, tiles, config, ensemble=spec)
    elif spec is not None:
        logger.info("[ INFO ] Self-ensemble of %d members per patch" % spec.V)
        y_preds = evaluate_device(model, patchLR, ensemble=spec, final="round")
    else:
        y_preds = (evaluate_device(model, patchLR, micro_batch=16, launch_batch=16) if opt.reference_loop
                   else evaluate_device(model, patchLR, micro_batch=opt.micro_batch))

    band = opt.band.upper()
    toOmit = []
    if os.path.exists("removedTrainSets%s.txt" % band):
        with open("removedTrainSets%s.txt" % band) as fh:
            toOmit = [int(float(line.split("\n")[0])) for line in fh.readlines()]
    outDir = (config["test_out"] if opt.totest == "TEST" else config["train_out"]) + "_" + basename
    i = FIRST_ID[("TEST" if opt.totest == "TEST" else "TRAIN", "NIR" if band == "NIR" else "RED")]
    os.makedirs(outDir, exist_ok=True)
    logger.info("[ SAVE ] Saving predicted images to %s..." % outDir)
    for img in y_preds:
        while i in toOmit:
            i += 1
        imsave_uint16(os.path.join(outDir, "imgset%04d.png" % i), img[:, :, 0].astype(np.uint16))
        i += 1


if __name__ == "__main__":
    opt = parser()
    main(parseConfig(opt.cfg), opt)
