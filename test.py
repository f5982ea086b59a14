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

--fuse applies the band's latest FuseNet checkpoint (train.py --modelType fusionNet; <model_out>/fuseNetCkpt_<cfg>/<band>) to the stitched, rounded
image of whichever path above produced it, on the device, and writes the result clipped to 0..65535 and rounded half to even (INTEGRATION.md,
'FuseNet').  No checkpoint there is an error naming the directory.  Without the flag every path above is what it was, byte for byte.

--method baseline [--baseline-mode esa|clear] [--baseline-frames raw|registered] writes the competition's bicubic-mean baseline instead
(probav_amd/baseline.py): every LR frame upscaled by the Keys cubic and the frames of maximum clearance averaged, in exact
integer arithmetic on the device.  It reads <preprocessing_out>/arrayDir (raw: every set, unregistered) or trimmedArrayDir (registered) and
needs no checkpoint; it does not combine with --ensemble, --tile-stride, --frame-windows, --weights ema or --fuse.  --method network (default) is the path above.
"""
import argparse
import logging
import os

import numpy as np

from probav_amd.inference import add_inference_args, fuse_images, inference_options, load_inputs, load_model, numbered, predict
from probav_amd.parseConfig import parseConfig
from probav_amd.pngio import imsave_uint16

logging.basicConfig(format="%(asctime)s - %(message)s", level=logging.INFO)
logger = logging.getLogger("probav_amd")


def parser(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", default="cfg/FINAL.cfg", type=str)
    p.add_argument("--band", type=str, default="RED")
    p.add_argument("--totest", type=str, default="TEST")
    p.add_argument("--micro-batch", type=int, default=2048, help="patches per forward launch; 16 = the reference's resolveByBatch (test.py:125). "
                   "Samples are independent, so the images do not depend on it")
    p.add_argument("--reference-loop", action="store_true", help="launch every micro-batch of 16 patches on its own, as the reference's loop does "
                   "(test.py:125-134; 3x slower, same pixels); by default the micro-batches are coalesced into launch sets")
    add_inference_args(p)
    p.add_argument("--method", type=str, default="network", choices=("network", "baseline"), help="network (default): the cfg's latest checkpoint; "
                   "baseline: the competition's bicubic-mean baseline of the LR frames, which needs no checkpoint")
    from probav_amd.baseline import add_cli_args, cli_spec
    add_cli_args(p)
    opt = p.parse_args(argv)
    if opt.method == "baseline":
        for given, flag in ((opt.ensemble != "none", "--ensemble"), (opt.tile_stride != 0, "--tile-stride"), (opt.weights == "ema", "--weights ema"),
                            (opt.frame_windows != 0, "--frame-windows"), (opt.fuse, "--fuse")):
            if given:
                p.error("%s predicts with the network: it cannot be combined with --method baseline" % flag)
    opt.baseline = cli_spec(p, opt, opt.method == "baseline", "--method baseline")
    for given, flag in ((opt.ensemble != "none", "--ensemble"), (opt.tile_stride != 0, "--tile-stride"), (opt.frame_windows != 0, "--frame-windows"),
                        (opt.fuse, "--fuse")):
        if given and opt.reference_loop:
            p.error("--reference-loop is the reference's plain loop: it cannot be combined with %s" % flag)
    inference_options(p, opt)
    return opt


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


def log_options(options):
    """The one log line that says which of the options predict the images (none for the plain prediction)."""
    spec, tiles, windows = options.ensemble, options.tiles, options.windows
    if windows is not None:
        logger.info("[ INFO ] %d frame windows at step %d, %s weights%s%s" % (windows.windows, windows.step, windows.weights,
                                                                           "" if tiles is None else ", overlapping tiles at stride %d (%s window)" % (tiles.stride, tiles.window),
                                                                           "" if spec is None else ", self-ensemble of %d members per window" % spec.V))
    elif tiles is not None:
        logger.info("[ INFO ] Overlapping tiles at stride %d, %s window%s" % (tiles.stride, tiles.window, "" if spec is None else ", self-ensemble of %d members per tile" % spec.V))
    elif spec is not None:
        logger.info("[ INFO ] Self-ensemble of %d members per patch" % spec.V)


def main(config, opt):
    if getattr(opt, "baseline", None) is not None:
        return main_baseline(config, opt)
    options = opt.inference
    logger.info("[ INFO ] Loading data...")
    inputs = load_inputs(config, opt.totest, opt.band, options)
    model, _ = load_model(config, opt.cfg, opt.band, options.weights, "test.py", gemm_route=opt.gemm_route, gemm_pair=opt.gemm_pair, gemm_x6=opt.gemm_x6, gemm_exotic=opt.gemm_exotic)
    logger.info("[ INFO ] Generating predictions...")
    log_options(options)
    y_preds = (predict(model, inputs, options, config, micro_batch=16, launch_batch=16) if opt.reference_loop
               else predict(model, inputs, options, config, micro_batch=opt.micro_batch))
    if options.fuse:
        logger.info("[ INFO ] Applying the band's FuseNet to the stitched images...")
        del model
        y_preds = fuse_images(y_preds, config, opt.cfg, opt.band, "test.py --fuse")
    outDir = (config["test_out"] if opt.totest == "TEST" else config["train_out"]) + "_" + os.path.basename(opt.cfg).split(".")[0]
    os.makedirs(outDir, exist_ok=True)
    logger.info("[ SAVE ] Saving predicted images to %s..." % outDir)
    for i, img in numbered(y_preds, opt.totest, opt.band):
        imsave_uint16(os.path.join(outDir, "imgset%04d.png" % i), img[:, :, 0].astype(np.uint16))


if __name__ == "__main__":
    opt = parser()
    main(parseConfig(opt.cfg), opt)
