#!/usr/bin/env python3
"""Training CLI with the reference's flags and flow (train.py:26-113): --cfg --band --modelType.

Loads the augmented patch pickles the reference's preprocessing writes
(<preprocessing_out>/augmentedPatchesDir/{TRAIN,TRAINVAL}patches{LR,HR}_<band>.npy, numpy.ma dumps), builds the
WDSR-B Conv3D network on the MI355X engine, and runs ModelTrainer.fitTrainData.  Under
`python -m torch.distributed.run --nproc-per-node N train.py ...` every rank trains on its shard of the data and the
flat gradient buffer is all-reduced once per step (RCCL over xGMI).
"""
import argparse
import logging
import os

import numpy as np
import torch

from probav_amd.inference import BAND_STATS
from probav_amd.loss import Losses
from probav_amd.modelsTF import WDSRConv3D
from probav_amd.parseConfig import parseConfig
from probav_amd.trainClass import ModelTrainer, make_optimizer

logging.basicConfig(format="%(asctime)s - %(message)s", level=logging.INFO)
logger = logging.getLogger("probav_amd")


def parser(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--cfg", default="cfg/yourcfg.cfg", type=str)
    p.add_argument("--band", type=str, default="NIR")
    p.add_argument("--modelType", type=str, default="patchNet")
    p.add_argument("--online-aug", dest="online_aug", action="store_true",
                   help="train from the un-augmented patches of `utils/dataGenerator.py --online-aug`: every batch is augmented on the GPU")
    p.add_argument("--random-crops", dest="random_crops", action="store_true",
                   help="train on crops cut on the GPU out of the registered scenes of trimmedArrayDir (needs `utils/dataGenerator.py --scene-split`)")
    p.add_argument("--crop-positions", dest="crop_positions", default="all", choices=("all", "grid"),
                   help="all: every valid origin, drawn uniformly (default); grid: the builder's patch grid, walked like --online-aug")
    p.add_argument("--crop-seed", dest="crop_seed", type=int, default=0, help="seed of the position / flip / turn / frame-order draws of --crop-positions all")
    p.add_argument("--crops-per-epoch", dest="crops_per_epoch", type=int, default=None,
                   help="samples per epoch with --crop-positions all (default: grid positions x augmentation multiplicity, what an epoch was)")
    # optimizer options on the device (probav_amd/trainClass.py: _GuardedOptions).  Flags, not cfg keys: the cfg is the reference's format
    p.add_argument("--global-clipnorm", dest="global_clipnorm", type=float, default=None,
                   help="Keras global_clipnorm: scale the whole gradient so that its global L2 norm is at most this (tf.clip_by_global_norm)")
    p.add_argument("--skip-nonfinite", dest="skip_nonfinite", action="store_true",
                   help="drop a step whose gradient holds an inf or a NaN (parameters, moments and EMA untouched; counted as 'Skipped steps')")
    p.add_argument("--ema-momentum", dest="ema_momentum", type=float, default=None,
                   help="Keras use_ema / ema_momentum: keep a moving average of the weights with this momentum (e.g. 0.99); checkpoints gain an 'ema' entry")
    p.add_argument("--validate-on", dest="validate_on", type=str, default="raw", choices=("raw", "ema"),
                   help="the weights the validation runs on (ema needs --ema-momentum); default raw")
    opt = p.parse_args(argv)
    if opt.random_crops and opt.online_aug:
        p.error("--random-crops and --online-aug are mutually exclusive")
    if not opt.random_crops and (opt.crop_positions != "all" or opt.crop_seed != 0 or opt.crops_per_epoch is not None):
        p.error("--crop-positions, --crop-seed and --crops-per-epoch need --random-crops")
    if opt.crops_per_epoch is not None and (opt.crop_positions != "all" or opt.crops_per_epoch < 1):
        p.error("--crops-per-epoch must be positive and applies to --crop-positions all")
    if opt.global_clipnorm is not None and not opt.global_clipnorm > 0:
        p.error("--global-clipnorm must be positive")
    if opt.ema_momentum is not None and not 0.0 <= opt.ema_momentum <= 1.0:
        p.error("--ema-momentum must be in [0, 1]")
    if opt.validate_on == "ema" and opt.ema_momentum is None:
        p.error("--validate-on ema needs --ema-momentum")
    return opt


def training_scenes(dataDir, band):
    """The training scenes' indices into trimmedArrayDir that `utils/dataGenerator.py --scene-split` wrote."""
    scenes = os.path.join(dataDir, "TRAINscenes_%s.npy" % band)
    if not os.path.exists(scenes):
        raise SystemExit("--random-crops needs %s: run `utils/dataGenerator.py --scene-split` (stage 5) first -- it holds out whole scenes for "
                         "validation, because random crops would overlap a patch split's validation patches" % scenes)
    return np.load(scenes)


def patchNet(config, opt):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1 or os.environ.get("PROBAV_FORCE_DP") == "1":     # (PROBAV_FORCE_DP=1: the data-parallel step on ONE GPU, over a world-size-1 RCCL group)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=int(os.environ.get("RANK", "0")), world_size=world, device_id=torch.device("cuda", local))
    logger.info("[ INFO ] Loading data...")
    dataDir = os.path.join(config["preprocessing_out"], "augmentedPatchesDir")
    load = lambda n: np.load(os.path.join(dataDir, n % opt.band), allow_pickle=True)
    augment = crop_data = None
    if opt.random_crops:
        # the scenes stay whole on the device; samples are cut out of them per batch (probav_amd/crops.py)
        from probav_amd import crops
        from probav_amd.augment import AugmentSpec
        crop_data = crops.load_scenes(config, opt.band, training_scenes(dataDir, opt.band))
        augment = AugmentSpec.from_config(config, seed=opt.crop_seed)
        X_train = y_train = None
    elif opt.online_aug:
        # the un-augmented arrays and the permutation table stage 5 saved: the augmented set stays virtual (probav_amd/augment.py)
        from probav_amd.augment import AugmentSpec
        X_train, y_train = load("TRAINbasepatchesLR_%s.npy"), load("TRAINbasepatchesHR_%s.npy")
        augment = AugmentSpec.from_config(config, load("TRAINaugperms_%s.npy"))
    else:
        X_train, y_train = load("TRAINpatchesLR_%s.npy"), load("TRAINpatchesHR_%s.npy")
    X_val, y_val = load("TRAINVALpatchesLR_%s.npy"), load("TRAINVALpatchesHR_%s.npy")
    y_val_mask = ~np.ma.getmaskarray(y_val)                                                  # True = clear pixel
    mean, std = BAND_STATS["NIR" if opt.band == "NIR" else "RED"]
    X_val, y_val = np.array(X_val), np.array(y_val)
    if crop_data is None:
        y_train_mask = ~np.ma.getmaskarray(y_train)
        X_train, y_train = np.array(X_train), np.array(y_train)

    logger.info("[ INFO ] Building model...")
    k = config["kernel_size"]
    model = WDSRConv3D(name="superResolutionNet", band=opt.band, mean=mean, std=std, maxShift=config["max_shift"]).build(
        scale=config["scale"], numFilters=config["num_filters"], kernelSize=(k, k, k), numResBlocks=config["num_res_blocks"],
        expRate=config["exp_rate"], decayRate=config["decay_rate"], numImgLR=config["num_low_res_imgs"],
        patchSizeLR=config["patch_size"], isGrayScale=config["is_grayscale"], seed=0).to(torch.device("cuda", local))
    if opt.global_clipnorm is None and not opt.skip_nonfinite and opt.ema_momentum is None:
        optimizer = make_optimizer(config["optimizer"], model, config["learning_rate"])
    else:
        optimizer = make_optimizer(config["optimizer"], model, config["learning_rate"], global_clipnorm=opt.global_clipnorm,
                                   skip_nonfinite=opt.skip_nonfinite, use_ema=opt.ema_momentum is not None,
                                   ema_momentum=0.99 if opt.ema_momentum is None else opt.ema_momentum)
    target = config["scale"] * config["patch_size"]
    loss = Losses(targetShape=(target, target, 1))
    type_loss = {"l1": loss.shiftCompensatedL1Loss, "l2": loss.shiftCompensatedL2Loss,
                 "sobel_l1_mix": loss.shiftCompensatedL1EdgeLoss, "l1msssim": loss.shiftCompensatedRevSSIM}[config["loss"]]
    basename = os.path.basename(opt.cfg).split(".")[0]
    ckptDir = os.path.join(config["model_out"], "ckpt_%s" % basename, opt.band)
    logDir = os.path.join(config["model_out"], "logs_%s" % basename, opt.band)
    trainer = ModelTrainer(model=model, loss=type_loss, metric=loss.shiftCompensatedcPSNR, optimizer=optimizer,
                           ckptDir=ckptDir, logDir=logDir, validate_on=opt.validate_on)
    if crop_data is not None:
        dataset = crops.CropDataset(*crop_data, config, torch.device("cuda", local))
        trainer.fitTrainData(None, None, config["batch_size"], config["epochs"], [X_val, y_val, y_val_mask], saveBestOnly=False, initEpoch=0,
                             augment=augment, crops=(dataset, crops.CropSpec(opt.crop_positions, seed=opt.crop_seed)),
                             crops_per_epoch=opt.crops_per_epoch)
    else:
        trainer.fitTrainData(X_train, [y_train, y_train_mask], config["batch_size"], config["epochs"],
                             [X_val, y_val, y_val_mask], saveBestOnly=False, initEpoch=0, augment=augment)
    logger.info("[ SUCCESS ] Model checkpoint can be found in %s." % ckptDir)
    logger.info("[ SUCCESS ] Model logs can be found in %s." % logDir)


if __name__ == "__main__":
    opt = parser()
    config = parseConfig(opt.cfg)
    if opt.modelType != "patchNet":
        raise SystemExit("--modelType %s: only the patchNet (WDSR-B Conv3D) path is implemented; the reference's fusionNet "
                         "is a separate experimental model with hard-coded paths (train.py:116-188)" % opt.modelType)
    patchNet(config, opt)
