#!/usr/bin/env python3
"""Training CLI with the reference's flags and flow (train.py:26-113): --cfg --band --modelType.

Loads the augmented patch pickles the reference's preprocessing writes
(<preprocessing_out>/augmentedPatchesDir/{TRAIN,TRAINVAL}patches{LR,HR}_<band>.npy, numpy.ma dumps), builds the
WDSR-B Conv3D network on the MI355X engine, and runs ModelTrainer.fitTrainData.  Under
`python -m torch.distributed.run --nproc-per-node N train.py ...` every rank trains on its shard of the data and the
flat gradient buffer is all-reduced once per step (RCCL over xGMI).

--modelType fusionNet --fusion-input DIR trains the reference's stitching network instead (FuseNetConv2D, models/modelsTF.py:391-474, train.py:116-188;
INTEGRATION.md, 'FuseNet'): DIR holds the imgsetNNNN.png that `test.py --totest TRAIN` writes, the target and mask are
trimmedArrayDir/TRAINimgHR_<band>.npy matched by id, the split is train_test_split(test_size=split, random_state=17), the loss is the
shift-compensated L1 on 384 x 384, the metric the cPSNR, the optimizer the cfg's; checkpoints go to <model_out>/fuseNetCkpt_<cfg>/<band>.  Unlike
the reference: one band per run, paths from the cfg and the flags instead of the author's home directory, and all images of the folder instead
of the first 1 160.
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
    p.add_argument("--fusion-input", dest="fusion_input", type=str, default=None,
                   help="with --modelType fusionNet: the folder of imgsetNNNN.png that `test.py --totest TRAIN` wrote (the stitched predictions FuseNet corrects)")
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
    p.add_argument("--gemm-route", dest="gemm_route", action="store_true",
                   help="the engine's general matrix route (WDSRModel.set_gemm_route): launches that would run the generic VALU kernels -- a cfg whose "
                        "num_filters, exp_rate or decay_rate are not the shipped ones, e.g. cfg/p16t9c85r12f64.cfg -- run on the fp32-input MFMA instead")
    p.add_argument("--gemm-pair", dest="gemm_pair", action="store_true",
                   help="with --gemm-route: the route's fused pointwise pair (WDSRModel.set_gemm_pair): a block's expConv, ReLU and decConv in one launch "
                        "each way, the hidden tensor never in memory (F <= 64, decay channels <= 64; the shipped shape keeps its tuned pair)")
    p.add_argument("--gemm-x6", dest="gemm_x6", action="store_true",
                   help="with --gemm-route: the route's convolution launches (forward, backward-data) on the 16-bit matrix pipe (WDSRModel.set_gemm_x6): six bf16 piece products per "
                        "fp32 product, results equal to rounding; combines freely with --gemm-pair, which stays fp32")
    p.add_argument("--gemm-exotic", dest="gemm_exotic", action="store_true",
                   help="with --gemm-route: the 19-frame reducer's 5x5x5 and mirrored-pad launches (forward, backward-filter, the 5x5x5 backward-data) on the route's kernels "
                        "(WDSRModel.set_gemm_exotic) instead of the generic VALU kernels; a cfg of 7, 9 or 13 frames has none; combines freely with --gemm-pair and --gemm-x6")
    opt = p.parse_args(argv)
    if opt.fusion_input is not None and opt.modelType != "fusionNet":
        p.error("--fusion-input needs --modelType fusionNet")
    if opt.modelType == "fusionNet" and opt.fusion_input is None:
        p.error("--modelType fusionNet needs --fusion-input DIR (the PNGs of test.py --totest TRAIN)")
    if opt.gemm_route and opt.modelType == "fusionNet":
        p.error("--gemm-route is a switch of the patchNet engine: it cannot be combined with --modelType fusionNet")
    if opt.gemm_pair and opt.modelType == "fusionNet":
        p.error("--gemm-pair is a switch of the patchNet engine: it cannot be combined with --modelType fusionNet")
    if opt.gemm_pair and not opt.gemm_route:
        p.error("--gemm-pair needs --gemm-route")
    if opt.gemm_x6 and opt.modelType == "fusionNet":
        p.error("--gemm-x6 is a switch of the patchNet engine: it cannot be combined with --modelType fusionNet")
    if opt.gemm_x6 and not opt.gemm_route:
        p.error("--gemm-x6 needs --gemm-route")
    if opt.gemm_exotic and opt.modelType == "fusionNet":
        p.error("--gemm-exotic is a switch of the patchNet engine: it cannot be combined with --modelType fusionNet")
    if opt.gemm_exotic and not opt.gemm_route:
        p.error("--gemm-exotic needs --gemm-route")
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


def apply_engine_options(model, opt):
    """The engine switches among the flags, set on the freshly built model: --gemm-route, --gemm-pair, --gemm-x6, --gemm-exotic."""
    if opt.gemm_route:
        model.set_gemm_route(True)
    if opt.gemm_pair:
        model.set_gemm_pair(True)
    if opt.gemm_x6:
        model.set_gemm_x6(True)
    if opt.gemm_exotic:
        model.set_gemm_exotic(True)


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
    apply_engine_options(model, opt)
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


def fusion_data(config, band, directory):
    """(X [n, 384, 384, 1] float32, HR [n, 384, 384, 1] float32, clear [n, 384, 384, 1] bool, ids): every imgsetNNNN.png of `directory` with the
    HR image and mask of its id in trimmedArrayDir/TRAINimgHR_<band>.npy (ids as probav_amd.inference.numbered counts them).  A PNG whose id has
    no partner there is an error that names it."""
    import glob
    import re
    from probav_amd.inference import numbered
    from probav_amd.pngio import imread_uint16
    hr_path = os.path.join(config["preprocessing_out"], "trimmedArrayDir", "TRAINimgHR_%s.npy" % band)
    hr = np.load(hr_path, allow_pickle=True)
    index = {i: k for k, (i, _) in enumerate(numbered(range(len(hr)), "TRAIN", band))}
    files = sorted(f for f in glob.glob(os.path.join(directory, "imgset*.png")) if re.fullmatch(r"imgset\d{4}\.png", os.path.basename(f)))
    if not files:
        raise SystemExit("--fusion-input: no imgsetNNNN.png in %s" % directory)
    ids = [int(os.path.basename(f)[6:10]) for f in files]
    for i, f in zip(ids, files):
        if i not in index:
            raise SystemExit("--fusion-input: %s (id %d) has no partner in %s (the %s TRAIN ids there run over %d sets)" % (f, i, hr_path, band, len(hr)))
    rows = [index[i] for i in ids]
    X = np.stack([imread_uint16(f) for f in files]).astype(np.float32)[..., None]
    target = hr[rows][:, 0, 0]
    return X, np.array(target, dtype=np.float32)[..., None], ~np.ma.getmaskarray(target)[..., None], ids


def fusionNet(config, opt):
    """train.py:116-188 of the reference, on the device."""
    from probav_amd.inference import fuse_ckpt_dir
    from probav_amd.modelsTF import FuseNetConv2D
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    logger.info("[ INFO ] Loading data...")
    X, y, clear, ids = fusion_data(config, opt.band, opt.fusion_input)
    n = len(X)
    perm = np.random.RandomState(17).permutation(n)                 # train_test_split(test_size=split, random_state=17), as prep.splitPatches restates it
    n_test = int(np.ceil(config["split"] * n))
    test, train = perm[:n_test], perm[n_test:]
    if len(train) < 1 or n_test < 1:
        raise SystemExit("--fusion-input: %d images split %g leave an empty training or validation part" % (n, config["split"]))
    logger.info("[ INFO ] %d images (%d training, %d validation). Building model..." % (n, len(train), n_test))
    model = FuseNetConv2D(name="fusionNet", band=opt.band).build(seed=0).to(torch.device("cuda"))
    optimizer = make_optimizer(config["optimizer"], model, config["learning_rate"])
    loss = Losses(targetShape=(X.shape[1], X.shape[2], 1))
    ckptDir = fuse_ckpt_dir(config, opt.cfg, opt.band)
    logDir = os.path.join(config["model_out"], "fuseNetLogs_%s" % os.path.basename(opt.cfg).split(".")[0], opt.band)
    trainer = ModelTrainer(model=model, loss=loss.shiftCompensatedL1Loss, metric=loss.shiftCompensatedcPSNR, optimizer=optimizer, ckptDir=ckptDir, logDir=logDir,
                           multiGPU=False)
    batch = min(config["batch_size"], len(train))
    trainer.fitTrainData(X[train], [y[train], clear[train]], batch, config["epochs"], [X[test], y[test], clear[test]], saveBestOnly=False, initEpoch=0)
    if trainer.latest_checkpoint is None:                           # fewer steps than one evaluation interval: keep what was trained
        trainer.save()
    logger.info("[ SUCCESS ] Model checkpoint can be found in %s." % ckptDir)
    logger.info("[ SUCCESS ] Model logs can be found in %s." % logDir)


if __name__ == "__main__":
    opt = parser()
    config = parseConfig(opt.cfg)
    if opt.modelType == "fusionNet":
        fusionNet(config, opt)
    elif opt.modelType != "patchNet":
        raise SystemExit("--modelType %s: patchNet (WDSR-B Conv3D) or fusionNet (FuseNetConv2D)" % opt.modelType)
    else:
        patchNet(config, opt)
