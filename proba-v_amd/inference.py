"""What test.py and evaluate.py --model share: the band and id tables, the network's inference flags and their checks, loading, the one
dispatch into testClass and the numbering of the images.  The bicubic-mean baseline is not a network option: its flags live in baseline.py."""
import os
from dataclasses import dataclass

import numpy as np

from .ensemble import EnsembleSpec
from .frame_windows import WEIGHTS, FrameWindowSpec
from .tiles import LR_SIZE, TileSpec

BAND_STATS = {"NIR": (8075.2045, 3160.7272), "RED": (5266.2245, 3431.8614)}      # train.py:47-52
FIRST_ID = {("TEST", "NIR"): 1306, ("TEST", "RED"): 1160, ("TRAIN", "NIR"): 594, ("TRAIN", "RED"): 0}    # test.py:79-90


@dataclass(frozen=True)
class InferenceOptions:
    """How the network predicts an image: an EnsembleSpec, a TileSpec, a FrameWindowSpec (None: not asked for), "raw" or "ema" weights, and
    whether the band's FuseNet is applied to the stitched image (True; None: not asked for)."""
    ensemble: object = None
    tiles: object = None
    windows: object = None
    weights: str = "raw"
    fuse: object = None


def add_inference_args(p, where=""):
    """The ten flags of the network's inference options, and --gemm-route, a switch of the engine the network runs on (it stays in the parse result, opt.gemm_route,
    for load_model: it is no option of the prediction); `where` goes before the help of those that switch something on."""
    p.add_argument("--ensemble", type=str, default="none", choices=("none", "d8"), help=where + "test-time self-ensemble: d8 = the mean over the 4 quarter "
                   "turns x 2 flips of every patch (8 forward passes per patch); none = the plain prediction")
    p.add_argument("--ensemble-permute", type=int, default=0, help="with --ensemble d8: P further frame orders, crossed with the 8 geometric variants "
                   "(8 (P + 1) members, at most 256)")
    p.add_argument("--ensemble-seed", type=int, default=0, help="seed of the frame orders: the same seed gives the same images")
    p.add_argument("--tile-stride", type=int, default=0, help=where + "predict overlapping tiles at this LR stride and blend them on the device "
                   "(it must divide 128 - patch_size and be at most patch_size; 8 = 3.5 x the forward passes); 0 = disjoint patches placed side by side")
    p.add_argument("--tile-window", type=str, default=None, choices=("hat", "box"), help="with --tile-stride: the blend window (default hat)")
    p.add_argument("--frame-windows", type=int, default=0, help=where + "predict W images per tile, each from another window of num_low_res_imgs "
                   "frames slid over the tile's frames sorted from clearest to dirtiest, and write their weighted mean (W forward passes per "
                   "tile; needs num_low_res_imgs_pre > num_low_res_imgs at preprocessing time); 0 = off")
    p.add_argument("--frame-window-step", type=int, default=None, help="with --frame-windows: positions of the sorted frame list between two windows (default 1)")
    p.add_argument("--frame-window-weights", type=str, default=None, choices=WEIGHTS, help="with --frame-windows: weigh every window by the clear "
                   "pixels of its frames (clear, default) or equally (uniform)")
    p.add_argument("--weights", type=str, default="raw", choices=("raw", "ema"), help=where + "which weights of the checkpoint to predict with: raw (default) or "
                   "the moving average a run with train.py --ema-momentum saved; ema on a checkpoint without one is an error")
    p.add_argument("--fuse", action="store_true", help=where + "apply the band's latest FuseNet checkpoint (train.py --modelType fusionNet) to the "
                   "stitched, rounded image on the device, then clip to 0..65535 and round half to even")
    p.add_argument("--gemm-route", dest="gemm_route", action="store_true", help=where + "the engine's general matrix route (WDSRModel.set_gemm_route): "
                   "launches that would run the generic VALU kernels -- a cfg whose num_filters, exp_rate or decay_rate are not the shipped ones -- run on "
                   "the fp32-input MFMA instead; any checkpoint, results equal to fp32 rounding")
    p.add_argument("--gemm-pair", dest="gemm_pair", action="store_true", help=where + "with --gemm-route: the route's fused pointwise pair "
                   "(WDSRModel.set_gemm_pair): a block's expConv, ReLU and decConv in one launch, the hidden tensor never in memory; the same bits")
    p.add_argument("--gemm-x6", dest="gemm_x6", action="store_true", help=where + "with --gemm-route: the route's convolution launches (forward, backward-data) on the 16-bit matrix pipe "
                   "(WDSRModel.set_gemm_x6): six bf16 piece products per fp32 product; results equal to rounding")
    p.add_argument("--gemm-exotic", dest="gemm_exotic", action="store_true", help=where + "with --gemm-route: the 19-frame reducer's 5x5x5 and mirrored-pad launches on the route's "
                   "kernels (WDSRModel.set_gemm_exotic) instead of the generic VALU kernels; a cfg of 7, 9 or 13 frames has none")


def inference_options(p, opt, applies=True, needs=""):
    """The parser errors of the ten flags (`p`: the ArgumentParser, `opt`: its result, with .cfg) -> InferenceOptions, also left in
    opt.inference.  --tile-window, --frame-window-step and --frame-window-weights are resolved to their defaults in `opt`; opt.windows is the
    FrameWindowSpec or None.  applies=False: the script is not predicting with the network, and a flag that switches an option on is an error
    naming `needs`, the flag that would make it predict."""
    if not applies:
        for given, flag in ((opt.ensemble != "none", "--ensemble"), (opt.weights != "raw", "--weights"), (opt.tile_stride != 0, "--tile-stride"),
                            (opt.frame_windows != 0, "--frame-windows"), (opt.fuse, "--fuse"), (opt.gemm_route, "--gemm-route"), (opt.gemm_pair, "--gemm-pair"),
                            (opt.gemm_x6, "--gemm-x6"), (opt.gemm_exotic, "--gemm-exotic")):
            if given:
                p.error("%s applies to %s (a folder of PNGs is scored as it is)" % (flag, needs))
    if opt.gemm_pair and not opt.gemm_route:
        p.error("--gemm-pair needs --gemm-route")
    if opt.gemm_x6 and not opt.gemm_route:
        p.error("--gemm-x6 needs --gemm-route")
    if opt.gemm_exotic and not opt.gemm_route:
        p.error("--gemm-exotic needs --gemm-route")
    if opt.ensemble == "none" and opt.ensemble_permute:
        p.error("--ensemble-permute needs --ensemble d8")
    if opt.tile_stride == 0 and opt.tile_window is not None:
        p.error("--tile-window needs --tile-stride")
    if opt.frame_windows == 0 and opt.frame_window_step is not None:
        p.error("--frame-window-step needs --frame-windows")
    if opt.frame_windows == 0 and opt.frame_window_weights is not None:
        p.error("--frame-window-weights needs --frame-windows")
    ensemble = tiles = windows = config = None
    if opt.ensemble != "none":
        ensemble = EnsembleSpec(opt.ensemble, permute=opt.ensemble_permute, seed=opt.ensemble_seed)
    if opt.tile_stride or opt.frame_windows:
        from .parseConfig import parseConfig
        try:
            config = parseConfig(opt.cfg)
        except OSError as e:
            p.error("%s: cannot read --cfg: %s" % ("--tile-stride" if opt.tile_stride else "--frame-windows", e))
    if opt.tile_stride:
        opt.tile_window = opt.tile_window or "hat"
        try:
            tiles = TileSpec(opt.tile_stride, opt.tile_window).validate(config["patch_size"], LR_SIZE)
        except ValueError as e:
            p.error("--tile-stride: %s" % e)
    if opt.frame_windows:
        opt.frame_window_step = 1 if opt.frame_window_step is None else opt.frame_window_step
        opt.frame_window_weights = opt.frame_window_weights or "clear"
        try:
            windows = FrameWindowSpec(opt.frame_windows, opt.frame_window_step, opt.frame_window_weights)
            if "num_low_res_imgs_pre" not in config:
                raise ValueError("the cfg has no num_low_res_imgs_pre: the pool of registered frames the windows slide over")
            windows.validate(config["num_low_res_imgs_pre"], config["num_low_res_imgs"], config)
        except ValueError as e:
            p.error("--frame-windows: %s" % e)
    opt.windows = windows
    opt.inference = InferenceOptions(ensemble, tiles, windows, opt.weights, True if opt.fuse else None)
    return opt.inference


def load_model(config, cfg_path, band, weights, who, gemm_route=False, gemm_pair=False, gemm_x6=False, gemm_exotic=False):
    """The cfg's network on the device with its latest checkpoint restored (`weights`: "raw" or "ema") -> (model, trainer).  `who` names the
    command in the error of a checkpoint without an "ema" entry.  gemm_route: the engine's general matrix route (--gemm-route); gemm_pair: its fused pointwise pair (--gemm-pair);
    gemm_x6: its convolution launches in x6 arithmetic (--gemm-x6); gemm_exotic: the 19-frame reducer's exotic launches on the route (--gemm-exotic)."""
    from .modelsTF import WDSRConv3D
    from .trainClass import ModelTrainer
    mean, std = BAND_STATS["NIR" if band == "NIR" else "RED"]
    k = config["kernel_size"]
    model = WDSRConv3D(name="superResolutionNet", band=band, mean=mean, std=std, maxShift=config["max_shift"]).build(
        scale=config["scale"], numFilters=config["num_filters"], kernelSize=(k, k, k), numResBlocks=config["num_res_blocks"],
        expRate=config["exp_rate"], decayRate=config["decay_rate"], numImgLR=config["num_low_res_imgs"],
        patchSizeLR=config["patch_size"], isGrayScale=config["is_grayscale"]).to("cuda")
    if gemm_route:
        model.set_gemm_route(True)
    if gemm_pair:
        model.set_gemm_pair(True)
    if gemm_x6:
        model.set_gemm_x6(True)
    if gemm_exotic:
        model.set_gemm_exotic(True)
    basename = os.path.basename(cfg_path).split(".")[0]
    try:
        trainer = ModelTrainer(model, None, None, None, os.path.join(config["model_out"], "ckpt_%s" % basename, band),
                               os.path.join(config["model_out"], "logs_%s" % basename, band), weights=weights)   # restores the latest checkpoint
    except ValueError as exc:
        if weights != "ema":
            raise
        raise SystemExit("%s --weights ema: %s" % (who, exc))
    return model, trainer


def load_inputs(config, split, band, options):
    """What `predict` takes: the registered frames of trimmedArrayDir/<split>imgLR_<band>.npy (masked [sets, T_pre, 1, H, H]) when tiles or
    frame windows are asked for, else the patches of resolverDir/<split>patchesLR_<band>.npy as [sets, 64, 22, 22, T, 1] (test.py:38)."""
    if options.tiles is not None or options.windows is not None:
        return np.load(os.path.join(config["preprocessing_out"], "trimmedArrayDir", "%simgLR_%s.npy" % (split, band)), allow_pickle=True)
    patchLR = np.load(os.path.join(config["preprocessing_out"], "resolverDir", "%spatchesLR_%s.npy" % (split, band)), allow_pickle=True)
    return np.array(patchLR).transpose((0, 1, 4, 5, 2, 3))


def predict(model, inputs, options, config, micro_batch=2048, launch_batch=None):
    """The images of `load_inputs`' array under `options`: a list of [G, G, 1] float64 arrays, one per image set (testClass.evaluate_device's
    form).  `micro_batch` and `launch_batch` are those of the plain prediction; the options choose their own launch sets."""
    from . import testClass
    if options.windows is not None:
        return testClass.evaluate_windowed_frames(model, inputs, options.windows, config, tiles=options.tiles, ensemble=options.ensemble)
    if options.tiles is not None:
        return testClass.evaluate_tiled_frames(model, inputs, options.tiles, config, ensemble=options.ensemble)
    if options.ensemble is not None:
        return testClass.evaluate_device(model, inputs, ensemble=options.ensemble, final="round")
    return testClass.evaluate_device(model, inputs, micro_batch=micro_batch, launch_batch=launch_batch)


def fuse_ckpt_dir(config, cfg_path, band):
    """Where train.py --modelType fusionNet keeps a band's checkpoints: <model_out>/fuseNetCkpt_<cfg>/<band>."""
    return os.path.join(config["model_out"], "fuseNetCkpt_%s" % os.path.basename(cfg_path).split(".")[0], band)


def load_fusenet(config, cfg_path, band, who):
    """The band's FuseNet on the device with its latest checkpoint restored -> model.  No checkpoint: SystemExit naming the directory looked in."""
    import glob
    from .modelsTF import FuseNetConv2D
    from .trainClass import ModelTrainer
    ckpt = fuse_ckpt_dir(config, cfg_path, band)
    if not (os.path.exists(os.path.join(ckpt, "checkpoint.pt-index")) or glob.glob(os.path.join(ckpt, "ckpt-*.pt"))):      # (asked before ModelTrainer makes the directory)
        raise SystemExit("%s: no FuseNet checkpoint under %s (train one with train.py --modelType fusionNet)" % (who, ckpt))
    model = FuseNetConv2D(name="fusionNet", band=band).build().to("cuda")
    ModelTrainer(model, None, None, None, ckpt, os.path.join(config["model_out"], "fuseNetLogs_%s" % os.path.basename(cfg_path).split(".")[0], band))
    return model


def fuse_images(images, config, cfg_path, band, who, batch=16):
    """--fuse: the band's FuseNet applied to the stitched, rounded images (a list of [G, G, 1] arrays, `predict`'s form) on the device, the
    result clipped to 0..65535 and rounded half to even -> the same form."""
    import torch
    model = load_fusenet(config, cfg_path, band, who)
    out = []
    with torch.no_grad():
        for k in range(0, len(images), batch):
            x = torch.as_tensor(np.stack([np.asarray(im)[:, :, 0] for im in images[k:k + batch]]).astype(np.float32)).to("cuda")
            y = torch.ops.probav.clip_round(model(x), 0.0, 65535.0)
            out += [a[:, :, None] for a in y.cpu().double().numpy()]
    return out


def numbered(images, split, band, directory="."):
    """(id, image) for every image in order: ids count up from the first of the split ("TEST", else TRAIN) and band ("NIR", else RED) and
    skip those of <directory>/removedTrainSets<BAND>.txt, as the reference's test.py:79-100 names its PNGs."""
    from .scoring import read_removed
    band = band.upper()
    omit = set(read_removed(band, directory))
    i = FIRST_ID[("TEST" if split == "TEST" else "TRAIN", "NIR" if band == "NIR" else "RED")]
    for img in images:
        while i in omit:
            i += 1
        yield i, img
        i += 1
