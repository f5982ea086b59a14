#!/usr/bin/env python3
"""Score super-resolved train images by the ESA PROBA-V measure (the reference's evaluate.py:17-87, which was left unfinished).

    python evaluate.py --cfg C --toCompare DIR [--benchmark DIR] [--band NIR|RED|both] [--norm PATH] [--formula esa|reference] [--out DIR]
    python evaluate.py --cfg C --band NIR --model          # the cfg's latest checkpoint on the TRAIN sets, no PNGs written
    python evaluate.py --cfg C --band NIR --model --ensemble d8 [--ensemble-permute P --ensemble-seed s]     # ... its test-time self-ensemble
    python evaluate.py --cfg C --band NIR --model --tile-stride 8 [--tile-window hat|box]                    # ... its overlapped, blended tiles
    python evaluate.py --cfg C --band NIR --model --frame-windows 3 [--frame-window-step s --frame-window-weights clear|uniform]   # ... its frame-window ensemble
    python evaluate.py --cfg C --band NIR --model --weights ema                                              # ... its EMA weights (train.py --ema-momentum)
    python evaluate.py --cfg C --band NIR --baseline [--baseline-mode esa|clear] [--baseline-frames raw|registered]   # the bicubic-mean baseline, no checkpoint
    python evaluate.py --cfg C --band NIR --model --benchmark-baseline                                       # the checkpoint against that baseline
    python evaluate.py --cfg C --band NIR --model --norm computed                                            # N_i from the esa / raw baseline (a stand-in for norm.csv)

--toCompare scores the imgsetNNNN.png of a folder (test.py's output) against resolverDir/TRAINimgHR_<band>.npy, matching by id: train ids
below 594 are RED, 594 .. 1159 NIR, ids from 1160 are test sets (no HR: counted, skipped).  --model resolves resolverDir/TRAINpatchesLR_<band>.npy
with the latest checkpoint exactly as `test.py --totest TRAIN` does (same ids, removedTrainSets<BAND>.txt skipped, the same uint16 cast) and
scores the images on the device; with --ensemble d8 the images are the self-ensemble `test.py --ensemble d8` writes (same three flags,
probav_amd/ensemble.py), so a checkpoint is scored with and without it in one place; with --tile-stride s the images are the blended overlapping
tiles `test.py --tile-stride s` writes (read from trimmedArrayDir/TRAINimgLR_<band>.npy, same set order and ids; probav_amd/tiles.py); with --frame-windows W
they are the frame-window ensemble `test.py --frame-windows W` writes (the same file and flags; probav_amd/frame_windows.py).  The metric (proba-v_amd/scoring.py) is the ESA shift-compensated clear PSNR; --formula reference gives
Losses.shiftCompensatedcPSNR instead (HR unmasked, what the reference's script computes).  The score is mean(N_i / cPSNR_i) with N_i from
norm.csv (default <raw_data>/norm.csv when present; lower is better).  --baseline scores the competition's bicubic-mean baseline of the band's
TRAIN sets (probav_amd/baseline.py; no checkpoint, no PNGs), --benchmark-baseline compares --model against it instead of a --benchmark folder, and
--norm computed takes N_i from the esa / raw baseline's own cPSNR: a stand-in, since ESA's norm.csv was made with another interpolator
(INTEGRATION.md).  The JSON line says where the norm came from: "norm_source": "file", "computed" or null.

Prints one JSON line; writes <out>/scores.csv and, when matplotlib imports and there is a --benchmark, <out>/comparison.png.
"""
import argparse
import contextlib
import logging
import os
import sys

import numpy as np

from probav_amd import scoring

logging.basicConfig(format="%(asctime)s - %(message)s", level=logging.INFO, stream=sys.stderr)
logger = logging.getLogger("probav_amd")

BAND_STATS = {"NIR": (8075.2045, 3160.7272), "RED": (5266.2245, 3431.8614)}      # test.py


def parser(argv=None):
    p = argparse.ArgumentParser(description="Score super-resolved PROBA-V train images by the ESA cPSNR")
    p.add_argument("--cfg", type=str, default="cfg/p16t12c85r12pre19.cfg")
    p.add_argument("--toCompare", type=str, default=None, help="folder of imgsetNNNN.png to score")
    p.add_argument("--benchmark", type=str, default=None, help="folder of imgsetNNNN.png to compare against")
    p.add_argument("--band", type=str, default="both", help="NIR, RED or both")
    p.add_argument("--norm", type=str, default=None, help="norm.csv (default: <raw_data>/norm.csv if present), or `computed`: N_i = the cPSNR of "
                   "this repository's own esa / raw bicubic-mean baseline (a stand-in: ESA's file was made with another interpolator)")
    p.add_argument("--formula", type=str, default="esa", choices=("esa", "reference"))
    p.add_argument("--model", action="store_true", help="score the cfg's latest checkpoint on resolverDir/TRAINpatchesLR_<band>.npy")
    p.add_argument("--out", type=str, default=".", help="folder for scores.csv and comparison.png")
    p.add_argument("--ensemble", type=str, default="none", choices=("none", "d8"), help="with --model: score the test-time self-ensemble "
                   "(d8 = the mean over 4 quarter turns x 2 flips of every patch), as test.py --ensemble writes it")
    p.add_argument("--ensemble-permute", type=int, default=0, help="with --ensemble d8: P further frame orders (8 (P + 1) members, at most 256)")
    p.add_argument("--ensemble-seed", type=int, default=0, help="seed of the frame orders")
    p.add_argument("--tile-stride", type=int, default=0, help="with --model: score the blend of overlapping tiles at this LR stride, as "
                   "test.py --tile-stride writes it; 0 = disjoint patches")
    p.add_argument("--tile-window", type=str, default=None, choices=("hat", "box"), help="with --tile-stride: the blend window (default hat)")
    from probav_amd.frame_windows import add_cli_args as add_window_args, cli_window_args
    add_window_args(p, "with --model: ")
    p.add_argument("--weights", type=str, default="raw", choices=("raw", "ema"), help="with --model: score the checkpoint's raw weights (default) or "
                   "the moving average saved by train.py --ema-momentum; ema on a checkpoint without one is an error")
    p.add_argument("--baseline", action="store_true", help="score the bicubic-mean baseline of the band's TRAIN sets (probav_amd/baseline.py); "
                   "no checkpoint, no PNGs written")
    p.add_argument("--benchmark-baseline", action="store_true", help="with --model: compare against the bicubic-mean baseline instead of a "
                   "--benchmark folder")
    from probav_amd.baseline import add_cli_args, cli_spec
    add_cli_args(p)
    p.add_argument("--border", type=int, default=3, help=argparse.SUPPRESS)
    opt = p.parse_args(argv)
    opt.band = opt.band.upper()
    if opt.band not in ("NIR", "RED", "BOTH"):
        p.error("--band must be NIR, RED or both, got %r" % opt.band)
    if int(opt.model) + int(opt.toCompare is not None) + int(opt.baseline) != 1:
        p.error("give exactly one of --toCompare DIR, --model and --baseline")
    if opt.benchmark_baseline and not opt.model:
        p.error("--benchmark-baseline applies to --model")
    if opt.benchmark_baseline and opt.benchmark is not None:
        p.error("give at most one of --benchmark DIR and --benchmark-baseline")
    opt.baseline_spec = cli_spec(p, opt, opt.baseline or opt.benchmark_baseline, "--baseline or --benchmark-baseline")
    if opt.ensemble != "none" and not opt.model:
        p.error("--ensemble applies to --model (a folder of PNGs is scored as it is)")
    if opt.ensemble == "none" and opt.ensemble_permute:
        p.error("--ensemble-permute needs --ensemble d8")
    if opt.weights != "raw" and not opt.model:
        p.error("--weights applies to --model (a folder of PNGs is scored as it is)")
    if opt.tile_stride and not opt.model:
        p.error("--tile-stride applies to --model (a folder of PNGs is scored as it is)")
    for name in ("toCompare", "benchmark"):
        d = getattr(opt, name)
        if d is not None and not os.path.isdir(d):
            p.error("--%s: no such folder %r" % (name, d))
    if opt.norm is not None and opt.norm != "computed" and not os.path.isfile(opt.norm):
        p.error("--norm: no such file %r" % opt.norm)
    if not os.path.isfile(opt.cfg):
        p.error("--cfg: no such file %r" % opt.cfg)
    from probav_amd.tiles import cli_tile_args
    cli_tile_args(p, opt)
    if opt.frame_windows and not opt.model:
        p.error("--frame-windows applies to --model (a folder of PNGs is scored as it is)")
    opt.windows = cli_window_args(p, opt)
    if not 0 <= opt.border <= 3:
        p.error("--border must be in 0..3")
    return opt


def model_images(config, cfg_path, band, ensemble=None, tiles=None, weights="raw", windows=None):
    """{id: uint16 image} of the latest checkpoint on the band's TRAIN sets: test.py's main with --totest TRAIN, without the PNGs.
    ensemble: an EnsembleSpec for the self-ensemble images test.py --ensemble writes (None: the plain prediction).
    tiles: a TileSpec for the blended overlapping tiles test.py --tile-stride writes (None: disjoint patches).
    weights: "raw" or "ema" -- the checkpoint entry test.py --weights predicts with.
    windows: a FrameWindowSpec for the frame-window ensemble test.py --frame-windows writes (None: one prediction per tile)."""
    import torch
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.testClass import evaluate_device, evaluate_tiled_frames, evaluate_windowed_frames
    from probav_amd.trainClass import ModelTrainer
    if tiles is not None or windows is not None:
        framesLR = np.load(os.path.join(config["preprocessing_out"], "trimmedArrayDir", "TRAINimgLR_%s.npy" % band), allow_pickle=True)
    else:
        dataDir = os.path.join(config["preprocessing_out"], "resolverDir")
        patchLR = np.load(os.path.join(dataDir, "TRAINpatchesLR_%s.npy" % band), allow_pickle=True)
        patchLR = np.array(patchLR).transpose((0, 1, 4, 5, 2, 3))
    mean, std = BAND_STATS[band]
    k = config["kernel_size"]
    model = WDSRConv3D(name="superResolutionNet", band=band, mean=mean, std=std, maxShift=config["max_shift"]).build(
        scale=config["scale"], numFilters=config["num_filters"], kernelSize=(k, k, k), numResBlocks=config["num_res_blocks"],
        expRate=config["exp_rate"], decayRate=config["decay_rate"], numImgLR=config["num_low_res_imgs"],
        patchSizeLR=config["patch_size"], isGrayScale=config["is_grayscale"]).to("cuda")
    basename = os.path.basename(cfg_path).split(".")[0]
    ckptDir = os.path.join(config["model_out"], "ckpt_%s" % basename, band)
    with contextlib.redirect_stdout(sys.stderr):            # the restore messages: stdout carries the JSON line only
        try:
            trainer = ModelTrainer(model, None, None, None, ckptDir, os.path.join(config["model_out"], "logs_%s" % basename, band), weights=weights)
        except ValueError as exc:
            if weights != "ema":
                raise
            raise SystemExit("evaluate.py --model --weights ema: %s" % exc)
    if trainer.latest_checkpoint is None and trainer._tf_latest() is None:
        raise SystemExit("evaluate.py --model: no checkpoint under %s" % ckptDir)
    if windows is not None:
        y_preds = evaluate_windowed_frames(model, framesLR, windows, config, tiles=tiles, ensemble=ensemble)
    elif tiles is not None:
        y_preds = evaluate_tiled_frames(model, framesLR, tiles, config, ensemble=ensemble)
    else:
        y_preds = evaluate_device(model, patchLR) if ensemble is None else evaluate_device(model, patchLR, ensemble=ensemble, final="round")
    del model, trainer
    torch.cuda.empty_cache()
    toOmit = scoring.read_removed(band)
    out, i = {}, scoring.FIRST_TRAIN_ID[band]
    for img in y_preds:
        while i in toOmit:
            i += 1
        out[i] = img[:, :, 0].astype(np.uint16)            # test.py's cast, a pixel clipped to 65536 included
        i += 1
    return out


def baseline_train_images(config, bands, spec):
    """{id: uint16 image} of the bicubic-mean baseline on the TRAIN sets of `bands` (probav_amd/baseline.py)."""
    from probav_amd import baseline
    out = {}
    for b in bands:
        imgs, ids = baseline.baseline_images(config, b, "TRAIN", spec)
        out.update(zip(ids, imgs))
    return out


def main(opt):
    from probav_amd.parseConfig import parseConfig
    config = parseConfig(opt.cfg)
    bands = scoring.BANDS if opt.band == "BOTH" else (opt.band,)
    norm_path = opt.norm
    if norm_path is None:
        cand = os.path.join(config.get("raw_data", ""), "norm.csv")
        norm_path = cand if config.get("raw_data") and os.path.isfile(cand) else None
    hr = {b: scoring.load_hr(config, b) for b in bands}
    removed = {b: scoring.read_removed(b) for b in bands}
    baseline_rows = {}                                      # BaselineSpec -> scored rows: one baseline serves --baseline, the benchmark and the norm

    def baseline_scored(spec):
        if spec not in baseline_rows:
            baseline_rows[spec] = scoring.score_images(baseline_train_images(config, bands, spec), hr, border=opt.border, formula=opt.formula,
                                                       removed=removed)
        return baseline_rows[spec]

    if norm_path == "computed":
        from probav_amd.baseline import BaselineSpec
        norm = {r["id"]: r["cpsnr"] for r in baseline_scored(BaselineSpec("esa", "raw"))[0]}
    else:
        norm = scoring.read_norm(norm_path) if norm_path else None
    norm_source = None if norm is None else ("computed" if norm_path == "computed" else "file")
    if opt.baseline:
        rows, counts = baseline_scored(opt.baseline_spec)
    elif opt.model:
        spec = None
        if opt.ensemble != "none":
            from probav_amd.ensemble import EnsembleSpec
            spec = EnsembleSpec(opt.ensemble, permute=opt.ensemble_permute, seed=opt.ensemble_seed)
        tiles = None
        if opt.tile_stride:
            from probav_amd.tiles import TileSpec
            tiles = TileSpec(opt.tile_stride, opt.tile_window)
        images = {}
        for b in bands:
            images.update(model_images(config, opt.cfg, b, ensemble=spec, tiles=tiles, weights=opt.weights, windows=getattr(opt, "windows", None)))
    else:
        images = scoring.load_sr_dir(opt.toCompare)
    if not opt.baseline:
        rows, counts = scoring.score_images(images, hr, border=opt.border, formula=opt.formula, removed=removed)
    bench_rows = None
    if opt.benchmark_baseline:
        bench_rows = baseline_scored(opt.baseline_spec)[0]
    elif opt.benchmark is not None:
        bench_rows, _ = scoring.score_images(scoring.load_sr_dir(opt.benchmark), hr, border=opt.border, formula=opt.formula, removed=removed)
    summary = scoring.summarize(rows, counts, norm=norm, bench_rows=bench_rows)
    summary["formula"] = opt.formula
    if opt.ensemble != "none":
        summary["ensemble"] = {"geometry": opt.ensemble, "permute": opt.ensemble_permute, "seed": opt.ensemble_seed}
    if opt.weights != "raw":
        summary["weights"] = opt.weights
    if opt.tile_stride:
        summary["tiles"] = {"stride": opt.tile_stride, "window": opt.tile_window}
    if getattr(opt, "windows", None) is not None:
        summary["frame_windows"] = {"windows": opt.windows.windows, "step": opt.windows.step, "weights": opt.windows.weights}
    if opt.baseline_spec is not None:
        summary["baseline"] = {"mode": opt.baseline_spec.mode, "frames": opt.baseline_spec.frames}
    summary["norm"] = norm_path
    summary["norm_source"] = norm_source
    os.makedirs(opt.out, exist_ok=True)
    scoring.write_csv(os.path.join(opt.out, "scores.csv"), rows, norm=norm, bench_rows=bench_rows)
    if bench_rows is not None:
        if scoring.plot_comparison(os.path.join(opt.out, "comparison.png"), rows, bench_rows):
            summary["comparison_png"] = os.path.join(opt.out, "comparison.png")
        else:
            logger.info("matplotlib does not import: comparison.png not written")
    print(scoring.json_line(summary), flush=True)
    return summary


if __name__ == "__main__":
    main(parser())
