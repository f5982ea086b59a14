#!/usr/bin/env python3
"""Score super-resolved train images by the ESA PROBA-V measure (the reference's evaluate.py:17-87, which was left unfinished).

    python evaluate.py --cfg C --toCompare DIR [--benchmark DIR] [--band NIR|RED|both] [--norm PATH] [--formula esa|reference] [--out DIR]
    python evaluate.py --cfg C --band NIR --model          # the cfg's latest checkpoint on the TRAIN sets, no PNGs written
    python evaluate.py --cfg C --band NIR --model --ensemble d8 [--ensemble-permute P --ensemble-seed s]     # ... its test-time self-ensemble
    python evaluate.py --cfg C --band NIR --model --tile-stride 8 [--tile-window hat|box]                    # ... its overlapped, blended tiles
    python evaluate.py --cfg C --band NIR --model --frame-windows 3 [--frame-window-step s --frame-window-weights clear|uniform]   # ... its frame-window ensemble
    python evaluate.py --cfg C --band NIR --model --weights ema                                              # ... its EMA weights (train.py --ema-momentum)
    python evaluate.py --cfg C --band NIR --model --fuse                                                     # ... with the band's FuseNet applied to the stitched image
    python evaluate.py --cfg C --band NIR --baseline [--baseline-mode esa|clear] [--baseline-frames raw|registered]   # the bicubic-mean baseline, no checkpoint
    python evaluate.py --cfg C --band NIR --model --benchmark-baseline                                       # the checkpoint against that baseline
    python evaluate.py --cfg C --band NIR --model --norm computed                                            # N_i from the esa / raw baseline (a stand-in for norm.csv)
    python evaluate.py --cfg C --band NIR --model --metrics cpsnr,cssim                                      # ... the cSSIM of the literature beside the cPSNR

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

--metrics cpsnr,cssim adds the shift-compensated SSIM published beside the cPSNR (proba-v_amd/scoring.py, on the device): per image its maximum
over the 49 shifts with that shift (cssim, su, sv) and the SSIM at the cPSNR's own shift (cssim_at_cpsnr_shift), their means in the JSON line; it works with
every source and inference flag above.  --formula does not affect it (HR is always masked there), and norm.csv has no SSIM counterpart: no cSSIM score.

Prints one JSON line; writes <out>/scores.csv and, when matplotlib imports and there is a --benchmark, <out>/comparison.png.
"""
import argparse
import contextlib
import logging
import os
import sys

import numpy as np

from probav_amd import scoring
from probav_amd.inference import InferenceOptions, add_inference_args, fuse_images, inference_options, load_inputs, load_model, numbered, predict

logging.basicConfig(format="%(asctime)s - %(message)s", level=logging.INFO, stream=sys.stderr)
logger = logging.getLogger("probav_amd")


def parser(argv=None):
    p = argparse.ArgumentParser(description="Score super-resolved PROBA-V train images by the ESA cPSNR")
    p.add_argument("--cfg", type=str, default="cfg/p16t12c85r12pre19.cfg")
    p.add_argument("--toCompare", type=str, default=None, help="folder of imgsetNNNN.png to score")
    p.add_argument("--benchmark", type=str, default=None, help="folder of imgsetNNNN.png to compare against")
    p.add_argument("--band", type=str, default="both", help="NIR, RED or both")
    p.add_argument("--norm", type=str, default=None, help="norm.csv (default: <raw_data>/norm.csv if present), or `computed`: N_i = the cPSNR of "
                   "this repository's own esa / raw bicubic-mean baseline (a stand-in: ESA's file was made with another interpolator)")
    p.add_argument("--formula", type=str, default="esa", choices=("esa", "reference"), help="the cPSNR's formula; it does not affect cSSIM, "
                   "where HR is always masked")
    p.add_argument("--metrics", type=str, default="cpsnr", help="cpsnr (default) or cpsnr,cssim: also the shift-compensated SSIM of every image "
                   "(extra CSV columns and JSON keys; --formula does not affect it)")
    p.add_argument("--model", action="store_true", help="score the cfg's latest checkpoint on resolverDir/TRAINpatchesLR_<band>.npy")
    p.add_argument("--out", type=str, default=".", help="folder for scores.csv and comparison.png")
    add_inference_args(p, "with --model: ")
    p.add_argument("--baseline", action="store_true", help="score the bicubic-mean baseline of the band's TRAIN sets (probav_amd/baseline.py); "
                   "no checkpoint, no PNGs written")
    p.add_argument("--benchmark-baseline", action="store_true", help="with --model: compare against the bicubic-mean baseline instead of a "
                   "--benchmark folder")
    from probav_amd.baseline import add_cli_args, cli_spec
    add_cli_args(p)
    p.add_argument("--border", type=int, default=3, help=argparse.SUPPRESS)
    opt = p.parse_args(argv)
    opt.band = opt.band.upper()
    try:
        opt.metrics = scoring.check_metrics(m.strip() for m in opt.metrics.split(","))
    except ValueError as e:
        p.error("--metrics: %s" % e)
    if opt.band not in ("NIR", "RED", "BOTH"):
        p.error("--band must be NIR, RED or both, got %r" % opt.band)
    if int(opt.model) + int(opt.toCompare is not None) + int(opt.baseline) != 1:
        p.error("give exactly one of --toCompare DIR, --model and --baseline")
    if opt.benchmark_baseline and not opt.model:
        p.error("--benchmark-baseline applies to --model")
    if opt.benchmark_baseline and opt.benchmark is not None:
        p.error("give at most one of --benchmark DIR and --benchmark-baseline")
    opt.baseline_spec = cli_spec(p, opt, opt.baseline or opt.benchmark_baseline, "--baseline or --benchmark-baseline")
    for name in ("toCompare", "benchmark"):
        d = getattr(opt, name)
        if d is not None and not os.path.isdir(d):
            p.error("--%s: no such folder %r" % (name, d))
    if opt.norm is not None and opt.norm != "computed" and not os.path.isfile(opt.norm):
        p.error("--norm: no such file %r" % opt.norm)
    if not os.path.isfile(opt.cfg):
        p.error("--cfg: no such file %r" % opt.cfg)
    inference_options(p, opt, applies=opt.model, needs="--model")
    if not 0 <= opt.border <= 3:
        p.error("--border must be in 0..3")
    return opt


def model_images(config, cfg_path, band, options=InferenceOptions(), gemm_route=False, gemm_pair=False, gemm_x6=False, gemm_exotic=False):
    """{id: uint16 image} of the latest checkpoint on the band's TRAIN sets: test.py's main with --totest TRAIN and the same `options` (an
    InferenceOptions: the self-ensemble, the blended overlapping tiles, the frame windows, the raw or EMA weights), without the PNGs.  gemm_route: --gemm-route, the engine's general matrix route; gemm_pair: --gemm-pair, its fused pointwise pair; gemm_x6: --gemm-x6, its convolution launches in x6 arithmetic; gemm_exotic: --gemm-exotic, the 19-frame reducer's exotic launches on the route."""
    import torch
    inputs = load_inputs(config, "TRAIN", band, options)
    with contextlib.redirect_stdout(sys.stderr):            # the restore messages: stdout carries the JSON line only
        model, trainer = load_model(config, cfg_path, band, options.weights, "evaluate.py --model", gemm_route=gemm_route, gemm_pair=gemm_pair, gemm_x6=gemm_x6, gemm_exotic=gemm_exotic)
    if trainer.latest_checkpoint is None and trainer._tf_latest() is None:
        raise SystemExit("evaluate.py --model: no checkpoint under %s" % trainer.ckptDir)
    y_preds = predict(model, inputs, options, config)
    del model, trainer
    torch.cuda.empty_cache()
    if options.fuse:
        with contextlib.redirect_stdout(sys.stderr):
            y_preds = fuse_images(y_preds, config, cfg_path, band, "evaluate.py --model --fuse")
    return {i: img[:, :, 0].astype(np.uint16) for i, img in numbered(y_preds, "TRAIN", band)}      # test.py's cast, a pixel clipped to 65536 included


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
                                                       removed=removed, metrics=opt.metrics)
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
        images = {}
        for b in bands:
            images.update(model_images(config, opt.cfg, b, opt.inference, gemm_route=opt.gemm_route, gemm_pair=opt.gemm_pair, gemm_x6=opt.gemm_x6, gemm_exotic=opt.gemm_exotic))
    else:
        images = scoring.load_sr_dir(opt.toCompare)
    if not opt.baseline:
        rows, counts = scoring.score_images(images, hr, border=opt.border, formula=opt.formula, removed=removed, metrics=opt.metrics)
    bench_rows = None
    if opt.benchmark_baseline:
        bench_rows = baseline_scored(opt.baseline_spec)[0]
    elif opt.benchmark is not None:
        bench_rows, _ = scoring.score_images(scoring.load_sr_dir(opt.benchmark), hr, border=opt.border, formula=opt.formula, removed=removed,
                                             metrics=opt.metrics)
    summary = scoring.summarize(rows, counts, norm=norm, bench_rows=bench_rows, metrics=opt.metrics)
    summary["formula"] = opt.formula
    if opt.metrics != ("cpsnr",):
        summary["metrics"] = list(opt.metrics)
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
    scoring.write_csv(os.path.join(opt.out, "scores.csv"), rows, norm=norm, bench_rows=bench_rows, metrics=opt.metrics)
    if bench_rows is not None:
        if scoring.plot_comparison(os.path.join(opt.out, "comparison.png"), rows, bench_rows):
            summary["comparison_png"] = os.path.join(opt.out, "comparison.png")
        else:
            logger.info("matplotlib does not import: comparison.png not written")
    print(scoring.json_line(summary), flush=True)
    return summary


if __name__ == "__main__":
    main(parser())
