#!/usr/bin/env python3
"""Overlapped-tile inference, measured (one process, one JSON line on stdout; --profile PATH also writes the figures as text).

--sets image sets of seeded synthetic registered frames [9, 1, 128, 128] with cloud discs (default 8), a seeded model, every shape warmed up,
then --windows rounds of three legs ALTERNATED in the same process, each window a whole number of calls sized to last longer than --seconds
and closed by a device synchronise:

  plain     testClass.evaluate_device(model, patches)           the 64 disjoint patches of every image (built once, outside the windows, as
                                                                test.py reads them from resolverDir)             -> t_plain per image
  composed  the tiled image from parts that exist without the feature: the builder's unfold copied to the host, pickClearPatchesLR and the
            transpose in numpy, resolve_device in launch sets of LAUNCH_BATCH tiles, one copy back, tile_blend_numpy on the host
  fused     testClass.evaluate_tiled_frames(model, frames, TileSpec(s), config)      (build_tiles -> forward -> tile_blend, one copy back)

The images of the composed and the fused leg are compared at the timed size and must be equal bit for bit (the tool fails otherwise).
Reported: t_fused / ((n^2 / 64) t_plain) -- the forward passes are n^2 / 64 times the plain path's by construction, the figure shows how close the
whole path (tile building included) comes to that --, t_composed over the same, the window-to-window spread of the plain leg, and peak device
memory of one call of each leg.  --kernel-calls N instead runs N fused calls and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the blend kernel's own share; the bytes it must move per call are printed beside it.

    python tools/tile_bench.py [--sets 8] [--stride 8] [--windows 3] [--seconds 1.2] [--profile profiles/tile_ab.txt]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import prep, synth, testClass, tiles  # noqa: E402
from probav_amd.modelsTF import WDSRConv3D  # noqa: E402
from probav_amd.tiles import TileSpec, tile_blend_numpy  # noqa: E402

CONFIG = {"patch_size": 16, "max_shift": 6, "scale": 3, "num_low_res_imgs": 9, "low_res_patch_thresholds": [0.85]}


def synthetic_frames(sets, T=9, H=128, seed=21):
    """Masked float64 [sets, T, 1, H, H] in the form of trimmedArrayDir/<...>imgLR_<band>.npy: smooth scenes plus noise, two or three cloud discs a frame."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :H]
    data = np.empty((sets, T, 1, H, H))
    mask = np.zeros((sets, T, 1, H, H), bool)
    for i in range(sets):
        scene = synth.NIR_MEAN + synth.NIR_STD * np.sin(yy / rng.uniform(5, 20) + rng.uniform(0, 6)) * np.cos(xx / rng.uniform(5, 20))
        for t in range(T):
            data[i, t, 0] = np.rint(np.clip(scene + rng.normal(0, 200, (H, H)), 0, 65535))
            for _ in range(int(rng.integers(2, 4))):
                cy, cx, rad = rng.integers(0, H), rng.integers(0, H), rng.integers(8, 26)
                mask[i, t, 0] |= (yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2
    return np.ma.masked_array(data, mask=mask)


def host_tiles(frames, stride):
    """The tile inputs with the dataset builder's own functions on the host: float32 [sets, n n, 22, 22, T, 1]."""
    patches, _ = prep._patches(frames, CONFIG["patch_size"] + CONFIG["max_shift"], stride, CONFIG["max_shift"] // 2)
    for thr in CONFIG["low_res_patch_thresholds"]:
        patches = prep.pickClearPatchesLR(patches, k=CONFIG["num_low_res_imgs"], clarityThreshold=thr)
    return np.array(patches).transpose((0, 1, 4, 5, 2, 3))


def composed_images(model, frames, spec):
    x = host_tiles(frames, spec.stride)
    n = int(round(x.shape[1] ** 0.5))
    flat = x.reshape((-1,) + x.shape[2:])
    outs = [testClass.resolve_device(model, flat[i:i + testClass.LAUNCH_BATCH]) for i in range(0, len(flat), testClass.LAUNCH_BATCH)]
    members = (torch.cat(outs) if len(outs) > 1 else outs[0]).cpu().numpy()
    imgs = tile_blend_numpy(members, spec.weights(members.shape[1]), n, CONFIG["scale"] * spec.stride).astype(np.float64)
    return [im[:, :, None] for im in imgs]


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def calls_for(fn, seconds):
    for _ in range(3):                                              # warm-up of every shape the leg uses
        fn()
    return max(2, int(math.ceil(seconds / window(fn, 2))))


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sets", type=int, default=8)
    p.add_argument("--stride", type=int, default=8)
    p.add_argument("--window", type=str, default="hat", choices=tiles.WINDOWS)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.2)
    p.add_argument("--kernel-calls", dest="kernel_calls", type=int, default=0)
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if not opt.kernel_calls and (opt.seconds < 1.0 or opt.windows < 3):
        raise SystemExit("at least three windows of at least a second each")
    spec = TileSpec(opt.stride, opt.window).validate(CONFIG["patch_size"], tiles.LR_SIZE)
    n = spec.n(CONFIG["patch_size"], tiles.LR_SIZE)
    S, G = CONFIG["scale"] * CONFIG["patch_size"], CONFIG["scale"] * tiles.LR_SIZE
    factor = n * n / 64.0

    dev = torch.device("cuda:0")
    model = WDSRConv3D("b", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)
    frames = synthetic_frames(opt.sets)
    patches = host_tiles(frames, CONFIG["patch_size"])               # what resolverDir holds for these frames
    plain = lambda: testClass.evaluate_device(model, patches)
    fused = lambda: testClass.evaluate_tiled_frames(model, frames, spec, CONFIG)
    composed = lambda: composed_images(model, frames, spec)
    must_move = {"tiles_per_image": n * n, "blend_bytes_per_image": (n * n * S * S + G * G) * 4, "blend_launches_per_call": 1,
                 "forward_launch_sets_per_call": -(-opt.sets * n * n // testClass.LAUNCH_BATCH)}
    if opt.kernel_calls:
        for _ in range(opt.kernel_calls):
            fused()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "tile_bench", "leg": "kernel-calls", "calls": opt.kernel_calls, "sets": opt.sets, "stride": opt.stride, **must_move}))
        return

    a, b = fused(), composed()
    equal = len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))
    if not equal:
        raise SystemExit("the fused and the composed tiled images differ at the timed size")
    differs = any(not np.array_equal(x, y) for x, y in zip(a, plain()))
    legs = (("plain", plain), ("composed", composed), ("fused", fused))
    calls = {name: calls_for(fn, opt.seconds) for name, fn in legs}
    t = {name: [] for name, _ in legs}
    for _ in range(opt.windows):                                      # A B C A B C ...: the legs see the same drift of the box
        for name, fn in legs:
            t[name].append(window(fn, calls[name]) / opt.sets)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "tile_bench", "device": torch.cuda.get_device_name(0), "sets": opt.sets, "stride": opt.stride, "window": opt.window, "n": n,
           "forward_factor": factor, "windows": opt.windows, "calls_per_window": calls, "s_per_image_windows": t, "s_per_image_median": med,
           "fused_over_factor_plain": med["fused"] / (factor * med["plain"]), "composed_over_factor_plain": med["composed"] / (factor * med["plain"]),
           "fused_over_composed": med["fused"] / med["composed"], "plain_spread": spread(t["plain"]),
           "peak_device_bytes": {name: peak(fn, dev) for name, fn in legs},
           "fused_equals_composed_bitwise": equal, "tiled_differs_from_plain": differs, "must_move": must_move, "plain_images_per_s": 1.0 / med["plain"]}
    if opt.profile:
        with open(opt.profile, "w") as fh:
            fh.write("tools/tile_bench.py on %s: one process, %d image sets, stride %d (%d x %d tiles, %.3f x the plain path's forward passes), %s window,\n"
                     "seeded model, %d alternated windows per leg, each longer than %.1f s\n\n"
                     % (res["device"], opt.sets, opt.stride, n, n, factor, opt.window, opt.windows, opt.seconds))
            for name, what in (("plain", "evaluate_device on the 64 disjoint patches"),
                               ("composed", "host tiles + resolve_device + tile_blend_numpy on the host"),
                               ("fused", "evaluate_tiled_frames (build_tiles + forward + tile_blend)")):
                fh.write("  %-8s %-60s %9.4f ms / image   windows %s   (%d calls each)\n"
                         % (name, what, med[name] * 1e3, ["%.4f" % (v * 1e3) for v in t[name]], calls[name]))
            fh.write("\n  fused / (%.3f plain) = %.4f    composed / (%.3f plain) = %.4f    fused / composed = %.4f    spread of the plain windows = %.2f %%\n"
                     % (factor, res["fused_over_factor_plain"], factor, res["composed_over_factor_plain"], res["fused_over_composed"], 100 * res["plain_spread"]))
            fh.write("  fused == composed bit for bit at this size: %s    tiled != plain image: %s\n" % (equal, differs))
            fh.write("  peak device memory of one call above what was allocated before it: plain %d B, composed %d B, fused %d B\n"
                     % tuple(res["peak_device_bytes"][k] for k in ("plain", "composed", "fused")))
            fh.write("  bytes the blend kernel must move per image (%d tiles): %d B, one launch per call; %d forward launch sets per call\n"
                     % (n * n, must_move["blend_bytes_per_image"], must_move["forward_launch_sets_per_call"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
