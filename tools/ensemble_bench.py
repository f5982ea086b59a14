#!/usr/bin/env python3
"""Test-time self-ensemble, measured (one process, one JSON line on stdout; --profile PATH also writes the figures as text).

--sets image sets of 64 patches (default 16), a seeded model, every shape warmed up, then --windows rounds of three legs ALTERNATED in the
same process, each window a whole number of calls sized to last longer than --seconds and closed by a device synchronise:

  plain   testClass.evaluate_device(model, patches)                                   -> t_plain per image
  torch   the "d8" ensemble composed here from parts that exist without the feature: torch.flip / rot90 / cat around resolve_device, the
          inverse turns, stack, mean, round, stitch_device (launch sets of LAUNCH_BATCH // 8 patches, like the fused path)
  fused   testClass.evaluate_device(model, patches, ensemble=EnsembleSpec("d8"))      (ensemble_expand -> forward -> ensemble_reduce + stitch)

The images of the torch and the fused leg are compared at the timed size and must be equal bit for bit (the tool fails otherwise).
Reported: t_fused / (8 t_plain), t_torch / (8 t_plain), the window-to-window spread of the plain leg, peak device memory of one torch and one
fused call, and the plain leg of a fresh child process that runs nothing else (--plain-only; no ensemble op is called there) beside this
process's.  --kernel-calls N instead runs N fused calls and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`; the bytes
the two kernels must move per launch are printed beside it.

    python tools/ensemble_bench.py [--sets 16] [--windows 3] [--seconds 1.2] [--profile profiles/ensemble_ab.txt]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import synth, testClass  # noqa: E402
from probav_amd.augment import FLIP_AXES  # noqa: E402
from probav_amd.modelsTF import WDSRConv3D  # noqa: E402


def torch_ensemble(model, patches, table):
    """evaluate_device(..., ensemble=spec, final="round") from existing parts only."""
    dev = next(model.parameters()).device
    p = torch.as_tensor(patches)
    sets = p.shape[0]
    flat = p.reshape((-1,) + tuple(p.shape[2:]))
    V = len(table)
    per = max(1, testClass.LAUNCH_BATCH // V)
    ident = np.arange(flat.shape[3])
    outs = []
    for i in range(0, flat.shape[0], per):
        x = flat[i:i + per].to(dev)
        variants, undo = [], []
        for row in table:
            f, k, perm = int(row[0]), int(row[1]), row[2:]
            dims = [a + 1 for a in FLIP_AXES[f]]
            xv = x if np.array_equal(perm, ident) else x.index_select(3, torch.as_tensor(perm.astype(np.int64)).to(dev))
            variants.append(torch.rot90(torch.flip(xv, dims) if dims else xv, k, dims=(1, 2)))
            undo.append((dims, k))
        sr = testClass.resolve_device(model, torch.cat(variants))                   # clipped and rounded members, variant-major
        members = sr.reshape((V, x.shape[0]) + tuple(sr.shape[1:]))
        back = [torch.flip(torch.rot90(members[v], -k, dims=(1, 2)), dims) if dims else torch.rot90(members[v], -k, dims=(1, 2))
                for v, (dims, k) in enumerate(undo)]
        outs.append(torch.round(torch.stack(back).mean(0)))
    imgs = testClass.stitch_device(torch.cat(outs) if len(outs) > 1 else outs[0], sets).cpu().numpy().astype(np.float64)
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
    p.add_argument("--sets", type=int, default=16)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--seconds", type=float, default=1.2)
    p.add_argument("--plain-only", dest="plain_only", action="store_true")
    p.add_argument("--kernel-calls", dest="kernel_calls", type=int, default=0)
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if opt.seconds < 1.0 or opt.windows < 3:
        raise SystemExit("at least three windows of at least a second each")
    child = None
    if not opt.plain_only and not opt.kernel_calls:                 # before this process opens the device: the plain leg alone, in a fresh process
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--sets", str(opt.sets), "--windows", str(opt.windows),
                              "--seconds", str(opt.seconds)], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit("the --plain-only child failed:\n" + out.stderr[-2000:])
        child = json.loads(out.stdout.strip().splitlines()[-1])

    dev = torch.device("cuda:0")
    model = WDSRConv3D("b", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)
    patches = synth.synth_batch(opt.sets * 64, seed=21)[0].reshape(opt.sets, 64, 22, 22, 9, 1)
    plain = lambda: testClass.evaluate_device(model, patches)
    if opt.plain_only:
        n = calls_for(plain, opt.seconds)
        t = [window(plain, n) / opt.sets for _ in range(opt.windows)]
        print(json.dumps({"tool": "ensemble_bench", "leg": "plain-only", "calls_per_window": n, "s_per_image_windows": t,
                          "images_per_s_median": 1.0 / float(np.median(t))}))
        return

    from probav_amd.ensemble import EnsembleSpec
    spec = EnsembleSpec("d8")
    table = spec.table(9)
    V, N = spec.V, opt.sets * 64
    per = min(N, max(1, testClass.LAUNCH_BATCH // V))
    fused = lambda: testClass.evaluate_device(model, patches, ensemble=spec, final="round")
    composed = lambda: torch_ensemble(model, patches, table)
    must_move = {"patches_per_launch": per, "expand_bytes_per_launch": per * 22 * 22 * 9 * 4 * (1 + V), "reduce_bytes_per_launch": per * 48 * 48 * 4 * (V + 1),
                 "launches_per_call": -(-N // per)}
    if opt.kernel_calls:
        for _ in range(opt.kernel_calls):
            fused()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "ensemble_bench", "leg": "kernel-calls", "calls": opt.kernel_calls, "sets": opt.sets, **must_move}))
        return

    a, b = fused(), composed()
    equal = len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    if not equal:
        raise SystemExit("the fused and the composed ensemble differ at the timed size")
    differs = any(not np.array_equal(x, y) for x, y in zip(a, plain()))
    calls = {"plain": calls_for(plain, opt.seconds), "torch": calls_for(composed, opt.seconds), "fused": calls_for(fused, opt.seconds)}
    t = {"plain": [], "torch": [], "fused": []}
    for _ in range(opt.windows):                                      # A B C A B C ...: the legs see the same drift of the box
        for name, fn in (("plain", plain), ("torch", composed), ("fused", fused)):
            t[name].append(window(fn, calls[name]) / opt.sets)
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "ensemble_bench", "device": torch.cuda.get_device_name(0), "sets": opt.sets, "patches": N, "V": V, "windows": opt.windows,
           "calls_per_window": calls, "s_per_image_windows": t, "s_per_image_median": med,
           "fused_over_8_plain": med["fused"] / (V * med["plain"]), "torch_over_8_plain": med["torch"] / (V * med["plain"]),
           "fused_over_torch": med["fused"] / med["torch"], "plain_spread": spread(t["plain"]),
           "fused_within_plain_spread_of_torch": med["fused"] <= med["torch"] * (1.0 + spread(t["plain"])),
           "peak_device_bytes": {"plain": peak(plain, dev), "torch": peak(composed, dev), "fused": peak(fused, dev)},
           "fused_equals_torch_bitwise": equal, "ensemble_differs_from_plain": differs, "must_move": must_move,
           "plain_only_child": child, "plain_images_per_s": 1.0 / med["plain"],
           "plain_vs_child": (1.0 / med["plain"]) / child["images_per_s_median"]}
    if opt.profile:
        with open(opt.profile, "w") as fh:
            fh.write("tools/ensemble_bench.py on %s: one process, %d image sets of 64 patches, seeded model, %d alternated windows per leg, each longer than %.1f s\n\n"
                     % (res["device"], opt.sets, opt.windows, opt.seconds))
            for name, what in (("plain", "evaluate_device"), ("torch", "d8 composed from torch.flip / rot90 / cat + resolve_device + mean"),
                               ("fused", "evaluate_device(ensemble=EnsembleSpec('d8'))")):
                fh.write("  %-5s %-68s %9.4f ms / image   windows %s   (%d calls each)\n"
                         % (name, what, med[name] * 1e3, ["%.4f" % (v * 1e3) for v in t[name]], calls[name]))
            fh.write("\n  fused / (8 plain) = %.4f    torch / (8 plain) = %.4f    fused / torch = %.4f    spread of the plain windows = %.2f %%\n"
                     % (res["fused_over_8_plain"], res["torch_over_8_plain"], res["fused_over_torch"], 100 * res["plain_spread"]))
            fh.write("  fused <= torch within the plain spread: %s    fused == torch bit for bit at this size: %s    ensemble != plain image: %s\n"
                     % (res["fused_within_plain_spread_of_torch"], equal, differs))
            fh.write("  peak device memory of one call above what was allocated before it: plain %d B, torch %d B, fused %d B\n"
                     % tuple(res["peak_device_bytes"][k] for k in ("plain", "torch", "fused")))
            fh.write("  plain leg here %.2f images / s; in a fresh process that runs only the plain leg (no ensemble op called) %.2f images / s (ratio %.4f)\n"
                     % (res["plain_images_per_s"], child["images_per_s_median"], res["plain_vs_child"]))
            fh.write("  bytes the kernels must move per launch (%d patches, %d launches per call): expand %d B, reduce %d B\n"
                     % (per, must_move["launches_per_call"], must_move["expand_bytes_per_launch"], must_move["reduce_bytes_per_launch"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
