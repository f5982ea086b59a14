#!/usr/bin/env python3
"""Optimizer options on the device, measured (one process, one box, one JSON line on stdout; --profile PATH also writes the figures as text):

  bitwise    3 training steps with make_optimizer(...) against 3 with global_clipnorm far above the norm + skip_nonfinite (scale == 1, nothing
             skipped, no EMA): the parameters must be the plain step's, bit for bit.
  step A/B   the full training step (forward + loss + backward + optimizer, ModelTrainer.trainStep, batch 128, shipped shapes) with the plain
             optimizer (the yardstick) against clip + guard + EMA: interleaved windows of --steps steps each (after --warmup), device time
             between the first and the last step's start events; medians over the windows, their ratio, and the spread of the plain windows
             among themselves (what the ratio has to exceed to mean anything).

    python tools/optim_guard_bench.py [--steps 100] [--windows 3] [--profile profiles/optim_guard_ab.txt]

Under `rocprofv3 --kernel-trace --stats -- python tools/optim_guard_bench.py` the launches the options add are grad_sumsq_kernel,
guard_finish_kernel and wn_forward_guard_kernel (in place of wn_forward_kernel<true>).
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import synth  # noqa: E402
from probav_amd.loss import Losses  # noqa: E402
from probav_amd.modelsTF import WDSRConv3D  # noqa: E402
from probav_amd.trainClass import ModelTrainer, make_optimizer  # noqa: E402


def trainer(dev, tmp, tag, **opts):
    model = WDSRConv3D("b", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
    model.load_variables(synth.synth_params(seed=7, perturb=True))
    model = model.to(dev)
    losses = Losses(targetShape=(48, 48, 1))
    tr = ModelTrainer(model, losses.shiftCompensatedL1Loss, losses.shiftCompensatedcPSNR, make_optimizer("nadam", model, 5e-4, **opts),
                      os.path.join(tmp, tag, "c"), os.path.join(tmp, tag, "l"))
    return tr, model


def window(tr, batch, steps):
    """ms per step: device time from the start of the first timed step to the start of the step after the last."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        tr.trainStep(*batch)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if opt.windows < 3:
        raise SystemExit("at least three windows per leg")
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="optim_guard_bench_")
    x, hr, mask = synth.synth_batch(16, seed=3)
    rep = lambda a: torch.from_numpy(np.concatenate([a] * (opt.batch // len(a) + 1))[:opt.batch]).to(dev)
    batch = (rep(x), rep(hr), rep(mask))

    # bitwise: the guarded launches at scale == 1, no skip, no EMA leave the plain step's parameters
    (ta, ma), (tb, mb) = trainer(dev, tmp, "bit_plain"), trainer(dev, tmp, "bit_guard", global_clipnorm=1e30, skip_nonfinite=True)
    small = tuple(t[:8] for t in batch)
    for _ in range(3):
        ta.trainStep(*small)
        tb.trainStep(*small)
    torch.cuda.synchronize()
    stats = {k: float(v) for k, v in tb.optimizer.guard_stats().items()}
    bitwise = bool(torch.equal(ma.flat.detach().view(torch.int32), mb.flat.detach().view(torch.int32))) and stats["scale"] == 1.0 and stats["skipped_total"] == 0
    del ta, ma, tb, mb

    legs = {"plain": trainer(dev, tmp, "plain")[0],
            "guarded": trainer(dev, tmp, "guarded", global_clipnorm=1.0, skip_nonfinite=True, use_ema=True, ema_momentum=0.99)[0]}
    for tr in legs.values():
        tr.tune_side_stream = False
        for _ in range(opt.warmup):
            tr.trainStep(*batch)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(opt.windows):                                     # A B A B ...: both legs see the same drift of the box
        for k, tr in legs.items():
            ms[k].append(window(tr, batch, opt.steps))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = (max(ms["plain"]) - min(ms["plain"])) / med["plain"]
    g = {k: float(v) for k, v in legs["guarded"].optimizer.guard_stats().items()}
    res = {"tool": "optim_guard_bench", "device": torch.cuda.get_device_name(0), "batch": opt.batch, "steps_per_window": opt.steps, "windows": opt.windows,
           "bitwise_scale1_no_skip_no_ema_equals_plain": bitwise, "plain_ms_per_step_windows": ms["plain"], "guarded_ms_per_step_windows": ms["guarded"],
           "plain_ms_per_step_median": med["plain"], "guarded_ms_per_step_median": med["guarded"], "guarded_over_plain": med["guarded"] / med["plain"],
           "plain_windows_spread_over_median": spread, "guarded_exceeds_plain_spread": (med["guarded"] - med["plain"]) > (max(ms["plain"]) - min(ms["plain"])),
           "guarded_leg_last_step": g}
    if opt.profile:
        with open(opt.profile, "w") as fh:
            fh.write("tools/optim_guard_bench.py on %s: one process, same box, interleaved windows\n\n" % res["device"])
            fh.write("bitwise: guarded step with scale == 1, no skip, no EMA == plain step over 3 steps: %s\n\n" % bitwise)
            fh.write("full training step, batch %d, T = 9, H = 22, %d windows of %d steps per leg, medians of the windows\n" % (opt.batch, opt.windows, opt.steps))
            fh.write("  plain optimizer (yardstick)      %.4f ms / step   windows %s\n" % (med["plain"], ["%.4f" % v for v in ms["plain"]]))
            fh.write("  clip + guard + EMA               %.4f ms / step   windows %s\n" % (med["guarded"], ["%.4f" % v for v in ms["guarded"]]))
            fh.write("  guarded / plain                  %.4f\n" % res["guarded_over_plain"])
            fh.write("  spread of the plain windows      %.4f of their median  (guarded - plain exceeds it: %s)\n" % (spread, res["guarded_exceeds_plain_spread"]))
            fh.write("  guarded leg, last step: norm %.6g, scale %.6g, skipped %d\n" % (g["norm"], g["scale"], int(g["skipped_total"])))
    print(json.dumps(res))
    if not bitwise:
        raise SystemExit("the guarded step with scale == 1, no skip and no EMA does NOT leave the plain step's parameters")


if __name__ == "__main__":
    main()
