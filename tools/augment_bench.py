#!/usr/bin/env python3
"""Online augmentation, measured (one process, one JSON line on stdout; --profile PATH also writes the figures as text):

  step A/B   ModelTrainer.fitTrainData on materialised host arrays (the yardstick) against fitTrainData(augment=spec): interleaved windows of
             --steps training steps each (after --warmup steps), shipped shapes (T = 9, H = 22, batch 128, num_low_res_permute = 19); the
             per-window figure is the device time between the first and the last timed step's start events divided by the steps between
             them; medians over the windows, and their ratio.
  kernel     device time per batch of torch.ops.probav.augment_batch at B = 128 and B = 2048, identity recipes and a mix of all 16 codes with
             random frame orders, each beside a device-to-device copy of the same byte count (events around --launches launches after 20).
  memory     host RSS growth from loading the un-augmented set and from materialising it 20 x and 320 x; device bytes the online path holds.

    python tools/augment_bench.py [--steps 200] [--windows 3] [--profile profiles/augment_step_ab.txt]
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import augment, prep, synth  # noqa: E402
from probav_amd.augment import AugmentSpec  # noqa: E402
from probav_amd.loss import Losses  # noqa: E402
from probav_amd.modelsTF import WDSRConv3D  # noqa: E402
from probav_amd.trainClass import ModelTrainer, make_optimizer  # noqa: E402


def rss():
    with open("/proc/self/statm") as fh:
        return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def materialise(lr, hr, mask, numPermute, flip, rotate, rng):
    a = prep.augmentByShufflingLRImgs(lr, numPermute=numPermute, rng=rng)
    h, m = np.tile(hr, (numPermute + 1, 1, 1, 1)), np.tile(mask, (numPermute + 1, 1, 1, 1))
    if flip:
        a, h, m = (prep.augmentByFlipping(x) for x in (a, h, m))
    if rotate:
        a, h, m = (prep.augmentByRotating(x) for x in (a, h, m))
    return tuple(np.ascontiguousarray(np.ma.getdata(x)) for x in (a, h, m))


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def time_launches(fn, launches):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches                       # microseconds per launch


def kernel_leg(dev, launches):
    rng = np.random.default_rng(0)
    N, T = 4096, 9
    x, hr, mask = synth.synth_batch(256, seed=1)
    rep = lambda a: torch.from_numpy(np.concatenate([a] * (N // len(a)))).to(dev)
    dl, dh, dm = rep(x), rep(hr), rep(mask)
    out = {}
    for B in (128, 2048):
        ident = np.zeros((B, 3 + T), np.int32)
        ident[:, 0], ident[:, 3:] = rng.permutation(N)[:B], np.arange(T)
        mixed = ident.copy()
        mixed[:, 1], mixed[:, 2] = np.arange(B) % 4, (np.arange(B) // 4) % 4
        mixed[:, 3:] = rng.permuted(np.broadcast_to(np.arange(T), (B, T)), axis=1)
        nbytes = B * (x[0].nbytes + hr[0].nbytes + mask[0].nbytes)
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        t_copy = time_launches(lambda: dst.copy_(src), launches)
        res = {"bytes_read_plus_written": 2 * nbytes, "copy_us": t_copy}
        for name, rec in (("identity", ident), ("mixed", mixed)):
            augment.validate_recipe(rec, N, T)
            r = torch.from_numpy(rec).to(dev)
            res[name + "_us"] = time_launches(lambda: torch.ops.probav.augment_batch(dl, dh, dm, r), launches)
            res[name + "_over_copy"] = res[name + "_us"] / t_copy
        res["mixed_over_identity"] = res["mixed_us"] / res["identity_us"]
        out["B%d" % B] = res
    return out


class TimedTrainer(ModelTrainer):
    """Start events of the training steps (device timeline of the training stream)."""

    def trainStep(self, x, hr, mk):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append(ev)
        super().trainStep(x, hr, mk)


def step_leg(dev, steps, warmup, windows, base_n):
    numPermute, batch = 19, 128
    x, hr, mask = synth.synth_batch(base_n, seed=3)
    spec = AugmentSpec(numPermute, False, False, seed=4)
    rss0 = rss()
    X, y, mk = materialise(x, hr, mask, numPermute, False, False, np.random.RandomState(4))
    rss_mat = rss() - rss0
    model = WDSRConv3D("b", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)
    losses = Losses(targetShape=(48, 48, 1))
    tmp = tempfile.mkdtemp(prefix="augment_bench_")
    tr = TimedTrainer(model, losses.shiftCompensatedL1Loss, losses.shiftCompensatedcPSNR, make_optimizer("nadam", model, 5e-4),
                      os.path.join(tmp, "c"), os.path.join(tmp, "l"), evalStep=10 ** 9)
    tr.tune_side_stream = False                                      # the engine's default mode in every window: no tuning steps inside the timing
    epochs = -(-(warmup + steps + 1) * batch // len(X))                # whole epochs that hold warm-up + timed steps
    val = [x[:8], hr[:8], mask[:8]]
    res = {"host": [], "online": []}

    def window(online):
        tr.marks, tr.step = [], 0
        if online:
            tr.fitTrainData(x, [hr, mask], batch, epochs, val, augment=spec)
        else:
            tr.fitTrainData(X, [y, mk], batch, epochs, val)
        torch.cuda.synchronize()
        return tr.marks[warmup].elapsed_time(tr.marks[warmup + steps]) / steps

    for _ in range(windows):                                          # A B A B ...: both paths see the same drift of the box
        res["host"].append(window(False))
        res["online"].append(window(True))
    mh, mo = median(res["host"]), median(res["online"])
    return {"batch": batch, "steps_per_window": steps, "warmup": warmup, "windows": windows, "base_samples": base_n, "multiplicity": spec.multiplicity,
            "host_ms_per_step_windows": res["host"], "online_ms_per_step_windows": res["online"],
            "host_ms_per_step_median": mh, "online_ms_per_step_median": mo, "online_over_host": mo / mh,
            "host_rss_materialised_20x_bytes": rss_mat}


def memory_leg(dev, base_n):
    x, hr, mask = synth.synth_batch(base_n, seed=5)
    per = x[0].nbytes + hr[0].nbytes + mask[0].nbytes
    out = {"base_samples": base_n, "bytes_per_sample": per, "base_bytes": base_n * per}
    for mult, (p, f, r) in ((20, (19, False, False)), (320, (19, True, True))):
        r0 = rss()
        arrays = materialise(x, hr, mask, p, f, r, np.random.RandomState(0))
        out["host_rss_growth_%dx_bytes" % mult] = rss() - r0
        out["materialised_%dx_bytes" % mult] = sum(a.nbytes for a in arrays)
        del arrays
    torch.cuda.synchronize()
    d0 = torch.cuda.memory_allocated(dev)
    ds = augment.DeviceDataset(x, hr, mask, dev)
    out["online_device_bytes"] = torch.cuda.memory_allocated(dev) - d0
    out["online_device_bytes_reported"] = ds.nbytes
    out["online_host_bytes"] = base_n * per                         # the un-augmented arrays the CLI loaded (they may be dropped after the upload)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--base", type=int, default=512, help="un-augmented samples of the step A/B")
    p.add_argument("--mem-base", dest="mem_base", type=int, default=128, help="un-augmented samples of the memory leg (materialised 320 x on the host)")
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if opt.steps < 200 or opt.launches < 200:
        raise SystemExit("windows of at least 200 steps / 200 launches")
    import logging
    logging.getLogger("probav_amd").setLevel(logging.WARNING)       # (the trainer's per-step lines: 1 400 of them)
    dev = torch.device("cuda:0")
    res = {"tool": "augment_bench", "device": torch.cuda.get_device_name(0),
           "kernel": kernel_leg(dev, opt.launches), "step_ab": step_leg(dev, opt.steps, opt.warmup, opt.windows, opt.base),
           "memory": memory_leg(dev, opt.mem_base)}
    if opt.profile:
        s, k, m = res["step_ab"], res["kernel"], res["memory"]
        with open(opt.profile, "w") as fh:
            fh.write("tools/augment_bench.py on %s: one process, same box, interleaved windows\n\n" % res["device"])
            fh.write("step A/B (batch %d, T = 9, H = 22, %d windows of %d steps each way, medians of the windows)\n" % (s["batch"], s["windows"], s["steps_per_window"]))
            fh.write("  fitTrainData on materialised host arrays   %.4f ms / step   windows %s\n" % (s["host_ms_per_step_median"], ["%.4f" % v for v in s["host_ms_per_step_windows"]]))
            fh.write("  fitTrainData(augment=spec)                 %.4f ms / step   windows %s\n" % (s["online_ms_per_step_median"], ["%.4f" % v for v in s["online_ms_per_step_windows"]]))
            fh.write("  online / host                              %.4f\n\n" % s["online_over_host"])
            fh.write("kernel (device time per batch, %d launches after 20)\n" % opt.launches)
            for B, r in k.items():
                fh.write("  %-5s %9d B moved   copy %8.2f us   identity %8.2f us (%.2f x copy)   mixed %8.2f us (%.2f x copy)   mixed / identity %.3f\n"
                         % (B, r["bytes_read_plus_written"], r["copy_us"], r["identity_us"], r["identity_over_copy"], r["mixed_us"], r["mixed_over_copy"],
                            r["mixed_over_identity"]))
            fh.write("\nmemory (%d un-augmented samples, %d B each = %d B)\n" % (m["base_samples"], m["bytes_per_sample"], m["base_bytes"]))
            for mult in (20, 320):
                fh.write("  materialised %3d x: %12d B of arrays, host RSS grew by %12d B\n" % (mult, m["materialised_%dx_bytes" % mult], m["host_rss_growth_%dx_bytes" % mult]))
            fh.write("  online: %d B on the device (any multiplicity), %d B of host arrays to upload from\n" % (m["online_device_bytes"], m["online_host_bytes"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
