#!/usr/bin/env python3
"""Random crops, measured (one process, device events, one JSON line on stdout; --profile PATH also writes the figures as text):

  (a) step A/B   ModelTrainer.fitTrainData(augment=spec) on the builder's base patches of the scenes (the --online-aug step, in its own code path)
                 against fitTrainData(crops=(CropDataset, CropSpec("all"))) on the same scenes: alternated windows of --steps training steps each
                 (after --warmup), shipped shapes, batch 128.  Per window: the device time between the first and the last timed step's start
                 events over the steps between them.  Reported: the medians, their ratio, and the --online-aug leg's own window-to-window spread
                 (max - min) / median, the margin the ratio is to be read against.
  (b) kernel     device time per batch of torch.ops.probav.crop_batch at B = 128 (uniform random rows), beside a device-to-device copy of the
                 bytes it must move (the three output tensors).
  (c) torch ops  the same batch composed from existing torch ops on the device (index arithmetic over pre-padded scenes, a stable sort for the
                 frame ranking, flips and turns per code group), timed the same way and compared with the kernel's output bitwise at the timed size.
  (d) start-up   device time of the validity table and the two position lists (window_counts + nonzero) for one band's scenes (--band-scenes).
  (e) memory     device bytes resident: the scenes, masks and lists, against the base-patch set of the same scenes (augment.DeviceDataset).

    python tools/crops_bench.py [--steps 200] [--windows 3] [--profile profiles/crops_ab.txt]
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import augment, crops, prep, synth  # noqa: E402
from probav_amd.augment import AugmentSpec  # noqa: E402
from probav_amd.loss import Losses  # noqa: E402
from probav_amd.modelsTF import WDSRConv3D  # noqa: E402
from probav_amd.trainClass import ModelTrainer, make_optimizer  # noqa: E402

CFG = {"patch_size": 16, "patch_stride": 16, "max_shift": 6, "scale": 3, "num_low_res_imgs": 9, "num_low_res_imgs_pre": 9,
       "low_res_patch_thresholds": [0.85], "high_res_threshold": 0.85, "num_low_res_permute": 19, "to_flip": False, "to_rotate": False}


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def spread(v):
    return (max(v) - min(v)) / median(v)


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


class TimedTrainer(ModelTrainer):
    """Start events of the training steps (device timeline of the training stream)."""

    def trainStep(self, x, hr, mk):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.marks.append(ev)
        super().trainStep(x, hr, mk)


def step_leg(dev, scenes, steps, warmup, windows):
    batch = 128
    lr_m, hr_m = scenes
    base_lr, base_hr = prep.gridPatches(lr_m, hr_m, CFG)
    bX, by, bmk = np.array(base_lr), np.array(base_hr), ~np.ma.getmaskarray(base_hr)
    spec = AugmentSpec.from_config(CFG, seed=4)
    ds = crops.CropDataset(np.ma.getdata(lr_m)[:, :, 0], np.ma.getmaskarray(lr_m)[:, :, 0], np.ma.getdata(hr_m)[:, 0, 0], np.ma.getmaskarray(hr_m)[:, 0, 0],
                           CFG, dev)
    model = WDSRConv3D("b", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)
    losses = Losses(targetShape=(48, 48, 1))
    tmp = tempfile.mkdtemp(prefix="crops_bench_")
    tr = TimedTrainer(model, losses.shiftCompensatedL1Loss, losses.shiftCompensatedcPSNR, make_optimizer("nadam", model, 5e-4),
                      os.path.join(tmp, "c"), os.path.join(tmp, "l"), evalStep=10 ** 9)
    tr.tune_side_stream = False                                      # the engine's default mode in every window: no tuning steps inside the timing
    need = warmup + steps + 1
    epochs = -(-need * batch // (len(bX) * spec.multiplicity))
    val = [bX[:8], by[:8], bmk[:8]]
    res = {"online": [], "crops": []}

    def window(use_crops):
        tr.marks, tr.step = [], 0
        if use_crops:
            tr.fitTrainData(None, None, batch, 1, val, augment=spec, crops=(ds, crops.CropSpec("all", seed=1)), crops_per_epoch=need * batch)
        else:
            tr.fitTrainData(bX, [by, bmk], batch, epochs, val, augment=spec)
        torch.cuda.synchronize()
        return tr.marks[warmup].elapsed_time(tr.marks[warmup + steps]) / steps

    for _ in range(windows):                                          # A B A B ...: both paths see the same drift of the box
        res["online"].append(window(False))
        res["crops"].append(window(True))
    mo, mc = median(res["online"]), median(res["crops"])
    mem = {"scenes": ds.S, "crops_device_bytes": ds.nbytes + 12 * (ds.V + ds.n_grid) + ds.valid.numel(), "valid_positions": ds.V, "grid_positions": ds.n_grid,
           "base_patches": len(bX), "base_patch_set_device_bytes": augment.DeviceDataset(bX, by, bmk, dev).nbytes}
    return {"batch": batch, "steps_per_window": steps, "warmup": warmup, "windows": windows, "online_ms_per_step_windows": res["online"],
            "crops_ms_per_step_windows": res["crops"], "online_ms_per_step_median": mo, "crops_ms_per_step_median": mc, "crops_over_online": mc / mo,
            "online_spread": spread(res["online"]), "crops_spread": spread(res["crops"])}, mem, ds


def torch_crop_batch(ds, plr, pmk, rec):
    """crops.crop_batch_numpy from existing torch ops, on the device: plr / pmk the scenes reflect-padded once, rec the recipe on the device."""
    g, dev = ds.geom, ds.device
    pos = ds.positions[rec[:, 0].long()].long()
    s, y, x = pos[:, 0], pos[:, 1], pos[:, 2]
    B, T = len(rec), plr.shape[1]
    w = torch.arange(g.win, device=dev)
    si, ti = s[:, None, None, None], torch.arange(T, device=dev)[None, :, None, None]
    yi, xi = (y[:, None] + w)[:, None, :, None], (x[:, None] + w)[:, None, None, :]
    counts = pmk[si, ti, yi, xi].sum((2, 3), dtype=torch.int64)                                        # [B, T]
    elig = counts < g.L
    elig = elig | ~elig.any(1, keepdim=True)
    key = torch.where(elig, counts, torch.full_like(counts, 1 << 40))
    order = torch.sort(key, dim=1, stable=True).indices                                                # (count, index) order, the ineligible last
    E = elig.sum(1)
    m = (g.k + E - 1) // E
    Q = torch.gather(order, 1, torch.arange(g.k, device=dev)[None, :] // m[:, None])                   # [B, k]
    frames = torch.gather(Q, 1, rec[:, 3:].long())                                                     # Q[perm[i]]
    lr_b = plr[s[:, None, None, None], frames[:, None, None, :], (y[:, None] + w)[:, :, None, None], (x[:, None] + w)[:, None, :, None]].unsqueeze(-1)
    h = torch.arange(g.side, device=dev)
    hy, hx = (g.r * y[:, None] + h)[:, :, None], (g.r * x[:, None] + h)[:, None, :]
    hr_b, mk_b = ds.hr[s[:, None, None], hy, hx].unsqueeze(-1), ds.hr_clear[s[:, None, None], hy, hx].unsqueeze(-1)
    outs = [torch.empty_like(t) for t in (lr_b, hr_b, mk_b)]
    code = rec[:, 1] * 4 + rec[:, 2]
    for c in range(16):
        rows = torch.nonzero(code == c)[:, 0]
        if len(rows):
            dims = [(), (1,), (2,), (1, 2)][c // 4]
            for o, t in zip(outs, (lr_b, hr_b, mk_b)):
                o[rows] = torch.rot90(torch.flip(t[rows], dims) if dims else t[rows], c % 4, (1, 2))
    return outs[0], outs[1], outs[2], Q.to(torch.int32)


def kernel_leg(ds, launches):
    g, dev, B = ds.geom, ds.device, 128
    spec = AugmentSpec(19, True, True)
    rec_h = next(crops.random_recipes(ds.V, g.k, spec, crops.CropSpec("all", seed=2), 0, B, 1))
    crops.validate_recipe(rec_h, ds.V, g.k)
    rec = torch.from_numpy(rec_h).to(dev)
    run = lambda: torch.ops.probav.crop_batch(ds.lr, ds.lr_mask, ds.hr, ds.hr_clear, ds.positions, rec, g.P, g.pad, g.win, g.r, g.L)
    nbytes = B * (g.win ** 2 * g.k * 4 + g.side ** 2 * 5)
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pw = (g.pad,) * 4
    plr = torch.nn.functional.pad(ds.lr, pw, mode="reflect")
    pmk = torch.nn.functional.pad(ds.lr_mask.float(), pw, mode="reflect").to(torch.uint8)
    composed = lambda: torch_crop_batch(ds, plr, pmk, rec)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(run(), composed()))
    t_k, t_c, t_t = time_launches(run, launches), time_launches(lambda: dst.copy_(src), launches), time_launches(composed, launches)
    return {"batch": B, "output_bytes": nbytes, "crop_batch_us": t_k, "copy_us": t_c, "crop_batch_over_copy": t_k / t_c, "torch_ops_us": t_t,
            "torch_ops_over_crop_batch": t_t / t_k, "torch_ops_equal_bitwise": bool(same)}


def startup_leg(dev, n_scenes, launches):
    g = crops.CropGeometry(CFG)
    rng = np.random.default_rng(7)
    masks = torch.from_numpy((rng.random((n_scenes, 384, 384)) < 0.04).view(np.uint8)).to(dev)

    def build():
        valid = torch.ops.probav.window_counts(masks, 0, g.side, g.r) < g.L_hr
        return torch.nonzero(valid).to(torch.int32), torch.nonzero(valid[:, ::g.stride, ::g.stride]).to(torch.int32)
    us = time_launches(build, launches)
    counts = time_launches(lambda: torch.ops.probav.window_counts(masks, 0, g.side, g.r), launches)
    return {"scenes": n_scenes, "table_and_lists_us": us, "window_counts_us": counts, "valid_positions": int(build()[0].shape[0])}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--scenes", type=int, default=8, help="scenes of the step A/B (64 grid patches each)")
    p.add_argument("--band-scenes", dest="band_scenes", type=int, default=566, help="scenes of one band, for the start-up leg")
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if opt.steps < 200 or opt.launches < 200 or opt.windows < 3:
        raise SystemExit("at least three windows of at least 200 steps / 200 launches")
    import logging
    logging.getLogger("probav_amd").setLevel(logging.WARNING)
    dev = torch.device("cuda:0")
    step, mem, ds = step_leg(dev, synth.synth_scenes(opt.scenes, seed=3), opt.steps, opt.warmup, opt.windows)
    res = {"tool": "crops_bench", "device": torch.cuda.get_device_name(0), "step_ab": step, "kernel": kernel_leg(ds, opt.launches),
           "startup": startup_leg(dev, opt.band_scenes, opt.launches), "memory": mem}
    if opt.profile:
        s, k, u, m = res["step_ab"], res["kernel"], res["startup"], res["memory"]
        with open(opt.profile, "w") as fh:
            fh.write("tools/crops_bench.py on %s: one process, device events, alternated windows\n\n" % res["device"])
            fh.write("(a) step A/B (batch %d, shipped shapes, %d windows of %d steps each way, medians of the windows)\n" % (s["batch"], s["windows"], s["steps_per_window"]))
            fh.write("  fitTrainData(augment=spec), base patches     %.4f ms / step   windows %s   spread (max - min) / median %.4f\n"
                     % (s["online_ms_per_step_median"], ["%.4f" % v for v in s["online_ms_per_step_windows"]], s["online_spread"]))
            fh.write("  fitTrainData(crops=(dataset, 'all'))         %.4f ms / step   windows %s   spread %.4f\n"
                     % (s["crops_ms_per_step_median"], ["%.4f" % v for v in s["crops_ms_per_step_windows"]], s["crops_spread"]))
            fh.write("  crops / online                               %.4f   (margin: the online leg's own spread, %.4f)\n\n" % (s["crops_over_online"], s["online_spread"]))
            fh.write("(b) crop_batch alone, B = %d (device time per launch, %d launches after 20)\n" % (k["batch"], opt.launches))
            fh.write("  crop_batch %8.2f us   device copy of its %d output bytes %8.2f us   ratio %.2f\n\n" % (k["crop_batch_us"], k["output_bytes"], k["copy_us"], k["crop_batch_over_copy"]))
            fh.write("(c) the same batch from existing torch ops on the device\n")
            fh.write("  %8.2f us   %.1f x crop_batch   output equal bitwise: %s\n\n" % (k["torch_ops_us"], k["torch_ops_over_crop_batch"], k["torch_ops_equal_bitwise"]))
            fh.write("(d) start-up: validity table and position lists of %d scenes (HR masks 384 x 384)\n" % u["scenes"])
            fh.write("  window_counts %8.2f us   table + both lists %8.2f us   %d valid positions\n\n" % (u["window_counts_us"], u["table_and_lists_us"], u["valid_positions"]))
            fh.write("(e) device bytes resident, %d scenes\n" % m["scenes"])
            fh.write("  scenes, masks, table and lists %d B (%d valid positions, %d on the grid)   base-patch set of the same scenes %d B (%d patches)\n"
                     % (m["crops_device_bytes"], m["valid_positions"], m["grid_positions"], m["base_patch_set_device_bytes"], m["base_patches"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
