#!/usr/bin/env python3
"""Input gradients, measured (one MI355X, one process, device events, alternated windows; one JSON line on stdout, --profile PATH also writes text):

  (1) step     forward + shift-L1 loss + backward at B = 128, T = 9 (shipped shapes), with and without `x.requires_grad`: --windows windows of --steps
               steps each way, alternated A B A B ...; per window the device time between the first and the last step's start events.  Reported: the
               medians, their difference (what d loss / d x costs a step) and the plain leg's own window-to-window spread, the margin to read it against.
  (2) kernel   probav_input_grad alone at that size, beside a device-to-device copy that moves the same number of bytes (the kernel reads g and act0 and
               writes dx; the copy reads and writes half that sum each).
  (3) composed the same dx from existing parts: probav_conv3d_forward on the backward-data geometry of mainConv1 with act0 as gate, the un-fused
               residual backward-data (probav_conv3d_forward on residConv1's backward-data geometry, r1 as gate), torch for the spread over the frames
               and 1 / std -- timed the same way and compared with the fused dx at the timed size.

    python tools/input_grad_bench.py [--steps 50] [--windows 3] [--launches 200] [--profile profiles/input_grad_ab.txt]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import _lib, synth  # noqa: E402
from probav_amd.loss import Losses  # noqa: E402
from probav_amd.modelsTF import WDSRConv3D  # noqa: E402

B, T, H, C, F = 128, 9, 22, 1, 32


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def spread(v):
    return (max(v) - min(v)) / median(v)


def timed(fn, n, warm):
    """device microseconds per call: n calls between two events, after `warm` calls"""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def alternate(legs, n, warm, windows):
    """{name: [us per call, one per window]}: the legs take turns, window by window"""
    res = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            res[k].append(timed(fn, n, warm))
    return res


def step_leg(dev, steps, warmup, windows):
    model = WDSRConv3D("b", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, T, 16, True, seed=0)
    model.load_variables(synth.synth_params(seed=7, perturb=True))
    model = model.to(dev)
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=8))
    loss_fn = Losses(targetShape=(48, 48, 1)).shiftCompensatedL1Loss
    xg = x.clone().requires_grad_(True)

    def step(inp):
        model.flat.grad = None
        inp.grad = None
        loss_fn(hr, mask, model(inp, training=True)).backward()
    res = alternate({"plain": lambda: step(x), "with_dx": lambda: step(xg)}, steps, warmup, windows)
    mp, mx = median(res["plain"]), median(res["with_dx"])
    return {"batch": B, "frames": T, "steps_per_window": steps, "windows": windows, "plain_us_windows": res["plain"], "with_dx_us_windows": res["with_dx"],
            "plain_us_median": mp, "with_dx_us_median": mx, "dx_cost_us": mx - mp, "with_dx_over_plain": mx / mp, "plain_spread": spread(res["plain"]),
            "with_dx_spread": spread(res["with_dx"])}


def conv(geom, x, gate, w, y):
    g = (ctypes.c_int32 * 17)(*geom)
    _lib.check(_lib.lib().probav_conv3d_forward(ctypes.byref(g), _lib.ptr(x), _lib.ptr(gate), _lib.ptr(w), None, None, _lib.ptr(y), 0, _lib.current_stream()),
               "probav_conv3d_forward")


def kernel_legs(dev, launches, windows):
    gen = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    g, act0 = rnd(B, H, H, T, F), torch.relu(rnd(B, H, H, T, F))
    wmain, w1 = 0.2 * rnd(3, 3, 3, C, F), 0.3 * rnd(3, 3, 1, C, 9)
    d1, r1 = rnd(B, H - 2, H - 2, 9), torch.relu(rnd(B, H - 2, H - 2, 9))
    std = float(synth.NIR_STD)
    dx = torch.empty(B, H, H, T, C, device=dev)
    L = _lib.lib()

    def fused():
        _lib.check(L.probav_input_grad(B, H, T, C, _lib.ptr(g), _lib.ptr(act0), _lib.ptr(wmain), _lib.ptr(d1), _lib.ptr(r1), _lib.ptr(w1), std, _lib.ptr(dx),
                                       _lib.current_stream()), "probav_input_grad")
    moved = (g.numel() + act0.numel() + dx.numel()) * 4
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    # the existing parts: backward-data = a correlation with the flipped, channel-swapped filter and pads k - 1 - p
    wmT = wmain.flip(0, 1, 2).permute(0, 1, 2, 4, 3).contiguous()
    w1T = w1.flip(0, 1).permute(0, 1, 2, 4, 3).contiguous()
    main, res = torch.empty(B, H, H, T, C, device=dev), torch.empty(B, H, H, 1, C, device=dev)
    gm = (B, H, H, T, F, H, H, T, C, 3, 3, 3, 1, 1, 1, 0, 0)
    gr = (B, H - 2, H - 2, 1, 9, H, H, 1, C, 3, 3, 1, 2, 2, 0, 0, 0)

    def composed():
        conv(gm, g, act0, wmT, main)
        conv(gr, d1, r1, w1T, res)
        return (main + res / T) / std
    fused()
    ref = composed()
    err = float((dx - ref).abs().max() / ref.abs().max())
    t = alternate({"fused": fused, "copy": lambda: dst.copy_(src), "composed": composed}, launches, 20, windows)
    mf, mc, mo = median(t["fused"]), median(t["copy"]), median(t["composed"])
    return {"batch": B, "frames": T, "bytes_moved": moved, "fused_us_windows": t["fused"], "copy_us_windows": t["copy"], "composed_us_windows": t["composed"],
            "fused_us": mf, "copy_us": mc, "fused_over_copy": mf / mc, "fused_tb_per_s": moved / mf * 1e-6, "composed_us": mo, "composed_over_fused": mo / mf,
            "fused_vs_composed_max_err_over_max": err}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if opt.windows < 3 or opt.steps < 20 or opt.launches < 100:
        raise SystemExit("at least three windows of at least 20 steps / 100 launches")
    dev = torch.device("cuda:0")
    res = {"tool": "input_grad_bench", "device": torch.cuda.get_device_name(0), "step": step_leg(dev, opt.steps, opt.warmup, opt.windows),
           "kernel": kernel_legs(dev, opt.launches, opt.windows)}
    if opt.profile:
        s, k = res["step"], res["kernel"]
        f3 = lambda v: ["%.1f" % q for q in v]
        with open(opt.profile, "w") as fh:
            fh.write("tools/input_grad_bench.py on %s: one process, device events, alternated windows\n\n" % res["device"])
            fh.write("(1) forward + shift-L1 loss + backward, B = %d, T = %d (%d windows of %d steps each way, medians of the windows)\n" % (B, T, s["windows"], s["steps_per_window"]))
            fh.write("  x does not require grad (wdsr_backward)        %9.1f us / step   windows %s   spread (max - min) / median %.4f\n" % (s["plain_us_median"], f3(s["plain_us_windows"]), s["plain_spread"]))
            fh.write("  x requires grad (wdsr_backward_input)          %9.1f us / step   windows %s   spread %.4f\n" % (s["with_dx_us_median"], f3(s["with_dx_us_windows"]), s["with_dx_spread"]))
            fh.write("  d loss / d x costs                             %9.1f us / step   ratio %.4f   (margin: the plain leg's own spread, %.4f)\n\n" % (s["dx_cost_us"], s["with_dx_over_plain"], s["plain_spread"]))
            fh.write("(2) probav_input_grad alone, B = %d, T = %d, C = %d (device time per launch, %d launches per window after 20)\n" % (B, T, C, opt.launches))
            fh.write("  kernel %8.2f us %s   device copy moving the same %d bytes %8.2f us %s   ratio %.2f   kernel: %.2f TB/s of its own bytes\n\n"
                     % (k["fused_us"], f3(k["fused_us_windows"]), k["bytes_moved"], k["copy_us"], f3(k["copy_us_windows"]), k["fused_over_copy"], k["fused_tb_per_s"]))
            fh.write("(3) the same dx from existing parts (two probav_conv3d_forward launches on backward-data geometries, torch for the frames and 1 / std)\n")
            fh.write("  %8.2f us %s   %.1f x the kernel   fused against composed at this size: max |difference| / max |dx| = %.3e\n"
                     % (k["composed_us"], f3(k["composed_us_windows"]), k["composed_over_fused"], k["fused_vs_composed_max_err_over_max"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
