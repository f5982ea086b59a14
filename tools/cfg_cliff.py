"""Diagnostic (not part of the product): what a cfg value other than the shipped one costs.  The one-wave-per-SIMD kernels of round 5 have
instances for the shipped configuration only (patch 16 -> 22 x 22 rows, 9 or 7 frames in the residual blocks, decay 0.8 -> 25 channels, 32 filters); every other value
runs the general kernels of rounds 2 - 4 -- correct (tests/test_gpu_parity.py::test_other_patch_sizes_agree_across_engines), slower per voxel.  This prints, per
configuration, ms per training step (forward + shift-L1 + backward), patches/s, and the throughput per VOXEL-MAC relative to the shipped configuration.
    python tools/cfg_cliff.py            (on the GPU box, from the repo root)
    --gemm-route       the table with the engine's general matrix route on (WDSRModel.set_gemm_route; INTEGRATION.md, 'The general matrix route')
    --filters F        only the num_filters = F row (batch 128, 12 blocks, expansion --exp, default 8)
    --ab               per row, the route off and on ALTERNATED in one process on one model: --windows windows per leg (default 3) of --steps steps each, timed
                       with device events; ms per step off / on, their ratio, the off leg's own window-to-window spread, the training workspace bytes off / on,
                       and the TFLOP/s of the fp32 kernel classes (probav_engine_profile: what the route's launches are booked under) with the route on
    --gemm-route --pair   the table with the route and its fused pointwise pair on
    --gemm-route [--pair] --x6   the table with the route's convolution launches in x6 arithmetic (WDSRModel.set_gemm_x6)
    --ab --pair        the same A/B with the route ON in both legs and the route's fused pointwise pair (WDSRModel.set_gemm_pair) alternated: ms per step pair off / on,
                       the off leg's spread, probav_workspace_bytes(e, B, 1) and the device memory in use at the end of each leg (workspace blocks released between legs), and the TFLOP/s of the pair's two launches
                       (classes pw_fwd / pw_bwd_data, algorithmic MACs F H + H D forward and 3 F H + 2 H D in reverse per voxel)
    --ab --x6          the same A/B with the route AND the pair on in both legs (the last row: the pair off) and the route's x6 arithmetic (WDSRModel.set_gemm_x6)
                       alternated: ms per step x6 off / on -- the off leg is the fp32 route, the yardstick of the same run --, the off leg's spread, whether on is
                       below off by more than three times that spread, and the TFLOP/s of the route's kernel classes in each leg (fp32 classes off, _x6 classes on)
                       against the published peaks: 157.3 TFLOP/s fp32 matrix, 2500 / 6 = 417 TFLOP/s of fp32-equivalent products in x6
    --ab --exotic      the same A/B with the route, the pair AND x6 on in both legs (one row: x6 off) and the route's exotic launches (WDSRModel.set_gemm_exotic)
                       alternated: the 19-frame rows, which have nine such launches a step, and the 9-frame 64-filter and shipped rows, which have none and must
                       not move; ms per step off / on, the off leg's spread, the census and the training workspace bytes of each leg, and the kernel classes of each leg"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from probav_amd import _lib as L
from probav_amd import ops, synth
from probav_amd.loss import Losses
from probav_amd.modelsTF import WDSRConv3D

dev = torch.device("cuda:0")
FP32_PEAK_TFLOPS = 157.3          # MI355X fp32 matrix peak, as published (not measured here)
FP32_CLASSES = (2, 3, 4, 5, 6, 7)   # engine.hip: conv3 fwd / bwd-data / wgrad, 1x1x1 fwd / bwd-data / wgrad -- the fp32 (VALU, fp32-MFMA, general matrix route) launches


def macs_per_patch(P, T, F=32, E=8, decay=0.8, R=12):
    """forward MACs of one patch (SURVEY.md section 8a's table, for any P / T / decay): residual blocks only -- the part the round-5 kernels serve."""
    H = P + 6
    D = int(F * decay)
    V = H * H * T
    return R * V * (F * F * E + F * E * D + 27 * D * F)


def build(P, T, B, decay, F, E, gemm, pair=False, x6=False):
    model = WDSRConv3D("cliff", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, F, (3, 3, 3), 12, E, decay, T, P, True, seed=0)
    model = model.to(dev)
    if gemm:
        model.set_gemm_route(True)
    if pair:
        model.set_gemm_pair(True)
    if x6:
        model.set_gemm_x6(True)
    rng = np.random.default_rng(1)
    H = P + 6
    x = torch.as_tensor(np.clip(rng.normal(synth.NIR_MEAN, synth.NIR_STD, (B, H, H, T, 1)), 0, 16383).astype(np.float32)).to(dev)
    hr = torch.as_tensor(np.clip(rng.normal(synth.NIR_MEAN, synth.NIR_STD, (B, 3 * P, 3 * P, 1)), 0, 16383).astype(np.float32)).to(dev)
    mask = torch.as_tensor(rng.random((B, 3 * P, 3 * P, 1)) < 0.9).to(dev)
    losses = Losses(targetShape=(3 * P, 3 * P, 1))

    def step():
        pred = model(x, training=True)
        loss = losses.shiftCompensatedL1Loss(hr, mask, pred)
        model.flat.grad = None
        loss.backward()
    return model, step


def timed(step, steps):
    """ms of each of `steps` steps, by device events."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(steps):
        step()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]


def release(model):
    model._ws.clear()
    del model
    torch.cuda.empty_cache()


def run(P, T, B, decay=0.8, F=32, steps=30, E=8, gemm=False, pair=False, x6=False):
    model, step = build(P, T, B, decay, F, E, gemm, pair, x6)
    for _ in range(5):
        step()
    ms = sorted(timed(step, steps))
    release(model)
    return ms[len(ms) // 2]


def fp32_class_tflops(model, step):
    """TFLOP/s (2 x algorithmic MACs / bracketed time) of the fp32 classes over one step, everything on the launch stream."""
    h = model._handle()
    n = 13
    model.set_side_stream_mode(0)
    L.check(L.lib().probav_engine_profile(h, 1, 4096), "probav_engine_profile")
    try:
        step()
        torch.cuda.synchronize()
        ms, macs, cnt = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_int64 * n)()
        L.check(L.lib().probav_engine_profile_read(h, n, ms, macs, cnt), "probav_engine_profile_read")
    finally:
        L.check(L.lib().probav_engine_profile(h, 0, 0), "probav_engine_profile")
        model.set_side_stream_mode(2)
    t, m, k = (sum(a[c] for c in FP32_CLASSES) for a in (ms, macs, cnt))
    return (2.0 * m / (t * 1e-3) / 1e12 if t > 0 else 0.0), t, int(k)


def run_ab(P, T, B, decay, F, E, steps, windows):
    model, step = build(P, T, B, decay, F, E, False)
    h = model._handle()
    legs, ws = {False: [], True: []}, {}
    for w in range(windows):
        for on in (False, True):
            model.set_gemm_route(on)
            ws[on] = int(L.lib().probav_workspace_bytes(h, B, 1))
            step()
            step()                                              # (the switch resizes the reverse pass's scratch: the first steps allocate)
            legs[on].append(sum(timed(step, steps)) / steps)
    counts = (ctypes.c_int32 * 4)()
    model.set_gemm_route(True)
    L.check(L.lib().probav_engine_route_counts(h, B, ctypes.byref(counts)), "probav_engine_route_counts")
    tf, tms, launches = fp32_class_tflops(model, step)
    release(model)
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(legs[False]), med(legs[True])
    return {"ms_per_step_off": round(off, 3), "ms_per_step_on": round(on, 3), "on_over_off": round(on / off, 4),
            "off_windows_ms": [round(v, 3) for v in legs[False]], "on_windows_ms": [round(v, 3) for v in legs[True]],
            "off_spread": round((max(legs[False]) - min(legs[False])) / off, 4),
            "train_workspace_bytes_off": ws[False], "train_workspace_bytes_on": ws[True], "route_launches_conv_wgrad": [counts[1], counts[3]],
            "valu_launches_left_conv_wgrad": [counts[0], counts[2]],
            "fp32_classes_on": {"launches": launches, "ms": round(tms, 3), "tflops": round(tf, 2), "of_fp32_matrix_peak_157.3": round(tf / FP32_PEAK_TFLOPS, 4)}}


def class_tflops(model, step, classes):
    """{class: (TFLOP/s, ms, launches)} of one step with every launch on the launch stream (probav_engine_profile)."""
    h, n = model._handle(), 13
    model.set_side_stream_mode(0)
    L.check(L.lib().probav_engine_profile(h, 1, 4096), "probav_engine_profile")
    try:
        step()
        torch.cuda.synchronize()
        ms, macs, cnt = (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_int64 * n)()
        L.check(L.lib().probav_engine_profile_read(h, n, ms, macs, cnt), "probav_engine_profile_read")
    finally:
        L.check(L.lib().probav_engine_profile(h, 0, 0), "probav_engine_profile")
        model.set_side_stream_mode(2)
    return {c: ((2.0 * macs[c] / (ms[c] * 1e-3) / 1e12 if ms[c] > 0 else 0.0), ms[c], int(cnt[c])) for c in classes}


def run_ab_pair(P, T, B, decay, F, E, steps, windows):
    """run_ab with the route on in both legs and the fused pointwise pair alternated."""
    model, step = build(P, T, B, decay, F, E, True)
    h = model._handle()
    legs, ws, peak, kind = {False: [], True: []}, {}, {False: 0, True: 0}, {}
    for w in range(windows):
        for on in (False, True):
            model.set_gemm_pair(on)
            kind[on] = int(L.lib().probav_engine_pair_kind(h))
            ws[on] = int(L.lib().probav_workspace_bytes(h, B, 1))
            model._ws.clear()
            ops.release_workspaces(dev)                         # (the other leg's blocks go back to the driver, so that what the device holds below is this leg's own)
            step()
            step()
            legs[on].append(sum(timed(step, steps)) / steps)
            free, total = torch.cuda.mem_get_info(dev)          # nothing is handed back during a leg: what the process holds now is the most it held
            peak[on] = max(peak[on], int(total - free))
    model.set_gemm_pair(True)
    cls = class_tflops(model, step, (5, 6))
    release(model)
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(legs[False]), med(legs[True])
    spread = (max(legs[False]) - min(legs[False])) / off
    pair = {name: {"launches": cls[c][2], "ms": round(cls[c][1], 3), "tflops": round(cls[c][0], 2), "of_fp32_matrix_peak_157.3": round(cls[c][0] / FP32_PEAK_TFLOPS, 4)}
            for name, c in (("pw_fwd", 5), ("pw_bwd_data", 6))}
    return {"pair_kind_off_on": [kind[False], kind[True]], "ms_per_step_pair_off": round(off, 3), "ms_per_step_pair_on": round(on, 3), "on_over_off": round(on / off, 4),
            "off_windows_ms": [round(v, 3) for v in legs[False]], "on_windows_ms": [round(v, 3) for v in legs[True]], "off_spread": round(spread, 4),
            "faster_by_more_than_the_spread": bool(off - on > spread * off),
            "train_workspace_bytes_off": ws[False], "train_workspace_bytes_on": ws[True], "device_bytes_in_use_off": peak[False], "device_bytes_in_use_on": peak[True],
            "pair_classes_on": pair}


X6_PEAK_TFLOPS = 2500.0 / 6        # MI355X dense bf16 matrix peak, as published, over the six piece products of one fp32 product (not measured here)
CLASS_NAMES = ("wn", "small", "conv3_fwd", "conv3_bwd_data", "conv3_wgrad", "pw_fwd", "pw_bwd_data", "pw_wgrad", "conv3_fwd_x6", "conv3_bwd_data_x6", "conv3_wgrad_x6",
               "pw_fwd_x6", "pw_bwd_data_x6")


def run_ab_x6(P, T, B, decay, F, E, steps, windows, pair=True):
    """run_ab with the route (and, pair=True, its fused pair) on in both legs and the route's x6 arithmetic alternated.  No size moves with the switch."""
    model, step = build(P, T, B, decay, F, E, True, pair)
    h = model._handle()
    legs, arith, cls = {False: [], True: []}, {}, {}
    for w in range(windows):
        for on in (False, True):
            model.set_gemm_x6(on)
            arith[on] = int(L.lib().probav_engine_gemm_arith(h))
            step()
            step()
            legs[on].append(sum(timed(step, steps)) / steps)
    for on in (False, True):
        model.set_gemm_x6(on)
        got = class_tflops(model, step, range(2, 13))
        # (the backward-filter classes are the fp32 route's in both legs)
        cls[on] = {CLASS_NAMES[c]: {"launches": v[2], "ms": round(v[1], 3), "tflops": round(v[0], 2),
                                    "of_peak": round(v[0] / (X6_PEAK_TFLOPS if c >= 8 else FP32_PEAK_TFLOPS), 4)} for c, v in got.items() if v[2]}
    kind = int(L.lib().probav_engine_pair_kind(h))
    release(model)
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(legs[False]), med(legs[True])
    spread = (max(legs[False]) - min(legs[False])) / off
    return {"pair_kind": kind, "gemm_arith_off_on": [arith[False], arith[True]], "ms_per_step_x6_off": round(off, 3), "ms_per_step_x6_on": round(on, 3), "on_over_off": round(on / off, 4),
            "off_windows_ms": [round(v, 3) for v in legs[False]], "on_windows_ms": [round(v, 3) for v in legs[True]], "off_spread": round(spread, 4),
            "faster_by_more_than_three_spreads": bool(off - on > 3 * spread * off), "classes_off": cls[False], "classes_on": cls[True]}


def run_ab_exotic(P, T, B, decay, F, E, steps, windows, x6=True):
    """run_ab with the route, its fused pair and (x6=True) its x6 arithmetic on in both legs and the route's exotic launches alternated.  The reverse scratch
    moves with the switch at 19 frames."""
    model, step = build(P, T, B, decay, F, E, True, True, x6)
    h = model._handle()
    legs, ws, census, cls = {False: [], True: []}, {}, {}, {}
    for w in range(windows):
        for on in (False, True):
            model.set_gemm_exotic(on)
            ws[on] = int(L.lib().probav_workspace_bytes(h, B, 1))
            counts = (ctypes.c_int32 * 4)()
            L.check(L.lib().probav_engine_route_counts(h, B, ctypes.byref(counts)), "probav_engine_route_counts")
            census[on] = list(counts)
            step()
            step()                                              # (the switch resizes the reverse pass's scratch: the first steps allocate)
            legs[on].append(sum(timed(step, steps)) / steps)
    for on in (False, True):
        model.set_gemm_exotic(on)
        got = class_tflops(model, step, range(2, 13))
        cls[on] = {CLASS_NAMES[c]: {"launches": v[2], "ms": round(v[1], 3), "tflops": round(v[0], 2),
                                    "of_peak": round(v[0] / (X6_PEAK_TFLOPS if c >= 8 else FP32_PEAK_TFLOPS), 4)} for c, v in got.items() if v[2]}
    arith = int(L.lib().probav_engine_gemm_arith(h))
    release(model)
    med = lambda v: sorted(v)[len(v) // 2]
    off, on = med(legs[False]), med(legs[True])
    spread = (max(legs[False]) - min(legs[False])) / off
    return {"gemm_arith": arith, "ms_per_step_exotic_off": round(off, 3), "ms_per_step_exotic_on": round(on, 3), "on_over_off": round(on / off, 4),
            "off_windows_ms": [round(v, 3) for v in legs[False]], "on_windows_ms": [round(v, 3) for v in legs[True]], "off_spread": round(spread, 4),
            "faster_by_more_than_three_spreads": bool(off - on > 3 * spread * off), "inside_one_spread": bool(abs(off - on) <= spread * off),
            "census_off": census[False], "census_on": census[True], "train_workspace_bytes_off": ws[False], "train_workspace_bytes_on": ws[True],
            "classes_off": cls[False], "classes_on": cls[True]}


# name, P, T, B, decay, F, E
TABLE = (("shipped: patch 16, 9 frames, decay 0.8", 16, 9, 128, 0.8, 32, 8),
         ("7 frames", 16, 7, 128, 0.8, 32, 8),
         ("13 frames (reducer v3)", 16, 13, 128, 0.8, 32, 8),
         ("19 frames (experimental reducer)", 16, 19, 64, 0.8, 32, 8),
         ("patch 32 (38 x 38 rows)", 32, 9, 40, 0.8, 32, 8),
         ("patch 24 (30 x 30 rows)", 24, 9, 64, 0.8, 32, 8),
         ("decay 0.5 (16 channels)", 16, 9, 128, 0.5, 32, 8),
         ("decay 0.9 (28 channels)", 16, 9, 128, 0.9, 32, 8),
         ("filters 64 (51 channels)", 16, 9, 128, 0.8, 64, 8),
         ("filters 48 / exp 6 (43 channels)", 16, 9, 128, 0.9, 48, 6))
# the rows of --ab: the shipped one (which must not move), the cfg values the route is for, 13 frames at 64 filters
AB_TABLE = (TABLE[0], TABLE[6], TABLE[7], TABLE[8], TABLE[9], ("filters 64, 13 frames", 16, 13, 128, 0.8, 64, 8))
# the rows of --ab --pair: the shapes the general pair takes, and the shipped one (which keeps its tuned pair and must not move)
PAIR_TABLE = (TABLE[8], TABLE[9], TABLE[7], AB_TABLE[5], TABLE[0])
# the rows of --ab --x6: the pair's rows with the pair on, and the 64-filter row with the pair off, where the pointwise launches change hands too
X6_TABLE = tuple(r + (True,) for r in PAIR_TABLE) + ((TABLE[8][0] + ", pair off",) + TABLE[8][1:] + (False,),)
# the rows of --ab --exotic: 19 frames at the shipped channels and at 64 filters (x6 on, and off), and the two rows without an exotic launch, which must not move
EXOTIC_TABLE = (TABLE[3] + (True,), ("19 frames, filters 64", 16, 19, 64, 0.8, 64, 8, True), ("19 frames, filters 64, x6 off", 16, 19, 64, 0.8, 64, 8, False),
                TABLE[8] + (True,), TABLE[0] + (True,))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gemm-route", dest="gemm_route", action="store_true")
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--exp", type=int, default=8)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--pair", action="store_true")
    ap.add_argument("--x6", action="store_true")
    ap.add_argument("--exotic", action="store_true")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--windows", type=int, default=3)
    opt = ap.parse_args()
    if opt.pair and not (opt.ab or opt.gemm_route):
        ap.error("--pair needs --ab or --gemm-route")
    if opt.x6 and not (opt.ab or opt.gemm_route):
        ap.error("--x6 needs --ab or --gemm-route")
    if opt.x6 and opt.ab and opt.pair:
        ap.error("--ab --x6 has the pair on in its legs: no --pair")
    if opt.exotic and (not opt.ab or opt.pair or opt.x6):
        ap.error("--exotic is --ab --exotic: the route, the pair and x6 are on in its legs")
    if opt.exotic:
        for name, P, T, B, decay, F, E, x6 in (r for r in EXOTIC_TABLE if opt.filters is None or r[5] == opt.filters):
            print(json.dumps(dict({"config": name, "batch": B}, **run_ab_exotic(P, T, B, decay, F, E, opt.steps or 4, opt.windows, x6))), flush=True)
        sys.exit(0)
    table = (PAIR_TABLE if opt.pair else AB_TABLE) if opt.ab else TABLE
    if opt.x6 and opt.ab:
        table = tuple(r for r in X6_TABLE if opt.filters is None or r[5] == opt.filters)
        for name, P, T, B, decay, F, E, pair in table:
            print(json.dumps(dict({"config": name, "batch": B}, **run_ab_x6(P, T, B, decay, F, E, opt.steps or 4, opt.windows, pair))), flush=True)
        sys.exit(0)
    if opt.filters is not None:
        table = (("filters %d / exp %d" % (opt.filters, opt.exp), 16, 9, 128, 0.8, opt.filters, opt.exp),)
    rows = []
    base = None
    for name, P, T, B, decay, F, E in table:
        try:
            if opt.ab:
                rows.append(dict({"config": name, "batch": B}, **(run_ab_pair if opt.pair else run_ab)(P, T, B, decay, F, E, opt.steps or 4, opt.windows)))
                print(json.dumps(rows[-1]), flush=True)
                continue
            med = run(P, T, B, decay, F, opt.steps or 30, E, opt.gemm_route, opt.pair, opt.x6)
        except Exception as ex:                                   # a configuration the engine refuses is a row of the table too
            rows.append({"config": name, "error": str(ex)[:200]})
            print(json.dumps(rows[-1]), flush=True)
            continue
        gmacs = macs_per_patch(P, T, F, E, decay) * B / (med * 1e-3) / 1e9
        if base is None:
            base = gmacs
        rows.append({"config": name, "batch": B, "gemm_route": bool(opt.gemm_route), "gemm_pair": bool(opt.pair), "ms_per_step_median": round(med, 3), "patches_per_s": round(B / (med * 1e-3), 1),
                     "block_GMAC_per_s": round(gmacs, 1), "per_mac_throughput_vs_shipped": round(gmacs / base, 3)})
        print(json.dumps(rows[-1]), flush=True)
