#!/usr/bin/env python3
"""The bicubic-mean baseline kernel, measured (one process, one box, one JSON line on stdout; --profile PATH also writes the figures as text):

  check      two sets of the workload against baseline.baseline_numpy, bit for bit, both modes, before anything is timed.
  A/B        torch.ops.probav.baseline_upscale_mean on one band's worth of device-resident image sets (--sets sets of 9..35 frames of 128 x 128,
             seeded) against a device copy that moves the same bytes: the kernel's bytes read plus written, counted from the shapes (frames
             2 B and masks 1 B per LR pixel of every frame it fetches, 36 B per LR pixel of every set written; the 2-pixel halo is not counted),
             as a copy of half that many bytes (a copy reads and writes each one).  Interleaved windows of --iters calls each (after --warmup),
             device time between events around a window; medians over the windows, the kernel over the copy, and the spread of the copy
             windows among themselves.

    python tools/baseline_bench.py [--sets 594] [--iters 20] [--windows 5] [--profile profiles/baseline_bench.txt]

There is no pass bar: no earlier path computes this.  The copy is the floor a kernel bound by memory traffic could reach.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from probav_amd import baseline, ops  # noqa: E402,F401

H = W = 128


def workload(n_sets, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(9, 36, n_sets)
    F = int(sizes.sum())
    frames = rng.integers(0, 65536, (F, H, W), dtype=np.uint16)
    clear = rng.integers(0, 100, (F, H, W), dtype=np.uint8) < 85
    for s, o in enumerate(np.cumsum(sizes) - sizes):
        if s % 3 == 0:
            clear[o:o + 2] = True                              # every third set has two frames tied at the maximum
    return frames, clear.view(np.uint8), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def traffic_bytes(clear, offsets, mode):
    """Bytes the kernel has to move, from the shapes: (read, written)."""
    F, S = len(clear), len(offsets) - 1
    written = S * 9 * H * W * 4
    if mode == "clear":
        return F * H * W * 3, written
    fetched = int(baseline.selected_frames_numpy(clear, offsets).sum())
    return F * H * W * 1 + fetched * H * W * 2, written         # every mask once for the counts, the chosen frames only


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sets", type=int, default=594)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    if opt.windows < 3:
        raise SystemExit("at least three windows per leg")
    if not torch.cuda.is_available():
        raise SystemExit("tools/baseline_bench.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    frames, clear, offsets = workload(opt.sets, opt.seed)
    f = torch.from_numpy(frames.view(np.int16)).to(dev).view(torch.uint16)
    c, o = torch.from_numpy(clear).to(dev), torch.from_numpy(offsets).to(dev)

    nchk = int(offsets[2])
    for mode in baseline.MODES:
        want, want_k = baseline.baseline_numpy(frames[:nchk], clear[:nchk], offsets[:3], mode)
        got, got_k = torch.ops.probav.baseline_upscale_mean(f[:nchk], c[:nchk], o[:3], mode)
        if not (np.array_equal(got.cpu().numpy(), want) and got_k.cpu().tolist() == want_k.tolist()):
            raise SystemExit("baseline_upscale_mean (%s) does NOT equal baseline_numpy on the first two sets" % mode)

    res = {"tool": "baseline_bench", "device": torch.cuda.get_device_name(0), "sets": opt.sets, "frames": int(len(frames)), "lr_size": H,
           "iters_per_window": opt.iters, "windows": opt.windows, "equals_numpy_on_two_sets": True, "modes": {}}
    lines = []
    for mode in baseline.MODES:
        rd, wr = traffic_bytes(clear, offsets, mode)
        half = (rd + wr) // 2
        src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        legs = {"kernel": lambda: torch.ops.probav.baseline_upscale_mean(f, c, o, mode), "copy": lambda: dst.copy_(src)}
        for fn in legs.values():
            for _ in range(opt.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(opt.windows):                               # A B A B ...: both legs see the same drift of the box
            for k, fn in legs.items():
                ms[k].append(window(fn, opt.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = (max(ms["copy"]) - min(ms["copy"])) / med["copy"]
        res["modes"][mode] = {"bytes_read": rd, "bytes_written": wr, "kernel_ms_windows": ms["kernel"], "copy_ms_windows": ms["copy"],
                              "kernel_ms_median": med["kernel"], "copy_ms_median": med["copy"], "kernel_over_copy": med["kernel"] / med["copy"],
                              "kernel_tb_per_s": (rd + wr) / med["kernel"] * 1e-9, "copy_tb_per_s": 2 * half / med["copy"] * 1e-9,
                              "copy_windows_spread_over_median": spread}
        lines += ["mode %s: %d bytes read + %d written = %.1f MB (from the shapes; halo not counted)" % (mode, rd, wr, (rd + wr) / 1e6),
                  "  kernel (the op, its allocations included)   %.4f ms / call  %.2f TB/s   windows %s" % (med["kernel"], (rd + wr) / med["kernel"] * 1e-9, ["%.4f" % v for v in ms["kernel"]]),
                  "  device copy of the same bytes               %.4f ms / call  %.2f TB/s   windows %s" % (med["copy"], 2 * half / med["copy"] * 1e-9, ["%.4f" % v for v in ms["copy"]]),
                  "  kernel / copy                               %.3f   (spread of the copy windows: %.4f of their median)" % (med["kernel"] / med["copy"], spread), ""]
        del src, dst
    if opt.profile:
        with open(opt.profile, "w") as fh:
            fh.write("tools/baseline_bench.py on %s: one process, same box, interleaved windows\n\n" % res["device"])
            fh.write("%d image sets, %d frames of %d x %d, device-resident; %d windows of %d calls per leg, medians of the windows\n" % (opt.sets, len(frames), H, W, opt.windows, opt.iters))
            fh.write("the first two sets equal baseline_numpy bit for bit in both modes\n\n")
            fh.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
