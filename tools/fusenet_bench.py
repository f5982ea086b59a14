#!/usr/bin/env python3
"""FuseNet, measured (one MI355X, one process, device events, alternated windows; one JSON line on stdout, --profile PATH also writes text).

At B = 16, 384 x 384 (one band's worth of stitched scenes per step) it times
  ours       torch.ops.probav.fusenet_forward, and forward + fusenet_backward (csrc/kernels_fusenet.hip)
  composed   the same network from torch ops on the device: F.conv2d on the explicitly (23, 24, 23, 24)-padded image, the normalisation by
             formula, leaky_relu, mean -- and its autograd for the parameter gradients
in windows that take turns (ours, composed, ours, ...), compares the two legs' branch m and filter gradient at the timed size, and records the
peak device memory of each leg.  By arithmetic alone the convolution is 2 * 384 * 384 * 2304 * 64 = 43.5 GFLOP per image each way; on the
fp32-input MFMA (157 TFLOP/s peak) that is 0.28 ms per image forward and the same for the filter gradient.

    python tools/fusenet_bench.py [--batch 16] [--size 384] [--iters 3] [--windows 3] [--profile profiles/fusenet_ab.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from probav_amd import fusenet_numpy as fn  # noqa: E402
from probav_amd import ops  # noqa: E402,F401


def timed(fn_, n, warm):
    """device milliseconds per call: n calls between two events, after `warm` calls"""
    for _ in range(warm):
        fn_()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn_()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def peak(fn_):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn_()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--size", type=int, default=384)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--profile", type=str, default=None)
    opt = p.parse_args()
    dev = torch.device("cuda:0")
    B, S = opt.batch, opt.size
    K, bias, gamma, beta = fn.init_params(0)
    flat = torch.tensor(fn.join_flat(K, bias, gamma, beta).astype(np.float32), device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randint(0, 16384, (B, S, S), device=dev, generator=gen).float()
    g = torch.randn(B, S, S, device=dev, generator=gen) / (B * S * S)

    def ours_fwd():
        return torch.ops.probav.fusenet_forward(x, flat, False)

    def ours_fwd_bwd():
        m, y, st = torch.ops.probav.fusenet_forward(x, flat, False)
        return m, torch.ops.probav.fusenet_backward(g, x, y, st, flat)

    def composed(params):
        Kt, bt, gt, be = params
        y = F.conv2d(F.pad(x[:, None], (23, 24, 23, 24)), Kt.permute(3, 2, 0, 1), bt)
        mu = y.mean((2, 3), keepdim=True)
        var = ((y - mu) ** 2).mean((2, 3), keepdim=True)
        a = gt.view(1, -1, 1, 1) * ((y - mu) * torch.rsqrt(var + fn.EPS)) + be.view(1, -1, 1, 1)
        return F.leaky_relu(a, fn.LEAK).mean(1)

    parts = [flat[:fn.N_KERNEL].view(48, 48, 1, 64), flat[fn.N_KERNEL:fn.N_KERNEL + 64], flat[fn.N_KERNEL + 64:fn.N_KERNEL + 128], flat[fn.N_KERNEL + 128:]]

    def comp_fwd():
        with torch.no_grad():
            return composed(parts)

    def comp_fwd_bwd():
        ps = [t.detach().clone().requires_grad_(True) for t in parts]
        m = composed(ps)
        (m * g).sum().backward()
        return m.detach(), ps[0].grad

    legs = {"ours_fwd": ours_fwd, "composed_fwd": comp_fwd, "ours_fwd_bwd": ours_fwd_bwd, "composed_fwd_bwd": comp_fwd_bwd}
    ms = {k: [] for k in legs}
    for _ in range(opt.windows):
        for k, f_ in legs.items():
            ms[k].append(timed(f_, opt.iters, 1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mem = {k: peak(f_) for k, f_ in legs.items()}
    m_o, d_o = ours_fwd_bwd()
    m_c, dK_c = comp_fwd_bwd()
    e_m = float((m_o - m_c).abs().max() / m_c.abs().max())
    e_dK = float((d_o[:fn.N_KERNEL].view(48, 48, 1, 64) - dK_c).abs().max() / dK_c.abs().max())
    gflop = 2.0 * S * S * 2304 * 64 * 1e-9
    res = {"tool": "fusenet_bench", "device": torch.cuda.get_device_name(0), "batch": B, "size": S, "iters": opt.iters, "windows": opt.windows, "ms_windows": ms,
           "ms_median": med, "peak_bytes": mem, "m_ours_vs_composed_max_err_over_max": e_m, "dK_ours_vs_composed_max_err_over_max": e_dK,
           "conv_gflop_per_image": gflop, "ours_fwd_ms_per_image": med["ours_fwd"] / B, "ours_bwd_ms_per_image": (med["ours_fwd_bwd"] - med["ours_fwd"]) / B,
           "ours_fwd_tflops": gflop * B / med["ours_fwd"], "ours_bwd_tflops": gflop * B / (med["ours_fwd_bwd"] - med["ours_fwd"])}
    if opt.profile:
        f3 = lambda v: ["%.2f" % q for q in v]
        with open(opt.profile, "w") as fh:
            fh.write("tools/fusenet_bench.py on %s: one process, device events, alternated windows (%d windows of %d calls after 1)\n\n" % (res["device"], opt.windows, opt.iters))
            fh.write("B = %d, %d x %d; the convolution is %.1f GFLOP per image each way\n" % (B, S, S, gflop))
            for k in legs:
                fh.write("  %-18s %9.2f ms   windows %s   peak memory %.2f GB\n" % (k, med[k], f3(ms[k]), mem[k] / 1e9))
            fh.write("\nours: forward %.3f ms per image (%.1f TFLOP/s of the convolution's arithmetic), backward %.3f ms per image (%.1f TFLOP/s)\n"
                     % (res["ours_fwd_ms_per_image"], res["ours_fwd_tflops"], res["ours_bwd_ms_per_image"], res["ours_bwd_tflops"]))
            fh.write("against the arithmetic floor of the fp32-input MFMA (157 TFLOP/s): %.3f ms per image each way\n" % (gflop / 157.0))
            fh.write("composed / ours: forward %.2f x, forward + backward %.2f x\n" % (med["composed_fwd"] / med["ours_fwd"], med["composed_fwd_bwd"] / med["ours_fwd_bwd"]))
            fh.write("the two legs at this size: max |m - m_composed| / max |m| = %.3e, max |dK - dK_composed| / max |dK| = %.3e (gates may differ where a ~ 0)\n" % (e_m, e_dK))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
