#!/usr/bin/env python3
"""cSSIM kernel timing (csrc/kernels_ssim.hip) on one band's worth of seeded, device-resident 384 x 384 images: one JSON line (also
written to --out) with
  fused_ms / us_per_image     probav_ssim_table on resident inputs and moments (device events; warm-up; median of --repeats windows)
  cpsnr_ms / x_cpsnr          probav_score_moments + probav_score_select on the same images, timed in alternation with the fused leg
  composed_ms / x_composed    the same table composed on the device from torch ops: fp64 conv2d with the separable taps, 49 shifts, five
                              maps each, in chunks of --chunk images (slices and multiply-adds if conv2d refuses fp64); alternated too
  numpy_s_per_image           scoring.cssim_table_numpy timed on --numpy-images images; numpy_est_s EXTRAPOLATES it to --images
  fp64_model_ms / share       the cost model of the kernel's header (316 VALU instructions per window and shift in the gfx950 code) at the
                              MI355X's published 78.6 TFLOP/s vector fp64 = 39.3e12 operations/s, and model / measured
  max_abs_fused_vs_composed   at the timed size;  max_abs_fused_vs_numpy on the --numpy-images images
    python tools/ssim_bench.py [--images 580 --repeats 5 --composed-repeats 2 --out profiles/ssim_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_OPS_PER_WINDOW_SHIFT, FP64_VALU_OPS_PER_S = 316, 39.3e12


def images(n, rng, S=384):
    hr = rng.integers(1000, 30000, (n, S, S)).astype(np.uint16)
    sr = np.clip(hr.astype(np.int64) + rng.integers(-300, 300, (n, S, S)), 0, 65535).astype(np.uint16)
    return sr, hr, rng.random((n, S, S)) < 0.9


def composed_table(s, h, m, border, g, chunk, how):
    """The direct form of the definition from torch ops, fp64, on the device."""
    import torch
    import torch.nn.functional as F
    N, S = s.shape[0], s.shape[1]
    ns, L = 2 * border + 1, S - 2 * border
    K = L - 10
    C1, C2 = (0.01 * 65535.0) ** 2, (0.03 * 65535.0) ** 2
    dbl = lambda t: (t.view(torch.int16).to(torch.int32) & 0xFFFF).double()

    def filt(a):                                            # [n, 5, L, L] -> [n, 5, K, K]: rows first, then columns
        if how == "conv2d":
            a = a.reshape(-1, 1, L, L)
            return F.conv2d(F.conv2d(a, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1)).reshape(-1, 5, K, K)
        rows = sum(g[q] * a[..., :, q:q + K] for q in range(11))
        return sum(g[p] * rows[..., p:p + K, :] for p in range(11))

    out = torch.full((N, ns * ns), float("nan"), dtype=torch.float64, device=s.device)
    for i in range(0, N, chunk):
        P = dbl(s[i:i + chunk, border:border + L, border:border + L])
        for u in range(ns):
            for v in range(ns):
                H = dbl(h[i:i + chunk, u:u + L, v:v + L])
                md = m[i:i + chunk, u:u + L, v:v + L].double()
                n = md.sum((1, 2))
                bias = (md * (H - P)).sum((1, 2)) / n
                x, y = md * (P + bias[:, None, None]), md * H
                mx, my, fxx, fyy, fxy = filt(torch.stack([x, y, x * x, y * y, x * y], 1)).unbind(1)
                vx, vy, cxy = fxx - mx * mx, fyy - my * my, fxy - mx * my
                val = (((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))).mean((1, 2))
                out[i:i + chunk, u * ns + v] = torch.where(n > 0, val, torch.full_like(val, float("nan")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=580)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--composed-repeats", type=int, default=2, help="the composed leg takes seconds: it joins only the first windows")
    ap.add_argument("--chunk", type=int, default=58)
    ap.add_argument("--numpy-images", type=int, default=3)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ssim_bench.txt"))
    opt = ap.parse_args()
    import torch
    from probav_amd import _lib, scoring
    dev = torch.device("cuda")
    S, border = 384, 3
    N, ns = opt.images, (2 * border + 1) ** 2
    sr, hr, mask = images(N, np.random.default_rng(0))
    s, h, m = scoring._to_device_u16(sr, dev), scoring._to_device_u16(hr, dev), scoring._to_device_mask(mask, dev).view(torch.uint8)
    L = _lib.lib()
    g = torch.from_numpy(scoring.gauss11()).to(dev)
    mom = torch.empty((N, ns, 3), dtype=torch.int64, device=dev)
    cp, sh, bi, nc = (torch.empty(N, dtype=torch.float64, device=dev), torch.empty((N, 2), dtype=torch.int32, device=dev),
                      torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev))
    nbytes = L.probav_ssim_scratch_bytes(N, S, border)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    table = torch.empty((N, ns), dtype=torch.float64, device=dev)

    def cpsnr():
        _lib.check(L.probav_score_moments(_lib.ptr(s), _lib.ptr(h), _lib.ptr(m), N, S, border, _lib.ptr(mom), _lib.current_stream()))
        _lib.check(L.probav_score_select(_lib.ptr(mom), N, border, _lib.ptr(cp), _lib.ptr(sh), _lib.ptr(bi), _lib.ptr(nc), _lib.current_stream()))

    def fused():
        _lib.check(L.probav_ssim_table(_lib.ptr(s), _lib.ptr(h), _lib.ptr(m), _lib.ptr(mom), _lib.ptr(g), N, S, border, _lib.ptr(scratch), nbytes,
                                       _lib.ptr(table), _lib.current_stream()))

    how = "conv2d"
    comp = None
    if not opt.no_composed:
        try:
            composed_table(s[:2], h[:2], m[:2], border, g, 2, how)
        except RuntimeError:
            how = "slices"

        def composed():
            nonlocal comp
            comp = composed_table(s, h, m, border, g, opt.chunk, how)
    legs = [("cpsnr", cpsnr), ("fused", fused)] + ([] if opt.no_composed else [("composed", composed)])
    cpsnr()
    fused()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for r in range(opt.repeats):                            # alternated windows: every repeat times each leg once, in turn
        for name, fn in legs:
            if name == "composed" and r >= opt.composed_repeats:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    k = opt.numpy_images
    t0 = time.perf_counter()
    want = scoring.cssim_table_numpy(sr[:k], hr[:k], mask[:k], border)
    np_s = (time.perf_counter() - t0) / k
    got = table.cpu().numpy()
    K = S - 2 * border - 10
    model_ms = N * ns * K * K * VALU_OPS_PER_WINDOW_SHIFT / FP64_VALU_OPS_PER_S * 1e3
    res = {"images": N, "S": S, "border": border, "fused_ms": round(med["fused"], 3), "us_per_image": round(med["fused"] * 1e3 / N, 2),
           "cpsnr_ms": round(med["cpsnr"], 3), "x_cpsnr": round(med["fused"] / med["cpsnr"], 1),
           "fp64_model_ms": round(model_ms, 3), "share_of_fp64_valu_model": round(model_ms / med["fused"], 3),
           "numpy_s_per_image": round(np_s, 3), "numpy_est_s": round(np_s * N, 1), "numpy_est_note": "extrapolated from %d images" % k,
           "x_numpy": round(np_s * N * 1e3 / med["fused"], 0), "max_abs_fused_vs_numpy": float(np.abs(got[:k] - want).max())}
    if not opt.no_composed:
        res.update({"composed_ms": round(med["composed"], 1), "composed_how": how, "x_composed": round(med["composed"] / med["fused"], 1),
                    "max_abs_fused_vs_composed": float((table - comp).abs().max())})
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        fh.write("tools/ssim_bench.py --images %d --repeats %d (median of alternated windows, device events)\n%s\n" % (N, opt.repeats, line))


if __name__ == "__main__":
    main()
