#!/usr/bin/env python3
"""Scoring kernel timing (csrc/kernels_score.hip) on seeded 384 x 384 images of ESA size (1160 train sets): one JSON line with
  device_ms / us_per_image    probav_score_moments + probav_score_select on device-resident inputs (events; warm-up; median of --repeats)
  valu_bound_ms / share       the cost model of the kernel's header: 7 VALU ops per pixel-shift at 78.6 Tops/s int32, and measured / model
  numpy_oracle_est_s          the int64 numpy oracle (tests/score_oracle.py's moments) timed on --oracle-images images and EXTRAPOLATED
    python tools/score_bench.py [--images 1160 --repeats 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_OPS_PER_VISIT, INT32_VALU_OPS_PER_S = 7, 78.6e12


def images(n, rng, S=384):
    hr = rng.integers(1000, 30000, (n, S, S)).astype(np.uint16)
    sr = np.clip(hr.astype(np.int64) + rng.integers(-300, 300, (n, S, S)), 0, 65535).astype(np.uint16)
    return sr, hr, rng.random((n, S, S)) < 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1160)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--oracle-images", type=int, default=4)
    opt = ap.parse_args()
    import torch
    from probav_amd import _lib, scoring
    dev = torch.device("cuda")
    S, border = 384, 3
    sr, hr, mask = images(opt.images, np.random.default_rng(0))
    s, h, m = scoring._to_device_u16(sr, dev), scoring._to_device_u16(hr, dev), scoring._to_device_mask(mask, dev).view(torch.uint8)
    N, ns = opt.images, (2 * border + 1) ** 2
    mom = torch.empty((N, ns, 3), dtype=torch.int64, device=dev)
    cp, sh, bi, nc = (torch.empty(N, dtype=torch.float64, device=dev), torch.empty((N, 2), dtype=torch.int32, device=dev),
                      torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev))
    L = _lib.lib()

    def run():
        _lib.check(L.probav_score_moments(_lib.ptr(s), _lib.ptr(h), _lib.ptr(m), N, S, border, _lib.ptr(mom), _lib.current_stream()))
        _lib.check(L.probav_score_select(_lib.ptr(mom), N, border, _lib.ptr(cp), _lib.ptr(sh), _lib.ptr(bi), _lib.ptr(nc), _lib.current_stream()))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(opt.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    dev_ms = float(np.median(times))
    t0 = time.perf_counter()
    res = scoring.shift_cpsnr(sr, hr, mask, border)                # with the host -> device copies
    wall_s = time.perf_counter() - t0
    visits = N * ns * (S - 2 * border) ** 2
    bound_ms = visits * VALU_OPS_PER_VISIT / INT32_VALU_OPS_PER_S * 1e3
    from tests import score_oracle
    k = opt.oracle_images
    t0 = time.perf_counter()
    want = score_oracle.moments(sr[:k], hr[:k], mask[:k], border)
    np_s = (time.perf_counter() - t0) * N / k
    assert np.array_equal(mom[:k].cpu().numpy(), want) and np.isfinite(res["cpsnr"]).all()
    print(json.dumps({"images": N, "S": S, "border": border, "device_ms": round(dev_ms, 3), "us_per_image": round(dev_ms * 1e3 / N, 3),
                      "valu_bound_ms": round(bound_ms, 3), "share_of_valu_bound": round(bound_ms / dev_ms, 3),
                      "wall_s_with_copies": round(wall_s, 3), "numpy_oracle_est_s": round(np_s, 1),
                      "numpy_oracle_est_note": "extrapolated from %d images" % k}))


if __name__ == "__main__":
    main()
