#!/usr/bin/env python3
"""Dataset builder timing on a synthetic corpus of ESA size (1160 train + 290 test sets, 9-35 frames of 128 x 128, textures rolled by
small shifts plus noise): one JSON line with
  stage2_device_ms / us_per_frame   the count + registration kernels (device events around probav_prep_count_nonzero + probav_prep_register)
  stage34_wall_s                    patch unfold (device) + pickClearPatchesLR / pickClearPatches bookkeeping of the train LR / HR patches
  png_decode_ms_per_frame           pngio.imread of 16-bit 128 x 128 frames (reported separately: disk + zlib, not the GPU)
  numpy_register_est_s              the numpy fp64-FFT restatement of the reference's registration, timed on 50 sets and EXTRAPOLATED
    python tools/prep_bench.py [--sets-train 1160 --sets-test 290]
--register masked [--register-window 8] [--rounds 5]: instead, the masked registration (probav_prep_register_masked) against the plain one
(probav_prep_register) on the same device-resident frames in the same process, in alternated timed windows (plain, masked, plain, ...),
each between device events after a warm-up of both: one JSON line with every window's time, the medians and masked_over_plain.
--refine [--rounds 5] [--iters 20] [--out profiles/refine_bench.txt]: instead, the mask refinement (probav_prep_refine_masks, default RefineSpec)
on the registered corpus with one planted cloud per set, against a device copy of the bytes its statement moves and against the same masks
composed from torch ops, alternated (refine, copy, torch, refine, ...); the torch-composed result must equal the kernel's bitwise.  One JSON
line with every window's time per call, the medians, refine_over_copy and torch_over_refine; the same line is written to --out.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def corpus(n_sets, rng):
    N = 128
    k = np.fft.fftfreq(N)
    filt = 1.0 / (1e-3 + np.hypot(k[:, None], k[None, :]) ** 1.5)
    sizes = rng.integers(9, 36, n_sets)
    frames, masks = [], []
    for n in sizes:
        t = np.fft.ifft2(np.fft.fft2(rng.standard_normal((N, N))) * filt).real
        t = 1000 + 20000 * (t - t.min()) / (t.max() - t.min())
        for _ in range(n):
            s = tuple(int(v) for v in rng.integers(-3, 4, 2))
            frames.append(np.clip(np.roll(t, s, axis=(0, 1)) + rng.normal(0, 30, (N, N)), 0, 65535).astype(np.uint16))
            masks.append(rng.random((N, N)) < 0.9)
    return np.stack(frames), np.stack(masks), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def masked_ab(opt, L, _lib, torch, n_frames, n_sets, fr, mk, od, rf, spec, sh, of_, om, oc):
    """Plain and masked registration of the SAME resident frames, alternated; both already warm (plain by main(), masked here)."""
    dev = fr.device
    reg = torch.empty(n_frames, dtype=torch.uint8, device=dev)
    st = _lib.current_stream()

    def plain():
        _lib.check(L.probav_prep_register(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(od), n_sets, n_frames, _lib.ptr(rf), _lib.ptr(spec), _lib.ptr(sh),
                                          _lib.ptr(of_), _lib.ptr(om), _lib.ptr(oc), st), "probav_prep_register")

    def masked():
        _lib.check(L.probav_prep_register_masked(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(od), n_sets, n_frames, _lib.ptr(rf), opt.register_window,
                                                 _lib.ptr(sh), _lib.ptr(reg), _lib.ptr(of_), _lib.ptr(om), _lib.ptr(oc), st),
                   "probav_prep_register_masked")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    timed(masked)                                          # warm-up: code object, the kernel's LDS attribute
    unregistered = int((reg == 0).sum())
    t_plain, t_masked = [], []
    for _ in range(opt.rounds):
        t_plain.append(timed(plain))
        t_masked.append(timed(masked))
    mp, mm = float(np.median(t_plain)), float(np.median(t_masked))
    shifts = (2 * opt.register_window + 1) ** 2
    print(json.dumps({"frames": int(n_frames), "sets": int(n_sets), "window": opt.register_window, "rounds": opt.rounds,
                      "plain_ms": [round(t, 2) for t in t_plain], "masked_ms": [round(t, 2) for t in t_masked],
                      "plain_median_ms": round(mp, 2), "masked_median_ms": round(mm, 2), "masked_over_plain": round(mm / mp, 2),
                      "masked_us_per_frame": round(mm * 1e3 / n_frames, 3),
                      "masked_pixel_pairs_per_s": round((n_frames - n_sets) * shifts * 128 * 128 / (mm * 1e-3), 0),
                      "frames_without_candidate": unregistered}))


def torch_refine(torch, fr, mk, groups, spec, out, flagged):
    """The statement of prep.refine_masks_numpy composed from torch ops on the device (sort / where / max_pool2d), one batch per set length:
    groups = [(T, frame indices [G, T] on the device)].  Writes out (uint8 0/1) and flagged (int32 [F, 2]) in place."""
    BIG = 1 << 20
    for T, idx in groups:
        x = fr.view(torch.int16)[idx].to(torch.int32) & 0xFFFF         # [G, T, H, W] (indexing is not there for uint16)
        c = mk[idx] != 0
        sat = c & (x > spec.saturation) if spec.saturation is not None else torch.zeros_like(c)
        cc = c & ~sat
        n = cc.sum(1)
        r = (torch.clamp(n - 1, min=0) // 2).unsqueeze(1)
        pick = lambda v: torch.where(cc, v, BIG).sort(dim=1).values.gather(1, r)
        med = pick(x)
        d = (x - med).abs()
        s = torch.clamp(pick(d), min=spec.floor)
        o = cc & (n >= spec.min_clear).unsqueeze(1) & (16 * d > spec.k16 * s)
        f = (sat | o).to(torch.float32)
        k = 2 * spec.dilate + 1
        g = torch.nn.functional.max_pool2d(f, k, stride=1, padding=spec.dilate) > 0 if spec.dilate else f > 0
        out[idx] = (c & ~g).to(torch.uint8)
        flagged[idx] = torch.stack([sat.sum((2, 3)), o.sum((2, 3))], -1).to(torch.int32)


def refine_abc(opt, F, M, off):
    """--refine: the mask refinement (probav_prep_refine_masks), a device copy that moves the bytes the statement needs (3 read and 1 written
    per pixel and frame: a uint16 copy of the frames, 2 read and 2 written) and the same masks composed from torch ops, on the same resident,
    registered frames in one process, in alternated timed windows between device events after a warm-up of all three.  The torch-composed
    masks, counts and flagged must equal the kernel's bitwise at this size.  One JSON line, also written to --out."""
    import torch
    from probav_amd import _lib, prep
    spec = prep.RefineSpec()
    rng = np.random.default_rng(1)
    _, rf, rm, _ = prep.device_register(F, M, off, off[:-1])
    for i in range(len(off) - 1):                          # an undetected cloud per set: a bright block in one frame, its mask saying clear
        f, y, x = int(rng.integers(off[i], off[i + 1])), int(rng.integers(0, 112)), int(rng.integers(0, 112))
        rf[f, y:y + 16, x:x + 16] = np.minimum(rf[f, y:y + 16, x:x + 16].astype(np.int64) + 3000, 65535).astype(np.uint16)
    dev = torch.device("cuda")
    n_frames, n_sets = len(rf), len(off) - 1
    fr, mk, od = torch.from_numpy(rf).to(dev), torch.from_numpy(rm.view(np.uint8)).to(dev), torch.from_numpy(off).to(dev)
    out_k, out_t, copy_dst = torch.empty_like(mk), torch.empty_like(mk), torch.empty_like(fr)
    flags = torch.empty(n_sets * 3 * 128 * 128, dtype=torch.int64, device=dev)       # pixel_masks: per set and pixel, one bit per frame
    cnt_k, flg_k = torch.empty(n_frames, dtype=torch.int32, device=dev), torch.empty(n_frames, 2, dtype=torch.int32, device=dev)
    flg_t = torch.empty_like(flg_k)
    sizes = np.diff(off)
    groups = [(int(T), torch.from_numpy(np.stack([np.arange(off[i], off[i + 1]) for i in np.nonzero(sizes == T)[0]])).to(dev))
              for T in np.unique(sizes)]
    L, st = _lib.lib(), _lib.current_stream()

    def kernel():
        _lib.check(L.probav_prep_refine_masks(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(od), n_sets, n_frames, 128, 128, int(sizes.max()), spec.k16, spec.floor,
                                              spec.min_clear, spec.dilate, -1 if spec.saturation is None else spec.saturation, _lib.ptr(flags), _lib.ptr(out_k), _lib.ptr(cnt_k), _lib.ptr(flg_k), st),
                   "probav_prep_refine_masks")

    legs = {"refine": (kernel, opt.iters), "copy": (lambda: copy_dst.copy_(fr), opt.iters),
            "torch": (lambda: torch_refine(torch, fr, mk, groups, spec, out_t, flg_t), 1)}

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn, _ in legs.values():                            # warm-up: code objects, the allocator's blocks
        timed(fn, 1)
    bitwise = bool(torch.equal(out_t, out_k) and torch.equal(flg_t, flg_k) and torch.equal(out_k.view(n_frames, -1).sum(1, dtype=torch.int32), cnt_k))
    assert bitwise, "the torch-composed masks differ from the kernel's"
    times = {k: [] for k in legs}
    for _ in range(opt.rounds):
        for k, (fn, iters) in legs.items():
            times[k].append(timed(fn, iters))
    med = {k: float(np.median(v)) for k, v in times.items()}
    px = n_frames * 128 * 128
    res = {"frames": int(n_frames), "sets": int(n_sets), "rounds": opt.rounds, "iters_per_window": opt.iters,
           "spec": {"k": spec.k, "floor": spec.floor, "min_clear": spec.min_clear, "dilate": spec.dilate, "saturation": spec.saturation},
           "refine_ms": [round(t, 3) for t in times["refine"]], "copy_ms": [round(t, 3) for t in times["copy"]],
           "torch_ms": [round(t, 2) for t in times["torch"]],
           "refine_median_ms": round(med["refine"], 3), "copy_median_ms": round(med["copy"], 3), "torch_median_ms": round(med["torch"], 2),
           "refine_over_copy": round(med["refine"] / med["copy"], 2), "torch_over_refine": round(med["torch"] / med["refine"], 1),
           "copy_bytes": 4 * px, "copy_GBps": round(4 * px / (med["copy"] * 1e-3) / 1e9, 1),
           # the statement: 3 read + 1 written per pixel and frame; the kernels: + 24 bytes per pixel and SET written, then read again (less the halo)
           "refine_bytes_statement": 4 * px, "refine_bytes_two_launches": 4 * px + 2 * 24 * n_sets * 128 * 128,
           "refine_compares": int(32 * px), "refine_lds_reads": int(16 * px), "refine_us_per_frame": round(med["refine"] * 1e3 / n_frames, 4),
           "newly_masked": int(mk.sum().item() - cnt_k.sum().item()), "flagged_saturated": int(flg_k[:, 0].sum().item()),
           "flagged_outliers": int(flg_k[:, 1].sum().item()), "torch_composed_equals_kernel_bitwise": bitwise}
    line = json.dumps(res)
    print(line)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            fh.write("tools/prep_bench.py --refine --sets-train %d --sets-test %d --rounds %d --iters %d   (ms per call, device events, alternated windows)\n"
                     % (opt.sets_train, opt.sets_test, opt.rounds, opt.iters))
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refine", action="store_true", help="time the mask refinement against a device copy and the torch-composed statement")
    ap.add_argument("--iters", type=int, default=20, help="--refine: calls per timed window of the kernel and the copy")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refine_bench.txt"),
                    help="--refine: where the result is written as well")
    ap.add_argument("--sets-train", type=int, default=1160)
    ap.add_argument("--sets-test", type=int, default=290)
    ap.add_argument("--register", default="freq", choices=["freq", "masked"])
    ap.add_argument("--register-window", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    opt = ap.parse_args()
    import torch
    from probav_amd import pngio, prep
    rng = np.random.default_rng(0)
    F, M, off = corpus(opt.sets_train + opt.sets_test, rng)
    n_frames = len(F)
    if opt.refine:
        refine_abc(opt, F, M, off)
        return
    prep.device_register(F[:off[2]], M[:off[2]], off[:3], off[:2])          # warm-up (code objects, attributes)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    counts = prep.device_count_nonzero(M, 128 * 128)
    order = np.concatenate([off[i] + np.argsort(-counts[off[i]:off[i + 1]].astype(np.int64)) for i in range(len(off) - 1)])
    prep.device_register(F[order], M[order], off, off[:-1])
    e1.record()
    torch.cuda.synchronize()
    wall2 = time.perf_counter() - t0
    # device-only time of the registration launches (no host copies): the inputs already resident
    import ctypes
    from probav_amd import _lib
    dev = torch.device("cuda")
    fr, mk = torch.from_numpy(F).to(dev), torch.from_numpy(M.view(np.uint8)).to(dev)
    od, rf = torch.from_numpy(off).to(dev), torch.from_numpy(off[:-1].astype(np.int32)).to(dev)
    spec = torch.empty((len(off) - 1) * 128 * 128 * 2, dtype=torch.float32, device=dev)
    sh, of_, om, oc = (torch.empty(n_frames, 2, dtype=torch.int32, device=dev), torch.empty_like(fr), torch.empty_like(mk),
                       torch.empty(n_frames, dtype=torch.int32, device=dev))
    cnt = torch.empty(n_frames, dtype=torch.int32, device=dev)
    L = _lib.lib()
    torch.cuda.synchronize()
    e0.record()
    _lib.check(L.probav_prep_count_nonzero(_lib.ptr(mk), n_frames, 128 * 128, _lib.ptr(cnt), _lib.current_stream()))
    _lib.check(L.probav_prep_register(_lib.ptr(fr), _lib.ptr(mk), _lib.ptr(od), len(off) - 1, n_frames, _lib.ptr(rf), _lib.ptr(spec),
                                      _lib.ptr(sh), _lib.ptr(of_), _lib.ptr(om), _lib.ptr(oc), _lib.current_stream()))
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1)
    if opt.register == "masked":
        masked_ab(opt, L, _lib, torch, n_frames, len(off) - 1, fr, mk, od, rf, spec, sh, of_, om, oc)
        return
    del fr, mk, spec, of_, om
    # stages 3-4 on the train part: 9 frames per set
    S = opt.sets_train
    sel = np.stack([off[i] + np.arange(9) for i in range(S)])
    lr = np.ma.masked_array(F[sel].astype(np.float64)[:, :, None], mask=~M[sel][:, :, None])
    hr = np.ma.masked_array(np.kron(F[off[:S]], np.ones((3, 3), np.uint16))[:, None, None],
                            mask=np.zeros((S, 1, 1, 384, 384), bool))
    t0 = time.perf_counter()
    pl, _ = prep._patches(lr, 22, 16, 3)
    ph, _ = prep._patches(hr, 48, 48, 0)
    pl = prep.pickClearPatchesLR(pl, 9, 0.85)
    pl, ph = prep.pickClearPatches(*prep.removeCorruptedTrainPatchSets(pl, ph, 0.85), 0.85)
    wall34 = time.perf_counter() - t0
    # PNG decode
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(200):
            p = os.path.join(d, "LR%03d.png" % i)
            pngio.imsave_uint16(p, F[i])
            paths.append(p)
        t0 = time.perf_counter()
        for p in paths:
            pngio.imread(p)
        png_ms = (time.perf_counter() - t0) * 1e3 / len(paths)
    # numpy fp64 FFT restatement of the reference's registration (register_translation + fourier_shift), 50 sets, extrapolated
    t0 = time.perf_counter()
    nf = 0
    for s in range(50):
        ref = F[off[s]].astype(np.float64)
        R = np.fft.fft2(ref)
        for f in range(off[s] + 1, off[s + 1]):
            img = F[f].astype(np.float64)
            I = np.fft.fft2(img)
            cc = np.fft.ifft2(R * np.conj(I))
            y, x = np.unravel_index(np.argmax(np.abs(cc)), cc.shape)
            np.fft.ifft2(I * np.exp(-2j * np.pi * (np.fft.fftfreq(128)[:, None] * y + np.fft.fftfreq(128)[None, :] * x))).real
            np.fft.ifft2(np.fft.fft2(M[f].astype(np.float64)))
            nf += 1
    np_s = (time.perf_counter() - t0) * (n_frames / max(1, nf + 50))
    print(json.dumps({"frames": int(n_frames), "sets": int(len(off) - 1), "stage2_device_ms": round(dev_ms, 2),
                      "us_per_frame": round(dev_ms * 1e3 / n_frames, 3), "stage2_wall_s_with_copies": round(wall2, 3),
                      "stage34_wall_s": round(wall34, 3), "png_decode_ms_per_frame": round(png_ms, 3),
                      "numpy_register_est_s": round(np_s, 1), "numpy_register_est_note": "extrapolated from 50 sets"}))


if __name__ == "__main__":
    main()
