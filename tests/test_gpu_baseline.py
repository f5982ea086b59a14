"""The bicubic-mean baseline kernel (csrc/kernels_baseline.hip) against its numpy statement, bit for bit, k_used included: clamped edges, band
and column-tile seams, the 64-bit accumulator and the clip, ties, all-unclear pixels, independence of the launch and of the frame order; the
torch op's contract; and test.py --method baseline / evaluate.py --baseline / --benchmark-baseline end to end on a synthetic dataset."""
import csv
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import score_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ("esa", "clear")


def _random(sizes, H, W, seed, p_clear=0.8):
    rng = np.random.default_rng(seed)
    F = sum(sizes)
    fr = rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    cl = (rng.random((F, H, W)) < p_clear).astype(np.uint8) * rng.integers(1, 256, (F, H, W)).astype(np.uint8)      # any nonzero value is clear
    return fr, cl, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(frames, clear, set_offsets) of a named case; computed once, shared, never modified."""
    if name == "ragged_5x7":                   # every pixel touches a clamp
        return _random([1, 2, 11], 5, 7, 0)
    if name == "workload_128":                 # the workload's row length, 16 bands of 8 LR rows
        return _random([9, 9], 128, 128, 1)
    if name == "two_column_tiles":             # W over 128: a second column tile with a ragged edge, H no multiple of the band
        return _random([3, 2], 11, 131, 2)
    if name == "wide_accumulator":             # sums past int32, and a pattern whose overshoot is clipped at both ends
        H, W = 10, 12
        y, x = np.mgrid[0:H, 0:W]
        board = lambda b: (((y // b + x // b) % 2) * 65535).astype(np.uint16)[None]
        # 35 frames at 65535 and 35 of a 0 / 65535 checkerboard; then what passes 2^31 for certain: 64 frames at 65535 (64 * 65535 * 729), and
        # 40 frames of a checkerboard of 2 x 2 blocks, where the cubic overshoots both ways (up to 40 * 65535 * 900)
        fr = np.concatenate([np.full((35, H, W), 65535, np.uint16), np.repeat(board(1), 35, 0), np.full((64, H, W), 65535, np.uint16), np.repeat(board(2), 40, 0)])
        cl = np.ones_like(fr, np.uint8)
        cl[35:70, 3:5, 4:9] = np.arange(35, dtype=np.uint8)[:, None, None] % 3 == 0                                # some frames unclear in a patch
        return fr, cl, np.array([0, 35, 70, 134, 174], np.int64)
    if name == "ties":                         # equal clear counts at the maximum, reached with different pixels
        fr, cl, off = _random([4, 5, 1], 9, 10, 3, p_clear=1.0)
        cl[0, 0, :3] = 0
        cl[2, 5, 2:5] = 0                      # set 0: frames 1 and 3 tie at 90, 0 and 2 at 87
        cl[4:9, 1, 1] = 0                      # set 1: all five tie
        cl[9] = 0                              # set 2: one frame, nothing clear
        return fr, cl, off
    if name == "all_unclear_pixels":
        fr, cl, off = _random([6, 3], 13, 9, 4, p_clear=0.5)
        cl[0:6, 2:7, 1:4] = 0                  # a block no frame of set 0 sees, across a band seam (LR rows 7 | 8)
        cl[0:6, 7:9, :] = 0
        cl[6:9] = 0                            # set 1: nothing clear anywhere
        return fr, cl, off
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, mode):
    from probav_amd import baseline
    out, k = baseline.baseline_numpy(*_case(name), mode)
    out.setflags(write=False), k.setflags(write=False)
    return out, k


def _run(fr, cl, off, mode, dev):
    from probav_amd import ops                            # noqa: F401  (registers torch.ops.probav.*)
    f = torch.from_numpy(np.ascontiguousarray(fr).view(np.int16)).to(dev).view(torch.uint16)
    out, k = torch.ops.probav.baseline_upscale_mean(f, torch.from_numpy(np.ascontiguousarray(cl)).to(dev), torch.from_numpy(np.asarray(off, np.int64)).to(dev), mode)
    assert out.dtype == torch.float32 and k.dtype == torch.int32
    return out.cpu().numpy(), k.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["ragged_5x7", "workload_128", "two_column_tiles", "wide_accumulator", "ties", "all_unclear_pixels"])
def test_kernel_equals_the_statement_bit_for_bit(dev, name, mode):
    fr, cl, off = _case(name)
    want, want_k = _want(name, mode)
    got, got_k = _run(fr, cl, off, mode, dev)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [(float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:5]])
    assert got_k.tolist() == want_k.tolist()


def test_the_cases_exercise_what_they_are_named_for():
    """The references themselves: the wide case needs more than int32 and clips at both ends; the tie cases tie."""
    from probav_amd import baseline
    fr, cl, off = _case("wide_accumulator")
    U = baseline.upscale_numpy(fr[134:135])[0]
    assert 64 * 65535 * 729 > 2 ** 31 and U.min() < 0 and 40 * int(U.max()) > 2 ** 31 and U.max() > 729 * 65535
    out, k = _want("wide_accumulator", "esa")
    assert np.all(out[0] == 65535) and np.all(out[2] == 65535) and out[3].min() == 0 and out[3].max() == 65535 and k.tolist() == [35, 12, 64, 40]
    assert np.any((out[3] > 0) & (out[3] < 65535))
    assert _want("ties", "esa")[1].tolist() == [2, 5, 1]
    fr, cl, off = _case("all_unclear_pixels")
    assert ((cl[:6] != 0).sum(0) == 0).any() and ((cl[:6] != 0).sum(0) > 0).any()


@pytest.mark.parametrize("mode", MODES)
def test_one_call_or_one_call_per_set(dev, mode):
    fr, cl, off = _case("ragged_5x7")
    want, want_k = _want("ragged_5x7", mode)
    for s in range(len(off) - 1):
        sl = slice(off[s], off[s + 1])
        got, k = _run(fr[sl], cl[sl], [0, off[s + 1] - off[s]], mode, dev)
        assert np.array_equal(got[0], want[s]) and k.tolist() == [want_k[s]]


@pytest.mark.parametrize("mode", MODES)
def test_frame_order_inside_a_set_does_not_matter(dev, mode):
    fr, cl, off = _case("all_unclear_pixels") if mode == "clear" else _case("ties")
    want, want_k = _want("all_unclear_pixels" if mode == "clear" else "ties", mode)
    order = np.concatenate([np.arange(off[s], off[s + 1])[::-1] for s in range(len(off) - 1)])
    got, k = _run(fr[order], cl[order], off, mode, dev)
    assert np.array_equal(got, want) and k.tolist() == want_k.tolist()


def test_bool_masks_and_the_python_wrapper(dev):
    from probav_amd import baseline
    fr, cl, off = _case("ragged_5x7")
    want, want_k = _want("ragged_5x7", "clear")
    out, k = baseline.baseline_device(fr, cl != 0, off, baseline.BaselineSpec("clear", "raw"))
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), want) and k.cpu().tolist() == want_k.tolist()
    with pytest.raises(ValueError, match="empty"):
        baseline.baseline_device(fr, cl, [0, 1, 1, 14])


def test_broken_sets_are_marked_not_read(dev):
    from probav_amd import ops                            # noqa: F401
    fr, cl, off = _case("ragged_5x7")
    f = torch.from_numpy(fr.view(np.int16)).to(dev).view(torch.uint16)
    c = torch.from_numpy(cl).to(dev)
    _, k = torch.ops.probav.baseline_upscale_mean(f, c, torch.tensor([0, 1, 1, 14], device=dev), "esa")       # set 1 is empty
    k = k.cpu().tolist()
    assert k[0] == 1 and k[1] == -1 and 1 <= k[2] <= 13
    _, k = torch.ops.probav.baseline_upscale_mean(f, c, torch.tensor([0, 1, 3, 15], device=dev), "clear")      # the offsets do not end at n_frames
    assert k.cpu().tolist() == [-1, -1, -1]
    from probav_amd import _lib as L
    out, k2, cnt = torch.empty(3, 15, 21, device=dev), torch.empty(3, dtype=torch.int32, device=dev), torch.empty(14, dtype=torch.int32, device=dev)
    o = torch.tensor([0, 1, 3, 14], device=dev)
    rc = L.lib().probav_baseline_upscale_mean(L.ptr(f), L.ptr(c), L.ptr(o), 3, 14, 5, 7, 4, 0, L.ptr(cnt), L.ptr(out), L.ptr(k2), L.current_stream())
    assert rc == L.PROBAV_EINVAL and b"scale" in L.lib().probav_last_error()
    rc = L.lib().probav_baseline_upscale_mean(L.ptr(f), L.ptr(c), L.ptr(o), 3, 14, 5, 7, 3, 2, L.ptr(cnt), L.ptr(out), L.ptr(k2), L.current_stream())
    assert rc == L.PROBAV_EINVAL and b"mode" in L.lib().probav_last_error()
    torch.cuda.synchronize()


def test_opcheck(dev):
    from probav_amd import ops                            # noqa: F401
    fr, cl, off = _case("ragged_5x7")
    f = torch.from_numpy(fr.view(np.int16)).to(dev).view(torch.uint16)
    c, o = torch.from_numpy(cl).to(dev), torch.from_numpy(off).to(dev)
    for mode in MODES:
        torch.library.opcheck(torch.ops.probav.baseline_upscale_mean.default, (f, c, o, mode))


def test_cpu_tensors_raise(built_lib):
    from probav_amd import baseline, ops              # noqa: F401
    fr, cl, off = _case("ragged_5x7")
    f, c, o = torch.from_numpy(fr.view(np.int16)).view(torch.uint16), torch.from_numpy(cl), torch.from_numpy(off)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.probav.baseline_upscale_mean(f, c, o, "esa")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        baseline.baseline_device(f, c, off)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _cli(args, cwd, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PROBAV_FORCE_DP")}
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (args, out.stdout[-1500:], out.stderr[-3000:])
    return out.stdout


def _objects(items):
    out = np.empty(len(items), dtype=object)
    for i, a in enumerate(items):
        out[i] = a
    return out


def test_clis_end_to_end(dev, tmp_path):
    """numpy dumps in the layout the dataset builder writes, a cfg and removedTrainSetsNIR.txt in the working directory, as tests/test_gpu_cli.py
    builds them; then the three commands."""
    from probav_amd import baseline, scoring, synth
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.parseConfig import parseConfig
    from probav_amd.pngio import imread_uint16
    from probav_amd.trainClass import ModelTrainer
    from tests.test_gpu_cli import CFG
    d = str(tmp_path)
    arr, res, trm = (os.path.join(d, "pre", k) for k in ("arrayDir", "resolverDir", "trimmedArrayDir"))
    for p in (arr, res, trm):
        os.makedirs(p)
    rng = np.random.default_rng(7)
    Y, X = np.mgrid[0:384, 0:384]
    hr = np.stack([np.rint(9000 + 3000 * np.sin(Y / (20.0 + s)) + 2500 * np.cos(X / (15.0 + s)) + 5 * X) for s in range(4)]).astype(np.uint16)
    lr = np.rint(hr.astype(np.float64).reshape(4, 128, 3, 128, 3).mean(axis=(2, 4)))
    sizes = {"TRAIN": [3, 5, 4, 6], "TEST": [2, 4]}
    sets = {}
    for key, ts in sizes.items():
        img, msk = [], []
        for s, T in enumerate(ts):
            f = np.clip(np.repeat(lr[s][None], T, 0) + rng.integers(-300, 301, (T, 128, 128)), 0, 65535).astype(np.uint16)
            q = (rng.random((T, 128, 128)) < 0.9).astype(np.uint8) * 255                                      # QM.png: 255 = clear
            q[0] = 255 if s % 2 else q[0]
            img.append(f[:, None]), msk.append(q[:, None])
        sets[key] = (img, msk)
        _objects(img).dump(os.path.join(arr, "%simgLR_NIR.npy" % key))
        _objects(msk).dump(os.path.join(arr, "%smskLR_NIR.npy" % key))
    hr_clear = rng.random((4, 384, 384)) < 0.95
    hr[:, None, None].dump(os.path.join(arr, "TRAINimgHR_NIR.npy"))
    (hr_clear.astype(np.uint8) * 255)[:, None, None].dump(os.path.join(arr, "TRAINmskHR_NIR.npy"))
    np.ma.masked_array(hr[:, None, None], mask=~hr_clear[:, None, None]).dump(os.path.join(res, "TRAINimgHR_NIR.npy"))
    cfgp = os.path.join(d, "mini.cfg")
    with open(cfgp, "w") as fh:
        fh.write(CFG.format(d=d))
    with open(os.path.join(d, "removedTrainSetsNIR.txt"), "w") as fh:
        fh.write("595.0\n")

    def statement(key, mode):
        img, msk = sets[key]
        off = np.concatenate([[0], np.cumsum([len(a) for a in img])])
        return baseline.baseline_numpy(np.concatenate(img)[:, 0], np.concatenate(msk)[:, 0], off, mode)[0].astype(np.uint16)

    # test.py --method baseline: no checkpoint anywhere; raw frames name every set from the band's first id
    _cli([os.path.join(ROOT, "test.py"), "--cfg", cfgp, "--band", "NIR", "--method", "baseline"], d)
    pngs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "testout_mini", "*.png")))
    assert pngs == ["imgset1306.png", "imgset1307.png"], pngs
    for name, w in zip(pngs, statement("TEST", "esa")):
        np.testing.assert_array_equal(imread_uint16(os.path.join(d, "testout_mini", name)), w)

    # registered frames: trimmedArrayDir holds the sets that were kept, named as test.py names them (595 removed)
    keep = [0, 2, 3]
    reg = np.stack([sets["TRAIN"][0][s][:3] for s in keep]).astype(np.float64)
    reg_clear = np.stack([sets["TRAIN"][1][s][:3] for s in keep]) != 0
    np.ma.masked_array(reg, mask=~reg_clear).dump(os.path.join(trm, "TRAINimgLR_NIR.npy"))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        imgs, ids = baseline.baseline_images(parseConfig(cfgp), "NIR", "TRAIN", baseline.BaselineSpec("clear", "registered"))
    finally:
        os.chdir(cwd)
    assert ids == [594, 596, 597]
    want, _ = baseline.baseline_numpy(reg.reshape(9, 128, 128), reg_clear.reshape(9, 128, 128), [0, 3, 6, 9], "clear")
    np.testing.assert_array_equal(imgs, want.astype(np.uint16))

    # evaluate.py --baseline: the cPSNR of the statement's images under the host scoring oracle
    a = json.loads(_cli([os.path.join(ROOT, "evaluate.py"), "--cfg", cfgp, "--band", "NIR", "--baseline", "--norm", "computed",
                         "--out", os.path.join(d, "o1")], d).strip().splitlines()[-1])
    ref = score_oracle.shift_cpsnr(statement("TRAIN", "esa"), hr, hr_clear, 3)
    rows = list(csv.DictReader(open(os.path.join(d, "o1", "scores.csv"))))
    assert [r["id"] for r in rows] == ["imgset%04d" % i for i in (594, 595, 596, 597)]                       # raw: every set, the removed one too
    for r, w in zip(rows, ref):
        assert abs(float(r["cpsnr"]) - w["cpsnr"]) < 1e-9 and (int(r["u"]), int(r["v"])) == w["shift"]
    assert a["scored"] == 4 and a["baseline"] == {"mode": "esa", "frames": "raw"} and a["norm_source"] == "computed"
    assert a["NIR"]["mean_cpsnr"] == pytest.approx(np.mean([w["cpsnr"] for w in ref]), abs=1e-9) and a["NIR"]["score"] == 1.0

    # evaluate.py --model --benchmark-baseline: a seeded, untrained checkpoint against the baseline
    cfg = parseConfig(cfgp)
    k = cfg["kernel_size"]
    model = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, cfg["max_shift"]).build(
        cfg["scale"], cfg["num_filters"], (k, k, k), cfg["num_res_blocks"], cfg["exp_rate"], cfg["decay_rate"], cfg["num_low_res_imgs"],
        cfg["patch_size"], cfg["is_grayscale"], seed=17)
    ModelTrainer(model, None, None, None, os.path.join(cfg["model_out"], "ckpt_mini", "NIR"), os.path.join(cfg["model_out"], "logs_mini", "NIR")).save()
    patches = synth.synth_batch(3 * 64, seed=6)[0].reshape(3, 64, 22, 22, 9, 1)
    np.ma.masked_array(patches.transpose(0, 1, 4, 5, 2, 3), mask=np.zeros((3, 64, 9, 1, 22, 22), bool)).dump(os.path.join(res, "TRAINpatchesLR_NIR.npy"))
    b = json.loads(_cli([os.path.join(ROOT, "evaluate.py"), "--cfg", cfgp, "--band", "NIR", "--model", "--benchmark-baseline", "--baseline-mode", "clear",
                         "--out", os.path.join(d, "o2")], d, 1200).strip().splitlines()[-1])
    bm = b["benchmark"]
    assert b["scored"] == 3 and bm["compared"] == 3 and bm["wins"] + bm["losses"] + bm["ties"] == 3 and bm["mean_delta_cpsnr"] is not None
    assert b["baseline"] == {"mode": "clear", "frames": "raw"} and b["norm_source"] is None
    ref_c = score_oracle.shift_cpsnr(statement("TRAIN", "clear"), hr, hr_clear, 3)
    rows = {r["id"]: r for r in csv.DictReader(open(os.path.join(d, "o2", "scores.csv")))}
    assert sorted(rows) == ["imgset0594", "imgset0596", "imgset0597"]
    for i in (594, 596, 597):
        assert abs(float(rows["imgset%04d" % i]["benchmark_cpsnr"]) - ref_c[i - 594]["cpsnr"]) < 1e-9
    deltas = [float(r["cpsnr"]) - float(r["benchmark_cpsnr"]) for r in rows.values()]
    assert bm["mean_delta_cpsnr"] == pytest.approx(np.mean(deltas), abs=1e-9)
