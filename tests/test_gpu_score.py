"""The scoring kernels (csrc/kernels_score.hip) against the exact oracle (tests/score_oracle.py): moments bit for bit over sizes, borders,
batch sizes, value ranges and sparse masks; the cPSNR within 1e-9 dB; exact ties; NaN / +inf images; the op under opcheck; the reference
formula; and evaluate.py end to end on a synthetic dataset, three ways (the PNG folder, --model, the oracle on the PNGs)."""
import csv
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import score_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _case(N, S, bits, seed, p_clear=0.85):
    rng = np.random.default_rng(seed)
    top = 1 << bits
    hr = rng.integers(0, top, (N, S, S)).astype(np.uint16)
    sr = np.clip(hr.astype(np.int64) + rng.integers(-top // 8, top // 8, (N, S, S)), 0, 65535).astype(np.uint16)
    sr[::3] = rng.integers(0, top, sr[::3].shape)            # some images uncorrelated: large |d|
    return sr, hr, rng.random((N, S, S)) < p_clear


def _device(*arrs, dev):
    from probav_amd.scoring import _to_device_mask, _to_device_u16
    return [_to_device_u16(a, dev) if a.dtype == np.uint16 else _to_device_mask(a, dev) for a in arrs]


def _check(sr, hr, mask, border, dev):
    from probav_amd import scoring
    s, h, m = _device(sr, hr, mask, dev=dev)
    mom = torch.ops.probav.esa_shift_moments(s, h, m, border).cpu().numpy()
    want = score_oracle.moments(sr, hr, mask, border)
    np.testing.assert_array_equal(mom, want)
    got = scoring.shift_cpsnr(sr, hr, mask, border=border)
    ref = score_oracle.select(want)
    for k, r in enumerate(ref):
        assert tuple(got["shift"][k]) == r["shift"] and got["n_clear"][k] == r["n_clear"], (k, got["shift"][k], r)
        if math.isnan(r["cpsnr"]):
            assert math.isnan(got["cpsnr"][k]) and math.isnan(got["bias"][k])
        else:
            assert got["cpsnr"][k] == r["cpsnr"] if math.isinf(r["cpsnr"]) else abs(got["cpsnr"][k] - r["cpsnr"]) < 1e-9
            assert got["bias"][k] == r["bias"]
    return got, ref


@pytest.mark.parametrize("bits", [14, 16])
def test_moments_bit_equal_at_384(dev, bits):
    _check(*_case(7, 384, bits, bits), 3, dev)


@pytest.mark.parametrize("S", [48, 96, 130])
@pytest.mark.parametrize("border", [0, 1, 3])
def test_moments_bit_equal_any_size_and_border(dev, S, border):
    _check(*_case(7, S, 16, S * 10 + border), border, dev)


@pytest.mark.parametrize("N", [1, 300])
def test_moments_bit_equal_any_batch(dev, N):
    _check(*_case(N, 48, 16, N, p_clear=0.6), 3, dev)


def test_sparse_masks_nan_and_perfect_images(dev):
    S, b = 48, 3
    sr, hr, mask = _case(5, S, 16, 9)
    mask[0] = False
    mask[0, 20, 17] = True                                  # a single clear pixel: only the shifts that see it count, each has cMSE 0
    mask[1] = False
    mask[1, :b, :] = True                                   # clear rows only the shifts u < b reach: the others have n = 0
    mask[2] = False                                         # nothing clear: NaN
    hr[3] = sr[3]                                           # a perfect prediction: +inf at shift (b, b)
    got, ref = _check(sr, hr, mask, b, dev)
    assert ref[0]["cpsnr"] == math.inf and got["n_clear"][0] == 1
    assert math.isnan(got["cpsnr"][2]) and tuple(got["shift"][2]) == (-1, -1) and got["n_clear"][2] == 0
    assert got["cpsnr"][3] == math.inf and tuple(got["shift"][3]) == (b, b)


def test_exact_ties_go_to_the_first_shift(dev):
    """A constant HR under a full mask gives every shift the same cMSE: shift (0, 0) must win; a periodic pattern ties a later pair."""
    S, b = 48, 3
    rng = np.random.default_rng(1)
    sr = rng.integers(0, 65536, (3, S, S)).astype(np.uint16)
    hr = np.full((3, S, S), 1234, np.uint16)
    mask = np.ones((3, S, S), bool)
    col = np.arange(S) % 2
    hr[1] = (1000 + 999 * col)[None, :].repeat(S, 0)        # period 2 in v, the same in every row
    sr[1] = np.roll(hr[1], 1, axis=1)                       # perfect at every even v and every u: (0, 0) first of 28 exact ties
    hr[2] = (np.arange(S) ** 2 * 7)[:, None].repeat(S, 1)
    sr[2] = hr[2] + 5                                       # a pure bias: cMSE 0 at u = b only, at every v (rows are constant): (b, 0)
    got, ref = _check(sr, hr, mask, b, dev)
    assert tuple(got["shift"][0]) == (0, 0)
    assert tuple(got["shift"][1]) == (0, 0) and got["cpsnr"][1] == math.inf
    assert tuple(got["shift"][2]) == (b, 0) and got["cpsnr"][2] == math.inf and got["bias"][2] == -5.0


def test_reference_formula_is_losses_cpsnr(dev):
    from probav_amd import scoring
    from probav_amd.loss import Losses
    sr, hr, mask = _case(4, 384, 16, 21)
    got = scoring.shift_cpsnr(sr, hr, mask, formula="reference")["cpsnr"]
    f = lambda a: torch.as_tensor(a.astype(np.float32))[..., None].to(dev)
    want = Losses(targetShape=(384, 384, 1)).shiftCompensatedcPSNR(f(hr), torch.as_tensor(mask)[..., None].to(dev), f(sr)).double().cpu().numpy()
    np.testing.assert_array_equal(got, want)
    esa = scoring.shift_cpsnr(sr, hr, mask)["cpsnr"]
    assert not np.array_equal(esa, got)                     # HR unmasked vs masked: not the same number


def test_opcheck(dev):
    sr, hr, mask = _case(3, 48, 16, 5)
    s, h, m = _device(sr, hr, mask, dev=dev)
    torch.library.opcheck(torch.ops.probav.esa_shift_cpsnr.default, (s, h, m, 3))
    torch.library.opcheck(torch.ops.probav.esa_shift_moments.default, (s, h, m, 1))


def _run(args, cwd, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PROBAV_FORCE_DP")}
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (args, out.stdout[-1500:], out.stderr[-3000:])
    return out.stdout


def test_evaluate_end_to_end(dev, tmp_path):
    from probav_amd import scoring
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.parseConfig import parseConfig
    from probav_amd.pngio import imread
    from probav_amd.trainClass import ModelTrainer
    from tests.test_gpu_prep import CFG, _write_raw
    d = str(tmp_path)
    _write_raw(d, np.random.default_rng(5))
    cfgp = os.path.join(d, "t.cfg")
    open(cfgp, "w").write(CFG.format(d=d))
    _run([os.path.join(ROOT, "utils", "dataGenerator.py"), "--cfg", cfgp, "--band", "NIR", "--seed", "3"], d, 900)
    cfg = parseConfig(cfgp)
    # a seeded, untrained checkpoint where test.py and evaluate.py --model look for it
    k = cfg["kernel_size"]
    model = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, cfg["max_shift"]).build(
        cfg["scale"], cfg["num_filters"], (k, k, k), cfg["num_res_blocks"], cfg["exp_rate"], cfg["decay_rate"], cfg["num_low_res_imgs"],
        cfg["patch_size"], cfg["is_grayscale"], seed=17)
    ModelTrainer(model, None, None, None, os.path.join(cfg["model_out"], "ckpt_t", "NIR"), os.path.join(cfg["model_out"], "logs_t", "NIR")).save()
    norm = {594: 40.5, 595: 41.0, 596: 42.25, 597: 39.75}
    with open(os.path.join(cfg["raw_data"], "norm.csv"), "w") as fh:
        fh.write("".join("imgset%04d,%r\n" % kv for kv in norm.items()))

    _run([os.path.join(ROOT, "test.py"), "--cfg", cfgp, "--band", "NIR", "--totest", "TRAIN"], d, 1200)
    folder = os.path.join(d, "trainout_t")
    assert sorted(os.listdir(folder)) == ["imgset0594.png", "imgset0596.png", "imgset0597.png"]     # 595 was removed
    open(os.path.join(folder, "imgset1306.png"), "wb").write(open(os.path.join(folder, "imgset0594.png"), "rb").read())   # a test id: skipped

    a = json.loads(_run([os.path.join(ROOT, "evaluate.py"), "--cfg", cfgp, "--band", "NIR", "--toCompare", folder, "--benchmark", folder,
                         "--out", os.path.join(d, "o1")], d, 600).strip().splitlines()[-1])
    b = json.loads(_run([os.path.join(ROOT, "evaluate.py"), "--cfg", cfgp, "--band", "NIR", "--model", "--out", os.path.join(d, "o2")],
                        d, 1200).strip().splitlines()[-1])
    for s in (a, b):
        assert (s["scored"], s["missing"], s["removed"]) == (3, 0, 1) and s["norm"] == os.path.join(cfg["raw_data"], "norm.csv")
        assert set(s["NIR"]) >= {"images", "mean_cpsnr", "score", "nan", "inf"} and s["formula"] == "esa"
    assert a["skipped"] == 1 and b["skipped"] == 0
    assert a["benchmark"]["ties"] == 3 and a["benchmark"]["mean_delta_cpsnr"] == 0.0

    # the oracle on the PNGs
    hr, clear = scoring.load_hr(cfg, "NIR")
    ids = [594, 596, 597]
    sr = np.stack([imread(os.path.join(folder, "imgset%04d.png" % i)) for i in ids])
    ref = score_oracle.shift_cpsnr(sr, hr[[i - 594 for i in ids]], clear[[i - 594 for i in ids]], 3)
    rows = {}
    for tag in ("o1", "o2"):
        rd = list(csv.DictReader(open(os.path.join(d, tag, "scores.csv"))))
        assert tuple(rd[0]) == scoring.CSV_FIELDS
        rows[tag] = {r["id"]: r for r in rd}
    assert sorted(rows["o1"]) == sorted(rows["o2"]) == ["imgset%04d" % i for i in ids]
    for i, r in zip(ids, ref):
        x, y = rows["o1"]["imgset%04d" % i], rows["o2"]["imgset%04d" % i]
        assert x == dict(y, benchmark_cpsnr=x["benchmark_cpsnr"])                        # identical scores, field for field
        assert abs(float(x["cpsnr"]) - r["cpsnr"]) < 1e-9 and (int(x["u"]), int(x["v"])) == r["shift"] and int(x["n_clear"]) == r["n_clear"]
        assert float(x["norm"]) == norm[i]
    want = float(np.mean([norm[i] / float(rows["o1"]["imgset%04d" % i]["cpsnr"]) for i in ids]))
    assert a["NIR"]["score"] == a["overall"]["score"] == b["NIR"]["score"] == pytest.approx(want, rel=1e-15, abs=0)
    assert os.path.exists(os.path.join(d, "o1", "comparison.png")) == (_has_matplotlib())


def _has_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False
