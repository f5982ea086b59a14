"""The cSSIM kernels (csrc/kernels_ssim.hip) against the fp64 numpy statement (scoring.cssim_table_numpy): every table entry within 1e-9
absolute with the same NaN pattern, over one window, sizes that are no multiple of the 64 x 64 tile, row-band and column-tile seams; the
selected shift exactly (ties included); perfect predictions; bits that do not depend on the batch; the cPSNR path unchanged; the ops
under opcheck; evaluate.py --metrics cpsnr,cssim end to end.

The bar.  Moments reach 4.3e9; fp64 roundoff over ~25 operations puts about 1e-5 absolute on a variance or a squared mean, and these are
divided by at least C2 = 3.9e6 or C1 = 4.3e5: a worst-case error near 1e-10 per window.  The bar is ten times that bound."""
import csv
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import score_oracle
from tests.ssim_helpers import noise_case, planted_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TOL = 1e-9


def mixed_case(N, S, seed, border=3, p_clear=0.85):
    """N images: 16-bit noise (a third uncorrelated) with the smooth planted-shift scene as the last one."""
    sr, hr, mask = noise_case(N, S, 16, seed, p_clear)
    d = min(1, border)
    s1, h1, m1 = planted_scene(S, seed + 1, dy=d, dx=min(2, border), p_clear=p_clear)
    sr[-1], hr[-1], mask[-1] = s1[0], h1[0], m1[0]
    return sr, hr, mask


def _table(sr, hr, mask, border, dev):
    from probav_amd.scoring import _to_device_mask, _to_device_u16
    t = torch.ops.probav.esa_shift_ssim_table(_to_device_u16(sr, dev), _to_device_u16(hr, dev), _to_device_mask(mask, dev), border)
    return t.cpu().numpy()


def _check(sr, hr, mask, border, dev, gap=True):
    """Table against the statement; then the selection: where the statement's best and second-best differ by more than 1e-6 the device's
    shift must be the statement's, exactly."""
    from probav_amd import scoring
    want = scoring.cssim_table_numpy(sr, hr, mask, border)
    got = scoring.shift_cssim(sr, hr, mask, border=border)
    assert got["table"].shape == want.shape and got["table"].dtype == np.float64
    assert np.array_equal(np.isnan(got["table"]), np.isnan(want))
    ok = ~np.isnan(want)
    err = float(np.abs(got["table"][ok] - want[ok]).max()) if ok.any() else 0.0
    print("S=%d b=%d N=%d: largest |device - numpy| = %.3e" % (sr.shape[1], border, len(sr), err))
    assert err < TOL
    cs, sh = scoring.cssim_select_numpy(want, border)
    for k in range(len(sr)):
        if math.isnan(cs[k]):
            assert math.isnan(got["cssim"][k]) and tuple(got["shift"][k]) == (-1, -1)
            continue
        row = np.sort(want[k][~np.isnan(want[k])])[::-1]
        if gap and len(row) > 1:
            assert row[0] - row[1] > 1e-6, (k, row[:2])
        if len(row) == 1 or row[0] - row[1] > 1e-6:
            assert tuple(got["shift"][k]) == tuple(sh[k]), (k, got["shift"][k], sh[k])
        assert abs(got["cssim"][k] - cs[k]) < TOL
        assert got["cssim"][k] == got["table"][k, got["shift"][k, 0] * (2 * border + 1) + got["shift"][k, 1]]
    return got, want


def test_one_window(dev):
    _check(*mixed_case(3, 17, 1), 3, dev)


@pytest.mark.parametrize("S", [48, 96, 130])
@pytest.mark.parametrize("border", [0, 1, 3])
def test_table_any_size_and_border(dev, S, border):
    _check(*mixed_case(7, S, S * 10 + border, border), border, dev)


def test_row_band_seams_at_384(dev):
    _check(*mixed_case(2, 384, 384), 3, dev)


def test_column_tiles_at_600(dev):
    _check(*mixed_case(1, 600, 600), 3, dev)


def test_nan_shifts_and_sparse_masks(dev):
    S, b = 48, 3
    sr, hr, mask = noise_case(4, S, 16, 9)
    mask[0] = False
    mask[0, 20, 17] = True                                  # a single clear pixel
    mask[1] = False
    mask[1, :b, :] = True                                   # clear rows only the shifts u < b reach: the others are NaN
    mask[2] = False                                         # nothing clear: NaN, (-1, -1)
    got, want = _check(sr, hr, mask, b, dev, gap=False)
    assert np.isnan(got["table"][2]).all() and math.isnan(got["cssim"][2]) and tuple(got["shift"][2]) == (-1, -1)
    assert np.isnan(got["table"][1].reshape(7, 7)[b:]).all() and not np.isnan(got["table"][1].reshape(7, 7)[:b]).any()


def test_ties_go_to_the_first_shift(dev):
    """A constant HR under a full mask: every shift sees the same crops, so the 49 entries must be the same bits and (0, 0) wins."""
    S, b = 48, 3
    rng = np.random.default_rng(1)
    sr = rng.integers(0, 65536, (2, S, S)).astype(np.uint16)
    hr = np.full((2, S, S), 1234, np.uint16)
    hr[1] = 40000
    mask = np.ones((2, S, S), bool)
    got, _ = _check(sr, hr, mask, b, dev, gap=False)
    for k in range(2):
        assert len(set(got["table"][k].view(np.int64).tolist())) == 1
        assert tuple(got["shift"][k]) == (0, 0)


@pytest.mark.parametrize("p_clear", [1.0, 0.3])
def test_perfect_prediction(dev, p_clear):
    from probav_amd import scoring
    S, b = 48, 3
    rng = np.random.default_rng(7)
    hr = rng.integers(0, 65536, (2, S, S)).astype(np.uint16)
    mask = rng.random((2, S, S)) < p_clear
    got = scoring.shift_cssim(hr.copy(), hr, mask, border=b)
    for k in range(2):
        assert tuple(got["shift"][k]) == (b, b) and abs(got["cssim"][k] - 1.0) < 1e-12


def test_bits_do_not_depend_on_the_batch(dev):
    from probav_amd import scoring
    S, b = 48, 3
    sr, hr, mask = noise_case(300, S, 16, 300, p_clear=0.6)
    big = _table(sr, hr, mask, b, dev)
    again = _table(sr, hr, mask, b, dev)
    assert np.array_equal(big.view(np.int64), again.view(np.int64))
    first7 = _table(sr[:7], hr[:7], mask[:7], b, dev)
    assert np.array_equal(first7.view(np.int64), big[:7].view(np.int64))
    for k in (0, 299):
        alone = _table(sr[k:k + 1], hr[k:k + 1], mask[k:k + 1], b, dev)
        assert np.array_equal(alone.view(np.int64), big[k:k + 1].view(np.int64)), k
    want = scoring.cssim_table_numpy(sr[:7], hr[:7], mask[:7], b)
    assert np.abs(big[:7] - want).max() < TOL


def test_cpsnr_path_is_unchanged(dev):
    from probav_amd import scoring
    sr, hr, mask = mixed_case(7, 96, 42)
    got = scoring.shift_cpsnr(sr, hr, mask, border=3)
    scoring.shift_cssim(sr, hr, mask, border=3)
    again = scoring.shift_cpsnr(sr, hr, mask, border=3)
    for k, r in enumerate(score_oracle.shift_cpsnr(sr, hr, mask, 3)):
        assert tuple(got["shift"][k]) == r["shift"] and got["n_clear"][k] == r["n_clear"] and got["bias"][k] == r["bias"]
        assert abs(got["cpsnr"][k] - r["cpsnr"]) < 1e-9
    for key in got:
        assert np.array_equal(got[key], again[key])


def test_ops_refuse_what_they_cannot_take(dev):
    z = torch.zeros((1, 16, 16), dtype=torch.uint16, device=dev)
    with pytest.raises(ValueError, match="11"):
        torch.ops.probav.esa_shift_ssim_table(z, z, z.bool(), 3)
    with pytest.raises(ValueError, match="border"):
        torch.ops.probav.esa_shift_cssim(z, z, z.bool(), 4)
    assert tuple(torch.ops.probav.esa_shift_ssim_table(z[:0], z[:0], z[:0].bool(), 1).shape) == (0, 9)


def test_opcheck(dev):
    from probav_amd.scoring import _to_device_mask, _to_device_u16
    sr, hr, mask = noise_case(3, 48, 16, 5)
    s, h, m = _to_device_u16(sr, dev), _to_device_u16(hr, dev), _to_device_mask(mask, dev)
    torch.library.opcheck(torch.ops.probav.esa_shift_ssim_table.default, (s, h, m, 3))
    torch.library.opcheck(torch.ops.probav.esa_shift_cssim.default, (s, h, m, 1))


def test_evaluate_end_to_end_with_cssim(dev, tmp_path):
    from probav_amd import scoring
    from probav_amd.modelsTF import WDSRConv3D
    from probav_amd.parseConfig import parseConfig
    from probav_amd.pngio import imread
    from probav_amd.trainClass import ModelTrainer
    from tests.test_gpu_prep import CFG, _write_raw
    from tests.test_gpu_score import _run
    d = str(tmp_path)
    _write_raw(d, np.random.default_rng(5))
    cfgp = os.path.join(d, "t.cfg")
    open(cfgp, "w").write(CFG.format(d=d))
    _run([os.path.join(ROOT, "utils", "dataGenerator.py"), "--cfg", cfgp, "--band", "NIR", "--seed", "3"], d, 900)
    cfg = parseConfig(cfgp)
    k = cfg["kernel_size"]
    model = WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, cfg["max_shift"]).build(
        cfg["scale"], cfg["num_filters"], (k, k, k), cfg["num_res_blocks"], cfg["exp_rate"], cfg["decay_rate"], cfg["num_low_res_imgs"],
        cfg["patch_size"], cfg["is_grayscale"], seed=17)
    ModelTrainer(model, None, None, None, os.path.join(cfg["model_out"], "ckpt_t", "NIR"), os.path.join(cfg["model_out"], "logs_t", "NIR")).save()
    _run([os.path.join(ROOT, "test.py"), "--cfg", cfgp, "--band", "NIR", "--totest", "TRAIN"], d, 1200)
    folder = os.path.join(d, "trainout_t")
    ids = [594, 596, 597]                                   # 595 was removed
    assert sorted(os.listdir(folder)) == ["imgset%04d.png" % i for i in ids]

    ev = [os.path.join(ROOT, "evaluate.py"), "--cfg", cfgp, "--band", "NIR"]
    a = json.loads(_run(ev + ["--toCompare", folder, "--benchmark", folder, "--metrics", "cpsnr,cssim", "--out", os.path.join(d, "o1")],
                        d, 600).strip().splitlines()[-1])
    b = json.loads(_run(ev + ["--model", "--metrics", "cpsnr,cssim", "--out", os.path.join(d, "o2")], d, 1200).strip().splitlines()[-1])
    c = json.loads(_run(ev + ["--toCompare", folder, "--out", os.path.join(d, "o3")], d, 600).strip().splitlines()[-1])
    assert "metrics" not in c and "mean_cssim" not in c["NIR"]
    assert tuple(next(csv.reader(open(os.path.join(d, "o3", "scores.csv"))))) == scoring.CSV_FIELDS

    hr, clear = scoring.load_hr(cfg, "NIR")
    sr = np.stack([imread(os.path.join(folder, "imgset%04d.png" % i)) for i in ids])
    idx = [i - 594 for i in ids]
    table = scoring.cssim_table_numpy(sr, hr[idx], clear[idx], 3)
    cs, sh = scoring.cssim_select_numpy(table, 3)
    rows = {}
    for tag in ("o1", "o2"):
        rd = list(csv.DictReader(open(os.path.join(d, tag, "scores.csv"))))
        assert tuple(rd[0]) == scoring.CSV_FIELDS_SSIM
        rows[tag] = {r["id"]: r for r in rd}
    old = {r["id"]: r for r in csv.DictReader(open(os.path.join(d, "o3", "scores.csv")))}
    for k, i in enumerate(ids):
        x, y = rows["o1"]["imgset%04d" % i], rows["o2"]["imgset%04d" % i]
        assert x == dict(y, benchmark_cpsnr=x["benchmark_cpsnr"], benchmark_cssim=x["benchmark_cssim"])      # identical scores, field for field
        assert abs(float(x["cssim"]) - cs[k]) < TOL and (int(x["su"]), int(x["sv"])) == tuple(sh[k])
        assert abs(float(x["cssim_at_cpsnr_shift"]) - table[k, int(x["u"]) * 7 + int(x["v"])]) < TOL
        assert x["benchmark_cssim"] == x["cssim"]
        assert {f: x[f] for f in scoring.CSV_FIELDS if f != "benchmark_cpsnr"} == {f: old["imgset%04d" % i][f] for f in scoring.CSV_FIELDS if f != "benchmark_cpsnr"}
    for s in (a, b):
        assert s["metrics"] == ["cpsnr", "cssim"] and s["NIR"]["cssim_nan"] == 0
        assert s["NIR"]["mean_cssim"] == pytest.approx(float(np.mean(cs)), abs=TOL)
    assert a["benchmark"]["mean_delta_cssim"] == 0.0 and a["benchmark"]["median_delta_cssim"] == 0.0
