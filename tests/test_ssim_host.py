"""cSSIM on the host: the numpy statement (scoring.cssim_table_numpy, the folded form) against the literal direct form of the definition,
its edge cases (one window, planted shift, bias invariance, NaN shifts, too-small images), the CSV / JSON writers with and without the
extra columns, evaluate.py's --metrics, score_images with both device functions replaced by the numpy statements, and the new ops on
CPU and fake tensors (no GPU anywhere)."""
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
from tests.ssim_helpers import direct_table, noise_case, planted_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("S", [17, 24, 48])
@pytest.mark.parametrize("border", [0, 1, 3])
def test_statement_equals_the_direct_form(S, border):
    from probav_amd import scoring
    sr, hr, mask = noise_case(3, S, 16, 10 * S + border)
    got = scoring.cssim_table_numpy(sr, hr, mask, border)
    want = direct_table(sr, hr, mask, border)
    assert got.shape == (3, (2 * border + 1) ** 2) and not np.isnan(want).any()
    assert np.abs(got - want).max() < 1e-12


def test_gauss11_is_the_stated_window():
    from probav_amd import scoring
    g = scoring.gauss11()
    raw = [math.exp(-(j - 5) ** 2 / (2 * 1.5 ** 2)) for j in range(11)]
    assert g.dtype == np.float64 and g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15
    np.testing.assert_allclose(g, np.array(raw) / sum(raw), rtol=1e-15, atol=0)
    assert np.array_equal(g, g[::-1]) or np.abs(g - g[::-1]).max() < 1e-17


def test_one_window_per_shift_at_the_smallest_size():
    """S = 17, b = 3: L = 11, K = 1; the table entry is the SSIM of the single 11 x 11 window, written out here in full."""
    from probav_amd import scoring
    sr, hr, mask = noise_case(1, 17, 16, 5, p_clear=0.7)
    got = scoring.cssim_table_numpy(sr, hr, mask, 3)
    g2 = np.outer(scoring.gauss11(), scoring.gauss11())
    P = sr[0, 3:14, 3:14].astype(np.float64)
    for (u, v) in ((0, 0), (2, 5), (6, 6)):
        H, m = hr[0, u:u + 11, v:v + 11].astype(np.float64), mask[0, u:u + 11, v:v + 11].astype(np.float64)
        bias = (m * (H - P)).sum() / m.sum()
        x, y = m * (P + bias), m * H
        mx, my = (g2 * x).sum(), (g2 * y).sum()
        vx, vy, cxy = (g2 * x * x).sum() - mx * mx, (g2 * y * y).sum() - my * my, (g2 * x * y).sum() - mx * my
        want = (2 * mx * my + scoring.SSIM_C1) * (2 * cxy + scoring.SSIM_C2) / ((mx * mx + my * my + scoring.SSIM_C1) * (vx + vy + scoring.SSIM_C2))
        assert abs(got[0, u * 7 + v] - want) < 1e-12


def test_planted_shift_is_recovered():
    from probav_amd import scoring
    sr, hr, mask = planted_scene(48, 3)
    table = scoring.cssim_table_numpy(sr, hr, mask, 3)
    cssim, shift = scoring.cssim_select_numpy(table, 3)
    assert tuple(shift[0]) == (4, 5) and cssim[0] > 0.99 and cssim[0] == table[0, 4 * 7 + 5]
    rest = np.delete(table[0], 4 * 7 + 5)
    assert cssim[0] - rest.max() > 3e-2


def test_a_constant_added_to_sr_changes_nothing():
    from probav_amd import scoring
    sr, hr, mask = noise_case(2, 24, 14, 8)                  # 14-bit values: + 3000 cannot clip
    a = scoring.cssim_table_numpy(sr, hr, mask, 3)
    b = scoring.cssim_table_numpy((sr + 3000).astype(np.uint16), hr, mask, 3)
    assert np.abs(a - b).max() < 1e-9


def test_nan_shifts_and_all_masked_images():
    from probav_amd import scoring
    S, b = 24, 3
    sr, hr, mask = noise_case(3, S, 16, 2)
    mask[0] = False                                         # nothing clear: every shift NaN
    mask[1] = False
    mask[1, :b, :] = True                                   # clear rows only the shifts u < b reach
    table = scoring.cssim_table_numpy(sr, hr, mask, b)
    cssim, shift = scoring.cssim_select_numpy(table, b)
    assert np.isnan(table[0]).all() and math.isnan(cssim[0]) and tuple(shift[0]) == (-1, -1)
    n = score_oracle.moments(sr, hr, mask, b)[:, :, 0]
    assert np.array_equal(np.isnan(table), n == 0)
    assert (n[1].reshape(7, 7)[:b] > 0).all() and (n[1].reshape(7, 7)[b:] == 0).all()
    assert not math.isnan(cssim[1]) and shift[1, 0] < b and not np.isnan(table[2]).any()
    # a window that sees only masked pixels contributes exactly 1: one clear pixel in a corner, far windows are all-masked
    mask[2] = False
    mask[2, 4, 4] = True
    t = scoring.cssim_table_numpy(sr[2:], hr[2:], mask[2:], 0)
    assert 0.0 < t[0, 0] < 1.0 + 1e-12


def test_too_small_an_image_is_refused():
    from probav_amd import scoring
    z = np.zeros((1, 16, 16), np.uint16)
    with pytest.raises(ValueError, match="11"):
        scoring.cssim_table_numpy(z, z, z, 3)
    assert scoring.cssim_table_numpy(z[:, :11, :11], z[:, :11, :11], np.ones((1, 11, 11), bool), 0).shape == (1, 1)
    with pytest.raises(ValueError, match="11"):
        scoring.shift_cssim(z, z, z, 3, device="cuda")       # refused before anything touches a device


ROWS = [{"id": 594, "band": "NIR", "cpsnr": 41.123456789012345, "u": 2, "v": 3, "bias": -1.5, "n_clear": 140000},
        {"id": 600, "band": "NIR", "cpsnr": math.inf, "u": 0, "v": 0, "bias": 0.0, "n_clear": 9},
        {"id": 7, "band": "RED", "cpsnr": math.nan, "u": -1, "v": -1, "bias": math.nan, "n_clear": 0}]
SSIM = [{"cssim": 0.91234567890123456, "su": 2, "sv": 4, "cssim_at_cpsnr_shift": 0.9},
        {"cssim": 1.0, "su": 0, "sv": 0, "cssim_at_cpsnr_shift": 1.0},
        {"cssim": math.nan, "su": -1, "sv": -1, "cssim_at_cpsnr_shift": math.nan}]
TODAY_CSV = ("id,band,cpsnr,u,v,bias,n_clear,norm,benchmark_cpsnr\r\n"
             "imgset0007,RED,nan,-1,-1,nan,0,43.0,30.0\r\n"
             "imgset0594,NIR,41.123456789012344,2,3,-1.5,140000,45.0,40.0\r\n"
             "imgset0600,NIR,inf,0,0,0.0,9,44.0,50.0\r\n")


def test_writers_without_metrics_are_todays(tmp_path):
    from probav_amd import scoring
    assert scoring.CSV_FIELDS == ("id", "band", "cpsnr", "u", "v", "bias", "n_clear", "norm", "benchmark_cpsnr")
    rows = sorted(ROWS, key=lambda r: r["id"])
    bench = [{"id": 594, "cpsnr": 40.0}, {"id": 600, "cpsnr": 50.0}, {"id": 7, "cpsnr": 30.0}]
    norm = {594: 45.0, 600: 44.0, 7: 43.0}
    p = tmp_path / "scores.csv"
    scoring.write_csv(str(p), rows, norm=norm, bench_rows=bench)
    assert open(p, newline="").read() == TODAY_CSV
    counts = {"scored": 3, "skipped": 0, "missing": 0, "removed": 0}
    s = scoring.summarize(rows, counts, norm=norm, bench_rows=bench)
    assert list(s["overall"]) == ["images", "mean_cpsnr", "nan", "inf", "score"]
    assert list(s["benchmark"]) == ["compared", "wins", "losses", "ties", "mean_delta_cpsnr", "median_delta_cpsnr"]
    assert s == scoring.summarize(rows, counts, norm=norm, bench_rows=bench, metrics=("cpsnr",))
    # rows that carry cSSIM keys change nothing unless cSSIM is asked for
    both = [dict(r, **x) for r, x in zip(ROWS, SSIM)]
    scoring.write_csv(str(p), sorted(both, key=lambda r: r["id"]), norm=norm, bench_rows=bench)
    assert open(p, newline="").read() == TODAY_CSV


def test_writers_with_cssim(tmp_path):
    from probav_amd import scoring
    assert scoring.CSV_FIELDS_SSIM[:len(scoring.CSV_FIELDS)] == scoring.CSV_FIELDS
    assert scoring.CSV_FIELDS_SSIM[len(scoring.CSV_FIELDS):] == ("cssim", "su", "sv", "cssim_at_cpsnr_shift", "benchmark_cssim")
    rows = sorted((dict(r, **x) for r, x in zip(ROWS, SSIM)), key=lambda r: r["id"])
    bench = [dict(r, cpsnr=40.0, cssim=c) for r, c in zip(rows, (0.5, 0.9, 0.95))]        # ids 7, 594, 600
    p = tmp_path / "scores.csv"
    m = ("cpsnr", "cssim")
    scoring.write_csv(str(p), rows, bench_rows=bench, metrics=m)
    got = list(csv.DictReader(open(p)))
    assert tuple(got[0]) == scoring.CSV_FIELDS_SSIM
    assert float(got[1]["cssim"]) == SSIM[0]["cssim"] and (got[1]["su"], got[1]["sv"]) == ("2", "4") and got[1]["cssim_at_cpsnr_shift"] == "0.9"
    assert got[0]["cssim"] == "nan" and got[0]["su"] == "-1" and got[1]["benchmark_cssim"] == "0.9"
    s = scoring.summarize(rows, {"scored": 3, "skipped": 0, "missing": 0, "removed": 0}, bench_rows=bench, metrics=m)
    assert s["overall"]["cssim_nan"] == 1 and s["RED"]["cssim_nan"] == 1 and s["NIR"]["cssim_nan"] == 0
    assert s["overall"]["mean_cssim"] == pytest.approx((SSIM[0]["cssim"] + 1.0) / 2) and s["RED"]["mean_cssim"] is None
    assert s["NIR"]["mean_cssim_at_cpsnr_shift"] == pytest.approx(0.95)
    assert s["benchmark"]["mean_delta_cssim"] == pytest.approx(((SSIM[0]["cssim"] - 0.9) + (1.0 - 0.95)) / 2)
    assert s["benchmark"]["median_delta_cssim"] == pytest.approx(((SSIM[0]["cssim"] - 0.9) + (1.0 - 0.95)) / 2)
    s["probe"] = math.nan
    d = json.loads(scoring.json_line(s))
    assert d["probe"] is None and d["RED"]["mean_cssim"] is None and d["overall"]["cssim_nan"] == 1
    with pytest.raises(ValueError, match="foo"):
        scoring.summarize(rows, {}, metrics=("cpsnr", "foo"))


def _evaluate(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--cfg", os.path.join(ROOT, "cfg", "p16t9c85r12.cfg")] + args,
                          capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_parser_takes_metrics(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    import evaluate
    base = ["--cfg", os.path.join(ROOT, "cfg", "p16t9c85r12.cfg"), "--model"]
    assert evaluate.parser(base).metrics == ("cpsnr",)
    assert evaluate.parser(base + ["--metrics", "cpsnr,cssim"]).metrics == ("cpsnr", "cssim")
    out = _evaluate(["--model", "--metrics", "foo"])
    assert out.returncode == 2 and "foo" in out.stderr and out.stdout == ""
    out = _evaluate(["--help"])
    assert out.returncode == 0 and "--metrics" in out.stdout and "does not affect" in out.stdout


def _fake_shift_cpsnr(sr, hr, mask, border=3, formula="esa", device=None):
    r = score_oracle.shift_cpsnr(sr, hr, mask, border)
    return {"cpsnr": np.array([x["cpsnr"] for x in r]), "shift": np.array([x["shift"] for x in r], np.int32),
            "bias": np.array([x["bias"] for x in r]), "n_clear": np.array([x["n_clear"] for x in r], np.int64)}


def test_score_images_with_cssim_is_aligned_by_id(monkeypatch):
    from probav_amd import scoring
    calls = []

    def fake_shift_cssim(sr, hr, mask, border=3, device=None):
        calls.append(len(sr))
        table = scoring.cssim_table_numpy(sr, hr, mask, border)
        cssim, shift = scoring.cssim_select_numpy(table, border)
        return {"cssim": cssim, "shift": shift, "table": table}

    monkeypatch.setattr(scoring, "shift_cpsnr", _fake_shift_cpsnr)
    monkeypatch.setattr(scoring, "shift_cssim", fake_shift_cssim)
    rng = np.random.default_rng(4)
    S, b = 20, 1
    hr = np.maximum(rng.integers(0, 65536, (4, S, S)), 100).astype(np.uint16)
    clear = rng.random((4, S, S)) < 0.9
    images = {594 + k: (hr[k] - 10 * (k + 1)).astype(np.uint16) for k in (0, 2, 3)}      # 595 removed; each image names its HR row by its bias
    images[1306] = hr[0]                                     # a test id
    rows, counts = scoring.score_images(images, {"NIR": (hr, clear)}, border=b, removed={"NIR": [595]}, metrics=("cpsnr", "cssim"))
    assert [r["id"] for r in rows] == [594, 596, 597] and [r["bias"] for r in rows] == [10.0, 30.0, 40.0] and calls == [3]
    assert counts == {"scored": 3, "skipped": 1, "missing": 0, "removed": 1}
    for r, k in zip(rows, (0, 2, 3)):
        table = scoring.cssim_table_numpy(images[r["id"]][None], hr[k:k + 1], clear[k:k + 1], b)[0]
        assert (r["u"], r["v"]) == (b, b) and (r["su"], r["sv"]) == (b, b)                # a perfect prediction up to its bias
        assert r["cssim"] == table.max() and abs(r["cssim"] - 1.0) < 1e-12
        assert r["cssim_at_cpsnr_shift"] == table[r["u"] * (2 * b + 1) + r["v"]]
    # the default asks for nothing new
    calls.clear()
    rows, _ = scoring.score_images(images, {"NIR": (hr, clear)}, border=b, removed={"NIR": [595]})
    assert calls == [] and set(rows[0]) == {"id", "band", "cpsnr", "u", "v", "bias", "n_clear"}
    with pytest.raises(ValueError, match="foo"):
        scoring.score_images(images, {"NIR": (hr, clear)}, border=b, metrics=("cpsnr", "foo"))


def test_ssim_ops_have_no_cpu_fallback(built_lib):
    from probav_amd import scoring
    sr = torch.zeros(1, 24, 24, dtype=torch.uint16)
    mask = torch.ones(1, 24, 24, dtype=torch.bool)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.probav.esa_shift_ssim_table(sr, sr, mask, 3)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.probav.esa_shift_cssim(sr, sr, mask, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.shift_cssim(sr, sr, mask, 3)


def test_ssim_ops_trace_on_fake_tensors():
    """The fake-tensor rules give the output shapes and dtypes without a device (as tests/test_ops_trace_cpu.py does for the step's ops)."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import probav_amd.ops  # noqa: F401
    with FakeTensorMode():
        sr = torch.empty((5, 48, 48), dtype=torch.uint16, device="cuda")
        mask = torch.empty((5, 48, 48), dtype=torch.bool, device="cuda")
        table = torch.ops.probav.esa_shift_ssim_table(sr, sr, mask, 3)
        cssim, shift = torch.ops.probav.esa_shift_cssim(sr, sr, mask, 1)
    assert tuple(table.shape) == (5, 49) and table.dtype == torch.float64 and table.device.type == "cuda"
    assert tuple(cssim.shape) == (5,) and cssim.dtype == torch.float64 and tuple(shift.shape) == (5, 2) and shift.dtype == torch.int32
    for name, ret in (("esa_shift_ssim_table", "-> Tensor"), ("esa_shift_cssim", "-> (Tensor, Tensor)")):
        schema = str(getattr(torch.ops.probav, name).default._schema)
        assert schema.endswith("(Tensor sr, Tensor hr, Tensor mask, SymInt border) " + ret) and "!" not in schema, schema
