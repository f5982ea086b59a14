"""Scoring on the host side: the exact oracle against a literal loop of the ESA formula, norm.csv parsing, the id -> band / HR-row rule,
the CSV / JSON writers, evaluate.py's argument errors, and no CPU fallback in the scoring op."""
import csv
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import score_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _literal(sr, hr, mask, border):
    """The formula as written, one shift and one pixel at a time (Python integers)."""
    S = len(sr)
    L = S - 2 * border
    best = None
    for u in range(2 * border + 1):
        for v in range(2 * border + 1):
            n = s1 = s2 = 0
            for i in range(L):
                for j in range(L):
                    if mask[u + i][v + j]:
                        d = int(hr[u + i][v + j]) - int(sr[border + i][border + j])
                        n, s1, s2 = n + 1, s1 + d, s2 + d * d
            if n == 0:
                continue
            c = Fraction(n * s2 - s1 * s1, n * n)
            if best is None or c < best[0]:
                best = (c, (u, v), Fraction(s1, n), n)
    return best


@pytest.mark.parametrize("S,border,seed", [(9, 0, 0), (10, 1, 1), (12, 3, 2), (13, 2, 3)])
def test_oracle_equals_the_literal_formula(S, border, seed):
    rng = np.random.default_rng(seed)
    sr = rng.integers(0, 65536, (3, S, S)).astype(np.uint16)
    hr = rng.integers(0, 65536, (3, S, S)).astype(np.uint16)
    hr[1] = np.clip(sr[1].astype(np.int64) + rng.integers(-3, 4, (S, S)), 0, 65535)
    mask = rng.random((3, S, S)) < 0.7
    mask[2, :, : S // 2] = False
    got = score_oracle.shift_cpsnr(sr, hr, mask, border)
    for k in range(3):
        c, shift, bias, n = _literal(sr[k].tolist(), hr[k].tolist(), mask[k].tolist(), border)
        assert got[k]["cmse"] == c and got[k]["shift"] == shift and got[k]["n_clear"] == n
        assert got[k]["bias"] == float(bias)
        assert abs(got[k]["cpsnr"] - 10 * math.log10(65535 ** 2 / float(c))) < 1e-9


def test_oracle_edge_cases():
    sr = np.full((3, 8, 8), 100, np.uint16)
    hr = sr.copy()
    mask = np.ones((3, 8, 8), bool)
    mask[1] = False                                          # nothing clear: NaN
    hr[2] += np.arange(8, dtype=np.uint16)[None, :]          # a pure brightness shift per column: no shift is perfect
    r = score_oracle.shift_cpsnr(sr, hr, mask, 1)
    assert r[0]["cpsnr"] == math.inf and r[0]["shift"] == (0, 0)
    assert math.isnan(r[1]["cpsnr"]) and r[1]["shift"] == (-1, -1) and r[1]["n_clear"] == 0
    assert math.isfinite(r[2]["cpsnr"])


def test_read_norm_accepts_whitespace_and_commas(tmp_path):
    from probav_amd import scoring
    p = tmp_path / "norm.csv"
    p.write_text("imgset0000 45.25\nimgset0594,51.5\n\nimgset1159\t 38.125 \nimgset0001 , 40\n")
    assert scoring.read_norm(str(p)) == {0: 45.25, 594: 51.5, 1159: 38.125, 1: 40.0}
    p.write_text("imgset0000 45.25 7\n")
    with pytest.raises(ValueError):
        scoring.read_norm(str(p))


def test_score_is_the_mean_of_norm_over_cpsnr():
    from probav_amd import scoring
    norm = {0: 40.0, 1: 50.0, 2: 30.0, 3: 20.0}
    assert scoring.score({0: 50.0, 1: 40.0}, norm) == pytest.approx((40 / 50 + 50 / 40) / 2)
    assert scoring.score({0: 50.0, 2: math.inf, 3: math.nan}, norm) == pytest.approx((40 / 50 + 0.0) / 2)
    assert scoring.score({0: 50.0}, None) is None and scoring.score({9: 50.0}, norm) is None


def test_ids_map_to_band_and_hr_row():
    from probav_amd import scoring
    assert [scoring.band_of(i) for i in (0, 593, 594, 1159, 1160, 1449)] == ["RED", "RED", "NIR", "NIR", None, None]
    assert [scoring.hr_index(i) for i in (0, 593, 594, 1159)] == [0, 593, 0, 565]
    with pytest.raises(ValueError):
        scoring.hr_index(1160)


def _fake_shift_cpsnr(sr, hr, mask, border=3, formula="esa", device=None):
    r = score_oracle.shift_cpsnr(sr, hr, mask, border)
    return {"cpsnr": np.array([x["cpsnr"] for x in r]), "shift": np.array([x["shift"] for x in r], np.int32),
            "bias": np.array([x["bias"] for x in r]), "n_clear": np.array([x["n_clear"] for x in r], np.int64)}


def test_images_are_aligned_by_id_not_position(monkeypatch):
    """HR rows include removed sets; images of removed sets are absent, test ids and bands not loaded are skipped."""
    from probav_amd import scoring
    monkeypatch.setattr(scoring, "shift_cpsnr", _fake_shift_cpsnr)
    rng = np.random.default_rng(4)
    S = 10
    hr = rng.integers(0, 65536, (4, S, S)).astype(np.uint16)
    clear = rng.random((4, S, S)) < 0.9
    # NIR ids 594..597; 595 removed; each image is its own HR plus a distinct constant, so the bias names the HR row it was scored against
    hr[:] = np.maximum(hr, 100)
    images = {594 + k: (hr[k] - 10 * (k + 1)).astype(np.uint16) for k in (0, 2, 3)}
    images[1306] = hr[0]                                     # a test id
    images[5] = hr[0]                                        # a RED id, RED not loaded
    rows, counts = scoring.score_images(images, {"NIR": (hr, clear)}, border=1, removed={"NIR": [595]})
    assert [r["id"] for r in rows] == [594, 596, 597]
    assert [r["bias"] for r in rows] == [10.0, 30.0, 40.0]
    assert counts == {"scored": 3, "skipped": 2, "missing": 0, "removed": 1}
    del images[597]
    _, counts = scoring.score_images(images, {"NIR": (hr, clear)}, border=1, removed={"NIR": [595]})
    assert counts["missing"] == 1


def test_csv_and_json_writers(tmp_path):
    from probav_amd import scoring
    rows = [{"id": 594, "band": "NIR", "cpsnr": 41.123456789012345, "u": 2, "v": 3, "bias": -1.5, "n_clear": 140000},
            {"id": 600, "band": "NIR", "cpsnr": math.inf, "u": 0, "v": 0, "bias": 0.0, "n_clear": 9},
            {"id": 7, "band": "RED", "cpsnr": math.nan, "u": -1, "v": -1, "bias": math.nan, "n_clear": 0}]
    bench = [{"id": 594, "cpsnr": 40.0}, {"id": 600, "cpsnr": 50.0}, {"id": 7, "cpsnr": 30.0}]
    norm = {594: 45.0, 600: 44.0, 7: 43.0}
    p = tmp_path / "scores.csv"
    scoring.write_csv(str(p), sorted(rows, key=lambda r: r["id"]), norm=norm, bench_rows=bench)
    got = list(csv.DictReader(open(p)))
    assert tuple(got[0]) == scoring.CSV_FIELDS
    assert got[1]["id"] == "imgset0594" and float(got[1]["cpsnr"]) == rows[0]["cpsnr"] and got[1]["u"] == "2" and got[1]["norm"] == "45.0"
    assert got[1]["benchmark_cpsnr"] == "40.0" and got[2]["cpsnr"] == "inf"
    s = scoring.summarize(rows, {"scored": 3, "skipped": 0, "missing": 0, "removed": 0}, norm=norm, bench_rows=bench)
    line = scoring.json_line(s)
    d = json.loads(line)
    assert "\n" not in line and d["scored"] == 3
    assert d["overall"]["nan"] == 1 and d["overall"]["inf"] == 1 and d["overall"]["mean_cpsnr"] == pytest.approx(41.123456789012345)
    assert d["NIR"]["score"] == pytest.approx((45.0 / 41.123456789012345 + 0.0) / 2) and d["RED"]["score"] is None
    b = d["benchmark"]
    assert (b["compared"], b["wins"], b["losses"], b["ties"]) == (2, 2, 0, 0) and b["mean_delta_cpsnr"] == pytest.approx(1.123456789012345)


@pytest.mark.parametrize("args,msg", [([], "exactly one"), (["--model", "--toCompare", "."], "exactly one"),
                                      (["--toCompare", "/nonexistent_dir_x"], "no such folder"), (["--model", "--band", "SWIR"], "--band"),
                                      (["--model", "--formula", "l2"], "invalid choice"), (["--model", "--norm", "/nonexistent.csv"], "--norm")])
def test_evaluate_cli_argument_errors(args, msg):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--cfg", os.path.join(ROOT, "cfg", "p16t9c85r12.cfg")] + args,
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and msg in out.stderr, out.stderr[-1500:]
    assert out.stdout == ""


def test_scoring_op_has_no_cpu_fallback(built_lib):
    from probav_amd import scoring
    sr = torch.zeros(1, 12, 12, dtype=torch.uint16)
    mask = torch.ones(1, 12, 12, dtype=torch.bool)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.probav.esa_shift_cpsnr(sr, sr, mask, 3)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.probav.esa_shift_moments(sr, sr, mask, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.shift_cpsnr(sr, sr, mask, 3)
