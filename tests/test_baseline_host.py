"""The bicubic-mean baseline on the host side (probav_amd/baseline.py): the integer weight table against the Keys cubic in Fractions, the
properties of the upscale (constants, linear ramps, overshoot and clip), the integer rounding of the mean, the two frame-selection modes, PIL's
bicubic away from the edges, a planted cloud scene, and the CLI surface (parser errors, norm_source)."""
import importlib.util
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import score_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "cfg", "p16t9c85r12.cfg")


def _cli(name):
    spec = importlib.util.spec_from_file_location("cli_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _keys(x):
    """The Keys cubic, a = -1/2, written out once more here (Keys 1981, eq. 15)."""
    x = abs(Fraction(x))
    if x <= 1:
        return Fraction(3, 2) * x ** 3 - Fraction(5, 2) * x ** 2 + 1
    if x < 2:
        return Fraction(-1, 2) * x ** 3 + Fraction(5, 2) * x ** 2 - 4 * x + 2
    return Fraction(0)


def test_weight_table_is_the_keys_cubic_in_fractions():
    from probav_amd import baseline
    assert baseline.WEIGHTS27 == ((0, 27, 0, 0), (-2, 21, 9, -1), (-1, 9, 21, -2))
    for ph in range(3):
        t = Fraction(ph, 3)
        want = [_keys(t + 1), _keys(t), _keys(1 - t), _keys(2 - t)]             # taps i0 - 1 .. i0 + 2
        assert [Fraction(w, 27) for w in baseline.WEIGHTS27[ph]] == want
        assert sum(baseline.WEIGHTS27[ph]) == 27
        assert [baseline.keys_cubic(d) for d in (t + 1, t, 1 - t, 2 - t)] == want
    # the phase of HR index Y is (Y - 1) mod 3 about i0 = floor((Y - 1) / 3): half-pixel centres, (Y + 1/2) / 3 - 1/2 = (Y - 1) / 3
    for Y in range(-3, 9):
        c = (Fraction(Y) + Fraction(1, 2)) / 3 - Fraction(1, 2)
        assert c == Fraction(Y - 1, 3) and (Y - 1) // 3 == c.numerator // c.denominator and Fraction((Y - 1) % 3, 3) == c - (Y - 1) // 3


@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (5, 7)])
def test_constant_frame_stays_constant_edges_included(H, W):
    from probav_amd import baseline
    for v in (0, 1, 12345, 65535):
        fr = np.full((3, H, W), v, np.uint16)
        assert np.all(baseline.upscale_numpy(fr) == 729 * v)
        for mode in baseline.MODES:
            out, k = baseline.baseline_numpy(fr, np.ones_like(fr, np.uint8), [0, 3], mode)
            assert out.dtype == np.float32 and out.shape == (1, 3 * H, 3 * W) and np.all(out == v) and k.dtype == np.int32 and k.tolist() == [3]


def test_linear_ramp_is_reproduced_at_interior_pixels():
    from probav_amd import baseline
    H, W = 9, 11
    y, x = np.mgrid[0:H, 0:W]
    U = baseline.upscale_numpy((3 * x + 6 * y).astype(np.uint16)[None])[0]
    Y, X = np.mgrid[0:3 * H, 0:3 * W]
    at_lr = ((Y - 1) % 3 == 0) & ((X - 1) % 3 == 0)                                # (X - 1) / 3 is an integer: the LR sample itself
    inner = (Y >= 6) & (Y < 3 * H - 6) & (X >= 6) & (X < 3 * W - 6)                # no tap is clamped
    want = 729 * ((X - 1) + 2 * (Y - 1))                                           # 3 (X - 1) / 3 + 6 (Y - 1) / 3, over 729
    assert at_lr[inner].sum() > 0 and np.array_equal(U[at_lr & inner], want[at_lr & inner])
    assert np.array_equal(U[at_lr], 729 * (3 * x + 6 * y).reshape(-1))              # ... which holds at the edges too: phase 0 reads one sample
    assert np.array_equal(U[inner], want[inner])                                   # the cubic reproduces a linear function between samples as well


def test_half_to_even_division_on_constructed_pairs():
    from probav_amd import baseline
    pairs = [(5, 2), (7, 2), (-5, 2), (-7, 2), (3, 2), (-3, 2), (1, 2), (-1, 2),    # exact halves to even and odd q, both signs
             (729 * 3, 729 * 2), (729 * 5, 729 * 2), (-729 * 5, 729 * 2),           # D = 729 K with K even: halves exist
             (10, 3), (11, 3), (-10, 3), (-11, 3), (0, 729), (-1, 729), (364, 729), (365, 729), (-364, 729), (-365, 729),
             (35 * 65535 * 1089, 729 * 35), (-(2 ** 38) - 1, 729 * 4096), (2 ** 38 + 729 * 2048, 729 * 4096)]
    N = np.array([p[0] for p in pairs], np.int64)
    D = np.array([p[1] for p in pairs], np.int64)
    got = baseline.round_half_even_div(N, D)
    want = [round(Fraction(n, d)) for n, d in pairs]                               # Python rounds a Fraction half to even, exactly
    assert got.tolist() == want
    assert baseline.round_half_even_div(5, 2) == 2 and baseline.round_half_even_div(7, 2) == 4 and baseline.round_half_even_div(-5, 2) == -2
    assert baseline.round_half_even_div(-7, 2) == -4 and baseline.round_half_even_div(-1, 2) == 0 and baseline.round_half_even_div(-3, 2) == -2
    with pytest.raises(ValueError):
        baseline.round_half_even_div(1, 0)


def test_step_edge_overshoots_both_ways_and_is_clipped():
    from probav_amd import baseline
    fr = np.zeros((1, 6, 8), np.uint16)
    fr[:, :, 4:] = 65535
    U = baseline.upscale_numpy(fr)[0]
    assert U.min() < 0 and U.max() > 729 * 65535                                   # the cubic's negative lobes
    out, _ = baseline.baseline_numpy(fr, np.ones_like(fr, np.uint8), [0, 1])
    assert out.min() == 0 and out.max() == 65535
    assert np.all(out[0][U < 0] == 0) and np.all(out[0][U > 729 * 65535] == 65535)
    # nothing is clipped before the mean: an undershoot of one frame is averaged with another frame's value, not replaced by 0 first
    two = np.concatenate([fr, np.full_like(fr, 30000)])
    out2, _ = baseline.baseline_numpy(two, np.ones_like(two, np.uint8), [0, 2])
    N = U + 729 * 30000
    assert np.array_equal(out2[0], np.clip(baseline.round_half_even_div(N, 729 * 2), 0, 65535).astype(np.float32))
    assert np.any((U < 0) & (out2[0] < 15000))


def test_esa_mode_uses_every_frame_tied_at_the_maximum_and_only_those():
    from probav_amd import baseline
    rng = np.random.default_rng(0)
    H, W = 4, 5
    sizes = [1, 4, 3]
    fr = rng.integers(0, 65536, (sum(sizes), H, W)).astype(np.uint16)
    cl = np.ones_like(fr, np.uint8)
    cl[0] = 0                                  # a one-frame set with nothing clear: still that frame
    cl[1, 0, 0] = 0                            # set 1: frames 2 and 4 tie at the maximum, 1 and 3 are one pixel short
    cl[3, 2, 2] = 0
    cl[5, :, :2] = 0                           # set 2: frame 6 and 7 tie (both with 3 unclear pixels), frame 5 worse
    cl[6, 0, :3] = 0
    cl[7, 3, 2:] = 0
    off = [0, 1, 5, 8]
    out, k = baseline.baseline_numpy(fr, cl, off, "esa")
    assert k.tolist() == [1, 2, 2]
    assert baseline.selected_frames_numpy(cl, off).tolist() == [True, False, True, False, True, False, True, True]
    for s, pick in enumerate(([0], [2, 4], [6, 7])):
        N = baseline.upscale_numpy(fr[pick]).sum(0)
        assert np.array_equal(out[s], np.clip(baseline.round_half_even_div(N, 729 * len(pick)), 0, 65535).astype(np.float32))
    one, k1 = baseline.baseline_numpy(fr[:1], cl[:1], [0, 1], "esa")
    assert k1.tolist() == [1] and np.array_equal(one[0], out[0])


def test_clear_mode_falls_back_to_all_frames_exactly_where_no_frame_is_clear():
    from probav_amd import baseline
    rng = np.random.default_rng(1)
    H, W = 5, 6
    fr = rng.integers(0, 65536, (4, H, W)).astype(np.uint16)
    cl = (rng.random((4, H, W)) < 0.6).astype(np.uint8)
    cl[:, 1, 2] = 0                            # no frame is clear here ...
    cl[:, 4, 5] = 0
    cl[:, 0, 0] = [0, 0, 7, 0]                 # ... and exactly one here (any nonzero value is clear)
    out, k = baseline.baseline_numpy(fr, cl, [0, 4], "clear")
    assert k.tolist() == [4]
    U = baseline.upscale_numpy(fr)
    none = np.repeat(np.repeat((cl != 0).sum(0) == 0, 3, 0), 3, 1)
    assert none[3:6, 6:9].all() and none[12:15, 15:18].all()
    all_frames = np.clip(baseline.round_half_even_div(U.sum(0), 729 * 4), 0, 65535)
    assert np.array_equal(out[0][none], all_frames[none].astype(np.float32))
    for Y in range(3 * H):
        for X in range(3 * W):
            pick = [f for f in range(4) if cl[f, Y // 3, X // 3]] or list(range(4))
            q = round(Fraction(int(sum(U[f, Y, X] for f in pick)), 729 * len(pick)))
            assert out[0, Y, X] == min(max(q, 0), 65535), (Y, X)
    assert np.array_equal(out[0, 0:3, 0:3], np.clip(baseline.round_half_even_div(U[2, 0:3, 0:3], 729), 0, 65535).astype(np.float32))


def test_bad_arguments_raise():
    from probav_amd import baseline
    fr = np.zeros((3, 4, 4), np.uint16)
    cl = np.ones_like(fr, np.uint8)
    with pytest.raises(ValueError, match="scale"):
        baseline.baseline_numpy(fr, cl, [0, 3], "esa", scale=2)
    with pytest.raises(ValueError, match="empty"):
        baseline.baseline_numpy(fr, cl, [0, 1, 1, 3])
    with pytest.raises(ValueError, match="mode"):
        baseline.baseline_numpy(fr, cl, [0, 3], "best")
    with pytest.raises(ValueError):
        baseline.baseline_numpy(fr, cl, [0, 2])
    big = np.zeros((4097, 1, 1), np.uint16)
    with pytest.raises(ValueError, match="4096"):
        baseline.baseline_numpy(big, np.ones_like(big, np.uint8), [0, 4097])
    baseline.baseline_numpy(big[:4096], np.ones((4096, 1, 1), np.uint8), [0, 4096])
    with pytest.raises(ValueError):
        baseline.BaselineSpec("best", "raw")
    with pytest.raises(ValueError):
        baseline.BaselineSpec("esa", "cooked")
    assert baseline.BaselineSpec() == baseline.BaselineSpec("esa", "raw")


def test_pil_bicubic_agrees_away_from_the_edges():
    """PIL's BICUBIC is the same kernel (a = -1/2) at the same centres, but it renormalises the taps at an edge instead of clamping the index, so
    only pixels at least 6 HR pixels from every edge are compared.  PIL resamples a mode-F image in two passes, each accumulated in double and
    stored as float32.  For uint16 data the first pass is at most 65535 * 33 / 27 < 2^17 in magnitude, so its stored value is off by at most half
    an ulp there, 2^-8; the second pass multiplies that by at most sum |w| = 33 / 27 and rounds once more, again by at most 2^-8 (the result is
    below 2^17 too): |PIL - U / 729| <= 2^-8 (33 / 27 + 1) = 0.00868 (the double-precision coefficients add ~1e-11).  Observed maximum on these
    frames: 0.00432."""
    Image = pytest.importorskip("PIL.Image")
    from probav_amd import baseline
    rng = np.random.default_rng(2)
    H, W = 17, 23
    tol = 2.0 ** -8 * (33 / 27 + 1)
    worst = 0.0
    for k in range(4):
        fr = rng.integers(0, 65536, (H, W)).astype(np.uint16)
        got = np.asarray(Image.fromarray(fr.astype(np.float32), mode="F").resize((3 * W, 3 * H), Image.BICUBIC), np.float64)
        want = baseline.upscale_numpy(fr[None])[0] / 729.0
        err = np.abs(got - want)[6:-6, 6:-6]
        worst = max(worst, float(err.max()))
    print("PIL bicubic against U / 729: max abs difference %.6f (bound %.6f)" % (worst, tol))
    assert worst <= tol


def _planted_scene():
    """HR 48 x 48 smooth; 6 LR frames = its 3 x 3 block means; frames 1 and 4 carry a bright square that their masks flag."""
    Y, X = np.mgrid[0:48, 0:48]
    hr = np.rint(20000 + 6000 * np.sin(Y / 9.0) + 5000 * np.cos(X / 7.0) + 40 * X).astype(np.int64)
    lr = np.rint(hr.reshape(16, 3, 16, 3).mean(axis=(1, 3))).astype(np.uint16)
    fr = np.repeat(lr[None], 6, 0).copy()
    cl = np.ones_like(fr, np.uint8)
    for f, (r, c) in ((1, (3, 4)), (4, (8, 6))):
        fr[f, r:r + 5, c:c + 5] += 25000
        cl[f, r:r + 5, c:c + 5] = 0
    return hr.astype(np.uint16), fr, cl


def test_planted_clouds_clear_mode_scores_higher_and_esa_avoids_flagged_frames():
    from probav_amd import baseline
    hr, fr, cl = _planted_scene()
    off = [0, 6]
    masked, _ = baseline.baseline_numpy(fr, cl, off, "clear")
    blind, _ = baseline.baseline_numpy(fr, np.ones_like(cl), off, "clear")
    clear_hr = np.ones((1, 48, 48), bool)
    a = score_oracle.shift_cpsnr(masked.astype(np.uint16), hr[None], clear_hr, 3)[0]["cpsnr"]
    b = score_oracle.shift_cpsnr(blind.astype(np.uint16), hr[None], clear_hr, 3)[0]["cpsnr"]
    print("planted scene: clear mode %.3f dB, the same call with every mask clear %.3f dB" % (a, b))
    assert a > b
    sel = baseline.selected_frames_numpy(cl, off)
    flagged = (cl == 0).reshape(6, -1).any(1)
    assert sel.tolist() == [True, False, True, True, False, True] and not (sel & flagged).any()
    esa, k = baseline.baseline_numpy(fr, cl, off, "esa")
    want = np.clip(baseline.round_half_even_div(baseline.upscale_numpy(fr[[0, 2, 3, 5]]).sum(0), 729 * 4), 0, 65535)
    assert k.tolist() == [4] and np.array_equal(esa[0], want.astype(np.float32))
    # every frame flagged somewhere: the maximum-clearance frames are then the least flagged ones, and only they
    cl2 = cl.copy()
    cl2[[0, 2, 3, 5], 0, 0] = 0
    cl2[0, 0, 1] = 0
    assert baseline.selected_frames_numpy(cl2, off).tolist() == [False, False, True, True, False, True]


@pytest.mark.parametrize("args,msg", [(["--method", "baseline", "--ensemble", "d8"], "--ensemble predicts with the network"),
                                      (["--method", "baseline", "--tile-stride", "8"], "--tile-stride predicts with the network"),
                                      (["--method", "baseline", "--weights", "ema"], "--weights ema predicts with the network"),
                                      (["--baseline-mode", "clear"], "need --method baseline"),
                                      (["--baseline-frames", "registered"], "need --method baseline"),
                                      (["--method", "baseline", "--baseline-mode", "best"], "invalid choice"),
                                      (["--method", "spline"], "invalid choice")])
def test_test_py_parser_errors(args, msg, capsys):
    test = _cli("test")
    with pytest.raises(SystemExit) as e:
        test.parser(["--cfg", CFG] + args)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_test_py_parser_defaults():
    from probav_amd.baseline import BaselineSpec
    test = _cli("test")
    o = test.parser(["--cfg", CFG])
    assert o.method == "network" and o.baseline is None
    o = test.parser(["--cfg", CFG, "--method", "baseline"])
    assert o.baseline == BaselineSpec("esa", "raw")
    o = test.parser(["--cfg", CFG, "--method", "baseline", "--baseline-mode", "clear", "--baseline-frames", "registered"])
    assert o.baseline == BaselineSpec("clear", "registered")


@pytest.mark.parametrize("args,msg", [(["--baseline", "--model"], "exactly one"), (["--baseline", "--toCompare", "."], "exactly one"),
                                      (["--baseline", "--benchmark-baseline"], "--benchmark-baseline applies to --model"),
                                      (["--toCompare", ".", "--benchmark-baseline"], "--benchmark-baseline applies to --model"),
                                      (["--model", "--benchmark-baseline", "--benchmark", "."], "at most one"),
                                      (["--model", "--baseline-mode", "clear"], "need --baseline or --benchmark-baseline"),
                                      (["--baseline", "--ensemble", "d8"], "--ensemble applies to --model"),
                                      (["--baseline", "--tile-stride", "8"], "--tile-stride applies to --model"),
                                      (["--baseline", "--weights", "ema"], "--weights applies to --model"),
                                      (["--baseline", "--norm", "/nonexistent.csv"], "--norm")])
def test_evaluate_py_parser_errors(args, msg, capsys):
    evaluate = _cli("evaluate")
    with pytest.raises(SystemExit) as e:
        evaluate.parser(["--cfg", CFG] + args)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_norm_computed_sets_norm_source(monkeypatch, tmp_path, capsys):
    """evaluate.py --baseline --norm computed, the device replaced by the host oracles: N_i is the esa / raw baseline's own cPSNR, so that
    baseline scores exactly 1; the JSON line names where the norm came from."""
    from probav_amd import baseline, scoring
    from tests.test_score_host import _fake_shift_cpsnr
    evaluate = _cli("evaluate")
    hr, fr, cl = _planted_scene()
    hrs = np.stack([hr, np.roll(hr, 2, 1)])
    monkeypatch.setattr(scoring, "shift_cpsnr", _fake_shift_cpsnr)
    monkeypatch.setattr(scoring, "load_hr", lambda config, band: (hrs, np.ones(hrs.shape, bool)))
    calls = []

    def fake_images(config, band, split, spec):
        calls.append((band, split, spec))
        out, _ = baseline.baseline_numpy(np.concatenate([fr, fr[:3]]), np.concatenate([cl, cl[:3]]), [0, 6, 9], spec.mode)
        return out.astype(np.uint16), [594, 595]

    monkeypatch.setattr(baseline, "baseline_images", fake_images)
    monkeypatch.chdir(tmp_path)
    s = evaluate.main(evaluate.parser(["--cfg", CFG, "--band", "NIR", "--baseline", "--norm", "computed", "--out", str(tmp_path)]))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["norm_source"] == "computed" and line["norm"] == "computed" and line["baseline"] == {"mode": "esa", "frames": "raw"}
    assert s["NIR"]["score"] == 1.0 and s["scored"] == 2
    assert calls == [("NIR", "TRAIN", baseline.BaselineSpec("esa", "raw"))]        # one baseline serves both the images and the norm
    # another baseline against the computed norm; no norm at all; a norm file
    s = evaluate.main(evaluate.parser(["--cfg", CFG, "--band", "NIR", "--baseline", "--baseline-mode", "clear", "--norm", "computed", "--out", str(tmp_path)]))
    assert s["norm_source"] == "computed" and s["baseline"]["mode"] == "clear" and len(calls) == 3 and s["NIR"]["score"] is not None
    s = evaluate.main(evaluate.parser(["--cfg", CFG, "--band", "NIR", "--baseline", "--out", str(tmp_path)]))
    assert s["norm_source"] is None and s["norm"] is None and s["NIR"]["score"] is None
    (tmp_path / "n.csv").write_text("imgset0594 40.0\nimgset0595 41.0\n")
    s = evaluate.main(evaluate.parser(["--cfg", CFG, "--band", "NIR", "--baseline", "--norm", str(tmp_path / "n.csv"), "--out", str(tmp_path)]))
    assert s["norm_source"] == "file" and s["NIR"]["score"] is not None


def test_baseline_has_no_cpu_fallback(built_lib):
    import torch
    from probav_amd import baseline, ops              # noqa: F401
    fr = torch.zeros(2, 4, 4, dtype=torch.uint16)
    cl = torch.ones(2, 4, 4, dtype=torch.uint8)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.probav.baseline_upscale_mean(fr, cl, torch.tensor([0, 2]), "esa")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        baseline.baseline_device(fr, cl, [0, 2])
