"""What test.py and evaluate.py share (probav_amd/inference.py, probav_amd/intmath.py), the host half: both parsers give the same
InferenceOptions for the same flags and the same error texts for the same bad input, `numbered` names the images as the reference's test.py does,
and the two integer-arithmetic statements hold against exact rationals and INTEGRATION.md's table of non-finite values."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

from probav_amd import inference
from probav_amd.intmath import clip_rint_numpy, round_half_even_div

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = """[Directories]
raw_data=raw
preprocessing_out=pre
model_out=modelInfo
train_out=trainout
test_out=testout

[Net]
num_low_res_imgs=9
scale=3

[Preprocessing]
max_shift=6
patch_size=16
{pre}low_res_patch_thresholds={thr}
"""


def _load(name):
    spec = importlib.util.spec_from_file_location("probav_cli_inf_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def clis():
    return _load("test"), _load("evaluate")


@pytest.fixture()
def cfgs(tmp_path):
    """(a pre19 cfg, one with two patch thresholds, one without num_low_res_imgs_pre)."""
    out = []
    for name, pre, thr in (("pre19.cfg", "num_low_res_imgs_pre=19\n", "0.85"), ("two.cfg", "num_low_res_imgs_pre=19\n", "0.85,0.7"), ("nopre.cfg", "", "0.85")):
        out.append(str(tmp_path / name))
        with open(out[-1], "w") as fh:
            fh.write(CFG.format(pre=pre, thr=thr))
    return out


def _fields(o):
    return (None if o.ensemble is None else (o.ensemble.geometry, o.ensemble.permute, o.ensemble.seed, o.ensemble.V),
            None if o.tiles is None else (o.tiles.stride, o.tiles.window),
            None if o.windows is None else (o.windows.windows, o.windows.step, o.windows.weights, o.windows.threshold),
            o.weights)


ALL = ["--frame-windows", "3", "--frame-window-step", "5", "--tile-stride", "8", "--ensemble", "d8", "--ensemble-permute", "1", "--weights", "ema"]
OPTIONS = [([], (None, None, None, "raw")),
           (["--ensemble", "d8"], (("d8", 0, 0, 8), None, None, "raw")),
           (["--ensemble", "d8", "--ensemble-permute", "2", "--ensemble-seed", "7"], (("d8", 2, 7, 24), None, None, "raw")),
           (["--tile-stride", "8"], (None, (8, "hat"), None, "raw")),
           (["--tile-stride", "4", "--tile-window", "box"], (None, (4, "box"), None, "raw")),
           (["--frame-windows", "3"], (None, None, (3, 1, "clear", None), "raw")),
           (["--frame-windows", "3", "--frame-window-step", "2"], (None, None, (3, 2, "clear", None), "raw")),
           (["--frame-windows", "3", "--frame-window-weights", "uniform"], (None, None, (3, 1, "uniform", None), "raw")),
           (["--weights", "ema"], (None, None, None, "ema")),
           (ALL, (("d8", 1, 0, 16), (8, "hat"), (3, 5, "clear", None), "ema"))]


def test_both_parsers_give_the_same_options(clis, cfgs):
    test_py, evaluate_py = clis
    for args, want in OPTIONS:
        a = test_py.parser(["--cfg", cfgs[0]] + args)
        b = evaluate_py.parser(["--cfg", cfgs[0], "--model"] + args)
        assert isinstance(a.inference, inference.InferenceOptions) and isinstance(b.inference, inference.InferenceOptions)
        assert _fields(a.inference) == _fields(b.inference) == want, args
        for opt in (a, b):                                              # the attributes of the parse result that callers and tests read
            assert opt.windows is opt.inference.windows and opt.weights == opt.inference.weights
            assert (opt.tile_stride, opt.tile_window) == ((0, None) if want[1] is None else want[1])
            assert (opt.frame_windows, opt.frame_window_step, opt.frame_window_weights) == ((0, None, None) if want[2] is None else want[2][:3])
    assert _fields(evaluate_py.parser(["--cfg", cfgs[0], "--toCompare", os.path.dirname(cfgs[0])]).inference) == (None, None, None, "raw")
    assert _fields(inference.InferenceOptions()) == (None, None, None, "raw")


STRIDES = "1 <= s <= 16 and (128 - 16) % s == 0; valid strides: [1, 2, 4, 7, 8, 14, 16]"
# (arguments after --cfg C, the parent commit's error text) for both scripts; {two} / {nopre}: --cfg is that file instead
SHARED_ERRORS = [
    (["--ensemble-permute", "1"], "--ensemble-permute needs --ensemble d8"),
    (["--tile-window", "hat"], "--tile-window needs --tile-stride"),
    (["--tile-stride", "3"], "--tile-stride: tile stride 3 does not tile 128-pixel frames with 16-pixel cores: " + STRIDES),
    (["--tile-stride", "32"], "--tile-stride: tile stride 32 does not tile 128-pixel frames with 16-pixel cores: " + STRIDES),
    (["--tile-stride", "-8"], "--tile-stride: tile stride -8 does not tile 128-pixel frames with 16-pixel cores: " + STRIDES),
    (["--frame-window-step", "2"], "--frame-window-step needs --frame-windows"),
    (["--frame-window-weights", "clear"], "--frame-window-weights needs --frame-windows"),
    (["--frame-windows", "65"], "--frame-windows: frame windows W = 65; 1 <= W <= 64"),
    (["--frame-windows", "-1"], "--frame-windows: frame windows W = -1; 1 <= W <= 64"),
    (["--frame-windows", "3", "--frame-window-step", "0"], "--frame-windows: frame window step = 0; step >= 1"),
    (["--frame-windows", "4", "--frame-window-step", "5"], "--frame-windows: 4 windows at step 5 over num_low_res_imgs = 9 frames need (W - 1) * step + k = 24 frames, "
     "the pool (num_low_res_imgs_pre) has 19: the largest valid W at this step is 3"),
    (["{two}", "--frame-windows", "3"], "--frame-windows: frame windows are defined for one patch threshold; low_res_patch_thresholds has 2 entries: [0.85, 0.7]"),
    (["{nopre}", "--frame-windows", "3"], "--frame-windows: the cfg has no num_low_res_imgs_pre: the pool of registered frames the windows slide over"),
]
TEST_PY_ERRORS = [
    (["--ensemble", "d8", "--reference-loop"], "--reference-loop is the reference's plain loop: it cannot be combined with --ensemble"),
    (["--tile-stride", "8", "--reference-loop"], "--reference-loop is the reference's plain loop: it cannot be combined with --tile-stride"),
    (["--frame-windows", "3", "--reference-loop"], "--reference-loop is the reference's plain loop: it cannot be combined with --frame-windows"),
    (["--ensemble", "d8", "--method", "baseline"], "--ensemble predicts with the network: it cannot be combined with --method baseline"),
    (["--tile-stride", "8", "--method", "baseline"], "--tile-stride predicts with the network: it cannot be combined with --method baseline"),
    (["--weights", "ema", "--method", "baseline"], "--weights ema predicts with the network: it cannot be combined with --method baseline"),
    (["--frame-windows", "3", "--method", "baseline"], "--frame-windows predicts with the network: it cannot be combined with --method baseline"),
    (["{none}", "--tile-stride", "8"], "--tile-stride: cannot read --cfg: [Errno 2] No such file or directory: '{none}'"),
    (["{none}", "--frame-windows", "3"], "--frame-windows: cannot read --cfg: [Errno 2] No such file or directory: '{none}'"),
    (["{none}", "--frame-windows", "3", "--tile-stride", "8"], "--tile-stride: cannot read --cfg: [Errno 2] No such file or directory: '{none}'"),
]
EVALUATE_PY_ERRORS = [            # without --model: a folder of PNGs is scored
    (["--ensemble", "d8"], "--ensemble applies to --model (a folder of PNGs is scored as it is)"),
    (["--weights", "ema"], "--weights applies to --model (a folder of PNGs is scored as it is)"),
    (["--tile-stride", "8"], "--tile-stride applies to --model (a folder of PNGs is scored as it is)"),
    (["--frame-windows", "3"], "--frame-windows applies to --model (a folder of PNGs is scored as it is)"),
    (["--ensemble-permute", "1"], "--ensemble-permute needs --ensemble d8"),
    (["--tile-window", "box"], "--tile-window needs --tile-stride"),
    (["--frame-window-step", "2"], "--frame-window-step needs --frame-windows"),
]


def _error_of(parse, argv, capsys):
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        parse(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err.strip().rsplit(": error: ", 1)[1]


def test_every_error_text_is_the_one_it_was(clis, cfgs, tmp_path, capsys):
    test_py, evaluate_py = clis
    names = {"{two}": cfgs[1], "{nopre}": cfgs[2], "{none}": str(tmp_path / "none.cfg")}

    def argv(args, extra):
        cfg = names.get(args[0])
        return ["--cfg", cfgs[0] if cfg is None else cfg] + extra + (args if cfg is None else args[1:])

    for args, text in SHARED_ERRORS:
        assert _error_of(test_py.parser, argv(args, []), capsys) == text, args
        assert _error_of(evaluate_py.parser, argv(args, ["--model"]), capsys) == text, args
    for args, text in TEST_PY_ERRORS:
        assert _error_of(test_py.parser, argv(args, []), capsys) == text.replace("{none}", names["{none}"]), args
    for args, text in EVALUATE_PY_ERRORS:
        assert _error_of(evaluate_py.parser, argv(args, ["--toCompare", str(tmp_path)]), capsys) == text, args
        assert _error_of(evaluate_py.parser, argv(args, ["--baseline"]), capsys) == text, args


NUMBERED = {("TEST", "NIR"): [1307, 1308, 1311, 1312, 1313, 1314], ("TEST", "RED"): [1161, 1162, 1165, 1166, 1167, 1168],
            ("TRAIN", "NIR"): [595, 596, 599, 600, 601, 602], ("TRAIN", "RED"): [1, 2, 5, 6, 7, 8]}
FIRST = {("TEST", "NIR"): 1306, ("TEST", "RED"): 1160, ("TRAIN", "NIR"): 594, ("TRAIN", "RED"): 0}


def test_numbered_skips_the_removed_ids(tmp_path):
    assert inference.FIRST_ID == FIRST
    from probav_amd import baseline, scoring
    assert baseline.FIRST_ID is inference.FIRST_ID and scoring.FIRST_TRAIN_ID == {"RED": 0, "NIR": 594} and scoring.FIRST_TEST_ID == 1160
    for (split, band), want in NUMBERED.items():
        first = FIRST[(split, band)]
        assert list(inference.numbered(range(6), split, band, str(tmp_path))) == [(first + j, j) for j in range(6)]      # no file: consecutive
        with open(str(tmp_path / ("removedTrainSets%s.txt" % band)), "w") as fh:    # the first id, two neighbours in the middle, one beyond the end
            fh.write("%d\n%d.0\n%d\n%d\n" % (first, first + 3, first + 4, first + 100))
        for b in (band, band.lower()):
            assert list(inference.numbered(range(6), split, b, str(tmp_path))) == list(zip(want, range(6)))
        os.remove(str(tmp_path / ("removedTrainSets%s.txt" % band)))
    assert [i for i, _ in inference.numbered("abc", "anything else", "red", str(tmp_path))] == [0, 1, 2]       # test.py's rule: not TEST is TRAIN


def test_round_half_even_div_against_exact_rationals():
    cases = [(N, D) for N in range(-50, 51) for D in range(1, 8)] + [(s * (2 ** 62 // 3), 2 ** 31 - 1) for s in (1, -1)]
    N, D = np.array([c[0] for c in cases], np.int64), np.array([c[1] for c in cases], np.int64)
    got = round_half_even_div(N, D)
    assert got.dtype == np.int64
    assert got.tolist() == [round(Fraction(n, d)) for n, d in cases]            # Python rounds a Fraction half to even
    assert int(round_half_even_div(5, 2)) == 2 and int(round_half_even_div(-7, 2)) == -4
    for bad in (0, np.array([3, 0, 2])):
        with pytest.raises(ValueError):
            round_half_even_div(np.array([1, 2, 3]), bad)
    from probav_amd import baseline
    assert baseline.round_half_even_div is round_half_even_div


def test_clip_rint_is_the_devices_clip_round():
    x = np.array([np.nan, np.inf, -np.inf, 0.5, -0.5, 1.5, 2.5, 65535.5, 65536.5], np.float32)
    got = clip_rint_numpy(x, 0.0, float(2 ** 16))                               # INTEGRATION.md, 'Non-finite values': NaN -> lo, +inf -> hi, -inf -> lo
    assert got.dtype == np.float32 and got.tolist() == [0.0, 65536.0, 0.0, 0.0, 0.0, 2.0, 2.0, 65536.0, 65536.0]
    got = clip_rint_numpy(x, -2.0, 4000.0)
    assert got.tolist() == [-2.0, 4000.0, -2.0, 0.0, -0.0, 2.0, 2.0, 4000.0, 4000.0] and np.signbit(got[4])
    assert clip_rint_numpy(np.float32(-1.5), -2.0, 0.0) == -2.0 and clip_rint_numpy(np.float32(-2.5), -3.0, 0.0) == -2.0
