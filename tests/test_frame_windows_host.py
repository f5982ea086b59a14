"""Frame-window ensemble, the host half (probav_amd/frame_windows.py): the eligibility limit against the builder's fp64 expression, the frame
choice against the dataset builder's own selection, the integer mean, the spec, the CLI flags and the ops' schemas on fake tensors.
Every comparison is an equality: the feature has no tolerances."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from probav_amd import frame_windows as fw, tiles
from probav_amd.frame_windows import FrameWindowSpec, frame_windows_gather_numpy, frame_windows_reduce_numpy, frame_windows_select_numpy, max_masked

from tests.frame_windows_helpers import LIMIT_22, THRESHOLD, WCONFIG, distinct_frames, eligible, synthetic_counts, unfolded_cloudy
from tests.tiles_helpers import HI, numpy_unfold, synthetic_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the limit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [484, 1024, 1936])
@pytest.mark.parametrize("threshold", [0.85, 0.7, 0.0, 1.0])
def test_max_masked_is_the_builders_fp64_test(pixels, threshold):
    L = max_masked(pixels, threshold)
    for c in range(pixels + 1):
        assert (c < L) == bool(c / pixels < (1 - threshold)), (c, L)
    assert 0 <= L <= pixels + 1
    if threshold == 1.0:
        assert L == 0
    if threshold == 0.0:
        assert L == pixels                                           # every frame but a fully masked one


def test_limit_of_the_shipped_geometry():
    assert LIMIT_22 == max_masked(484, THRESHOLD) == 73              # 72 / 484 < 0.15 <= 73 / 484


# ---- the frame choice ---------------------------------------------------------------------------------------------------------------
def _builder_choice(counts, pixels, k, threshold):
    return tiles.select_frames(np.asarray(counts)[None], pixels, k, [threshold])[0]


CASES = [(9, 22, 9, 1, 1), (13, 22, 9, 5, 1), (19, 22, 9, 3, 5), (12, 22, 7, 6, 1), (64, 22, 9, 56, 1), (2, 22, 9, 1, 1), (10, 5, 3, 8, 1)]


@pytest.mark.parametrize("T_pre,win,k,W,step", CASES, ids=["T%dw%dk%dW%ds%d" % c for c in CASES])
def test_select_on_the_synthetic_rows(T_pre, win, k, W, step):
    pixels = win * win
    L = max_masked(pixels, THRESHOLD)
    names, counts = synthetic_counts(T_pre, pixels, k, L)
    for want in ("zero", "full", "E=0", "E=1", "E=T_pre", "edge"):
        assert want in names
    sel, weight = frame_windows_select_numpy(counts, pixels, k, L, W, step)
    assert sel.shape == (len(counts), W, k) and sel.dtype == np.int32 and weight.shape == (len(counts), W) and weight.dtype == np.int32
    assert sel.min() >= 0 and sel.max() < T_pre
    rows = np.arange(len(counts))[:, None]
    choice = _builder_choice(counts, pixels, k, THRESHOLD)
    np.testing.assert_array_equal(counts[rows, sel[:, 0]], counts[rows, choice])      # the same count sequence whatever the tie order
    E = eligible(counts, L)
    for n in range(len(counts)):
        c = counts[n].astype(np.int64)
        elig = c < L if (c < L).any() else np.ones(T_pre, bool)
        assert elig[sel[n]].all()                                    # only eligible frames
        m = -(-k // E[n])
        # window j is Q shifted by j step, Q the eligible frames by (count, index), each m times
        order = sorted(np.nonzero(elig)[0], key=lambda t: (c[t], t))
        Q = [t for t in order for _ in range(m)]
        for j in range(W):
            assert sel[n, j].tolist() == [Q[(j * step + i) % len(Q)] for i in range(k)], (n, j)
        if len(set(c[elig].tolist())) == E[n]:                       # pairwise distinct eligible counts: the builder's frames themselves
            np.testing.assert_array_equal(sel[n, 0], choice[n])
        raw = (pixels - c[sel[n]]).sum(-1)
        np.testing.assert_array_equal(weight[n], raw if raw.any() else np.ones(W, np.int64))
    if "distinct" in names:
        np.testing.assert_array_equal(sel[names["distinct"], 0], choice[names["distinct"]])
    assert (weight[names["full"]] == 1).all()                        # no clear pixel in any frame: all weights 0 -> all 1
    assert (weight[names["zero"]] == k * pixels).all()
    usel, uw = frame_windows_select_numpy(counts, pixels, k, L, W, step, weights="uniform")
    np.testing.assert_array_equal(usel, sel)
    assert (uw == 1).all()


def test_select_on_the_cloudy_frames_reaches_every_branch():
    _, patches, counts = unfolded_cloudy(13)
    assert patches.shape == (32, 13, 22, 22) and counts.shape == (32, 13)
    k, W, L = 9, 5, LIMIT_22
    sel, weight = frame_windows_select_numpy(counts, 484, k, L, W, 1)
    rows = np.arange(32)[:, None]
    choice = _builder_choice(counts, 484, k, THRESHOLD)
    np.testing.assert_array_equal(counts[rows, sel[:, 0]], counts[rows, choice])
    none = ((counts < L).sum(-1) == 0).sum()
    raw = (484 - counts.astype(np.int64)[rows[:, :, None], sel]).sum(-1)
    zero = (raw == 0).all(-1).sum()
    E = eligible(counts, L)
    wraps = ((W - 1) + k > E * -(-k // E)).sum()
    assert (none, zero, wraps) == (18, 8, 6), (none, zero, wraps)
    assert none > 0 and zero > 0 and wraps > 0 and none < 32         # a changed helper must not silently stop covering the branches
    assert (weight[(raw == 0).all(-1)] == 1).all() and (weight > 0).all()
    # no tile of this input has pairwise distinct eligible counts (clear frames tie at 0): the frames themselves are compared on the
    # synthetic rows above and on distinct_frames below
    assert not [n for n in range(32) if (counts[n] < L).sum() > 1 and len(set(counts[n][counts[n] < L].tolist())) == (counts[n] < L).sum()]


def test_distinct_frames_have_distinct_counts_in_every_tile():
    frames = distinct_frames()
    data, mask = np.ma.getdata(frames).reshape(2, 9, 64, 64), np.ma.getmaskarray(frames).reshape(2, 9, 64, 64)
    for stride in (16, 8):
        counts = numpy_unfold(data, mask, 3, 22, stride)[2].reshape(-1, 9)
        assert (counts < LIMIT_22).all() and all(len(set(row.tolist())) == 9 for row in counts)
        assert len({tuple(np.argsort(row)) for row in counts}) == 2          # another frame order per image
        sel, _ = frame_windows_select_numpy(counts, 484, 9, LIMIT_22, 1, 1)
        np.testing.assert_array_equal(sel[:, 0], _builder_choice(counts, 484, 9, THRESHOLD))


def test_gather_is_test_pys_transpose_per_window():
    rng = np.random.default_rng(0)
    patches = rng.standard_normal((3, 6, 5, 5)).astype(np.float32)
    sel = rng.integers(0, 6, (3, 4, 2)).astype(np.int32)
    x = frame_windows_gather_numpy(patches, sel)
    assert x.shape == (3, 4, 5, 5, 2, 1) and x.dtype == np.float32 and x.flags.c_contiguous
    for n in range(3):
        for j in range(4):
            np.testing.assert_array_equal(x[n, j, :, :, :, 0], patches[n, sel[n, j]].transpose(1, 2, 0))
    with pytest.raises(ValueError):
        frame_windows_gather_numpy(patches, sel[:2])


# ---- the reduce statement -----------------------------------------------------------------------------------------------------------
def test_reduce_ties_go_to_the_even_value():
    for a, b, want in ((10.0, 11.0, 10.0), (11.0, 12.0, 12.0), (0.0, 1.0, 0.0), (65535.0, 65536.0, 65536.0)):
        sr = np.stack([np.full((3, 3), a, np.float32), np.full((3, 3), b, np.float32)])
        assert (frame_windows_reduce_numpy(sr, np.array([[1, 1]], np.int32)) == want).all(), (a, b)
        assert (frame_windows_reduce_numpy(sr, np.array([[7, 7]], np.int32)) == want).all()
    sr = np.stack([np.full((2, 2), 0.0, np.float32), np.full((2, 2), 1.0, np.float32)])
    assert (frame_windows_reduce_numpy(sr, np.array([[3, 1]], np.int32)) == 0.0).all()     # a quarter and three quarters are not ties
    assert (frame_windows_reduce_numpy(sr, np.array([[1, 3]], np.int32)) == 1.0).all()
    assert (frame_windows_reduce_numpy(sr, np.array([[0, 5]], np.int32)) == 1.0).all()     # a zero weight drops the member


def test_reduce_clips_members_and_takes_both_layouts():
    rng = np.random.default_rng(1)
    N, W, S = 3, 4, 10
    sr = synthetic_members(rng, N * W, S)
    w = rng.integers(0, 4357, (N, W)).astype(np.int32)
    w[:, 0] = 1
    out = frame_windows_reduce_numpy(sr, w)
    assert out.shape == (N, S, S) and out.dtype == np.float32 and out.min() >= 0 and out.max() <= HI
    np.testing.assert_array_equal(frame_windows_reduce_numpy(sr[..., None], w), out)
    np.testing.assert_array_equal(frame_windows_reduce_numpy(np.rint(np.clip(sr, 0, HI)), w), out)       # idempotent on rounded members
    p = np.rint(np.clip(sr.astype(np.float64), -500.0, 4000.0)).reshape(N, W, S, S)
    got = frame_windows_reduce_numpy(sr, w, lo=-500.0, hi=4000.0)
    for n in range(N):
        for y in range(S):
            for x in range(S):
                Nn, D = sum(int(w[n, j]) * int(p[n, j, y, x]) for j in range(W)), int(w[n].sum())
                q, r = divmod(Nn, D)
                q += 2 * r > D or (2 * r == D and q % 2 == 1)
                assert got[n, y, x] == float(q)
    for bad_w in (np.zeros((N, W), np.int32), -w, w.astype(np.float32), w[:2]):
        with pytest.raises(ValueError):
            frame_windows_reduce_numpy(sr, bad_w)


def test_one_window_with_uniform_weights_is_the_identity_on_rounded_members():
    rng = np.random.default_rng(2)
    sr = synthetic_members(rng, 5, 30)
    np.testing.assert_array_equal(frame_windows_reduce_numpy(sr, np.ones((5, 1), np.int32)), np.rint(np.clip(sr, 0, HI)))
    np.testing.assert_array_equal(frame_windows_reduce_numpy(sr, np.full((5, 1), 4356, np.int32)), np.rint(np.clip(sr, 0, HI)))


def test_reduce_with_the_largest_weights_does_not_overflow():
    k, pixels, W, S = 9, 1936, 64, 4
    rng = np.random.default_rng(3)
    w = np.full((2, W), k * pixels, np.int32)
    w[1] = rng.integers(0, k * pixels + 1, W)
    sr = np.full((2 * W, S, S), HI, np.float32)
    sr[rng.integers(0, 2 * W, 60), rng.integers(0, S, 60), rng.integers(0, S, 60)] = 65535.0
    out = frame_windows_reduce_numpy(sr, w)
    for n in range(2):
        for y in range(S):
            for x in range(S):
                Nn = sum(int(w[n, j]) * int(sr[n * W + j, y, x]) for j in range(W))        # Python integers: no width at all
                D = sum(int(v) for v in w[n])
                q, r = divmod(Nn, D)
                q += 2 * r > D or (2 * r == D and q % 2 == 1)
                assert out[n, y, x] == float(q)
    assert (frame_windows_reduce_numpy(np.full((W, S, S), 1e9, np.float32), w[:1]) == HI).all()
    assert (frame_windows_reduce_numpy(np.full((W, S, S), HI, np.float32), np.full((1, W), 2 ** 31 - 1, np.int64)) == HI).all()


# ---- the spec -----------------------------------------------------------------------------------------------------------------------
def test_spec_validation():
    s = FrameWindowSpec(3, 5)
    assert (s.windows, s.step, s.weights, s.mode, s.threshold) == (3, 5, "clear", 0, None)
    assert FrameWindowSpec(2, weights="uniform").mode == 1 and FrameWindowSpec(64).windows == 64
    for bad in ((0,), (65,), (-1,), (3, 0), (3, -2)):
        with pytest.raises(ValueError):
            FrameWindowSpec(*bad)
    with pytest.raises(ValueError):
        FrameWindowSpec(3, weights="hat")
    assert s.validate(19, 9) is s
    with pytest.raises(ValueError, match=r"19.*18.*2|18.*largest valid W.*2"):
        s.validate(18, 9)
    assert FrameWindowSpec.largest(18, 9, 5) == 2 and FrameWindowSpec.largest(19, 9, 5) == 3 and FrameWindowSpec.largest(13, 9) == 5
    assert FrameWindowSpec.largest(200, 9) == 64 and FrameWindowSpec.largest(9, 9) == 1
    FrameWindowSpec(5).validate(13, 9)
    with pytest.raises(ValueError):
        FrameWindowSpec(6).validate(13, 9)
    FrameWindowSpec(1).validate(2, 9)                                # one window is the builder's own choice: it tiles a pool shorter than k
    with pytest.raises(ValueError):
        FrameWindowSpec(2).validate(65, 9)
    with pytest.raises(ValueError, match="one patch threshold"):
        s.validate(19, 9, dict(WCONFIG, low_res_patch_thresholds=[0.85, 0.7]))
    with pytest.raises(ValueError, match="one patch threshold"):
        s.bind(dict(WCONFIG, low_res_patch_thresholds=[0.85, 0.7]))
    b = s.bind(WCONFIG)
    assert b.threshold == 0.85 and b.limit(484) == 73 and (b.windows, b.step, b.weights) == (3, 5, "clear")
    with pytest.raises(ValueError, match="threshold"):
        s.limit(484)


def test_chunks_hold_whole_images_within_the_budget():
    from probav_amd.tiles import TileSpec
    spec = FrameWindowSpec(3, 2)
    t8 = TileSpec(8)
    # per image: 225 tiles; inputs 3 * 9 * 484 floats a tile outweigh the unfold (13 * 484) and the predictions (3 * 2304)
    assert fw.images_per_chunk(spec, t8, WCONFIG, 128, 13) == (1 << 30) // (4 * 225 * 27 * 484)
    assert fw.images_per_chunk(FrameWindowSpec(1), t8, WCONFIG, 128, 13) == tiles.images_per_chunk(t8, WCONFIG, 128, 13)
    assert fw.images_per_chunk(spec, t8, WCONFIG, 128, 13, budget=1) == 1
    assert fw.images_per_chunk(spec, TileSpec(16), WCONFIG, 128, 40, budget=1 << 26) == (1 << 26) // (4 * 64 * 40 * 484)


# ---- the ops, without a device ------------------------------------------------------------------------------------------------------
def test_ops_on_fake_tensors_and_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import probav_amd.ops  # noqa: F401
    assert str(torch.ops.probav.frame_windows_gather.default._schema).endswith(
        "(Tensor patches, Tensor counts, SymInt k, SymInt limit, SymInt windows, SymInt step, str mode) -> (Tensor, Tensor, Tensor)")
    assert str(torch.ops.probav.frame_windows_reduce.default._schema).endswith("(Tensor sr, Tensor weight, float lo, float hi) -> Tensor")
    with FakeTensorMode():
        patches, counts = torch.empty(37, 19, 22, 22), torch.empty(37, 19, dtype=torch.int32)
        x, weight, sel = torch.ops.probav.frame_windows_gather(patches, counts, 9, 73, 3, 5, "clear")
        assert tuple(x.shape) == (37, 3, 22, 22, 9, 1) and x.dtype == torch.float32
        assert tuple(weight.shape) == (37, 3) and weight.dtype == torch.int32 and tuple(sel.shape) == (37, 3, 9) and sel.dtype == torch.int32
        x, weight, sel = torch.ops.probav.frame_windows_gather(torch.empty(1, 2, 22, 22), torch.empty(1, 2, dtype=torch.int32), 9, 73, 1, 1, "uniform")
        assert tuple(x.shape) == (1, 1, 22, 22, 9, 1)
        assert tuple(torch.ops.probav.frame_windows_gather(torch.empty(2, 21, 44, 44), torch.empty(2, 21, dtype=torch.int32), 9, 291, 13, 1, "clear")[0].shape) \
            == (2, 13, 44, 44, 9, 1)
        for args in ((patches, counts, 9, 73, 3, 6, "clear"),        # (W - 1) step + k = 21 > 19
                     (patches, counts, 9, 73, 0, 1, "clear"), (patches, counts, 9, 73, 65, 1, "clear"), (patches, counts, 0, 73, 1, 1, "clear"),
                     (patches, counts, 9, 73, 3, 0, "clear"), (patches, counts, 9, -1, 3, 5, "clear"), (patches, counts, 9, 486, 3, 5, "clear"),
                     (patches, counts, 9, 73, 3, 5, "hat"), (patches.double(), counts, 9, 73, 3, 5, "clear"), (patches, counts.long(), 9, 73, 3, 5, "clear"),
                     (patches, counts[:36], 9, 73, 3, 5, "clear"), (torch.empty(37, 19, 22, 21), counts, 9, 73, 3, 5, "clear"),
                     (torch.empty(2, 65, 5, 5), torch.empty(2, 65, dtype=torch.int32), 3, 4, 2, 1, "clear"),
                     (torch.empty(2, 22, 44, 44), torch.empty(2, 22, dtype=torch.int32), 9, 291, 2, 1, "clear")):      # does not fit LDS
            with pytest.raises(ValueError):
                torch.ops.probav.frame_windows_gather(*args)
        w = torch.empty(37, 3, dtype=torch.int32)
        for sr in (torch.empty(111, 48, 48), torch.empty(111, 48, 48, 1)):
            out = torch.ops.probav.frame_windows_reduce(sr, w, 0.0, HI)
            assert tuple(out.shape) == (37, 48, 48) and out.dtype == torch.float32
        sr = torch.empty(111, 48, 48)
        for args in ((sr, w[:36]), (sr, w.long()), (sr.double(), w), (torch.empty(111, 48, 47), w), (sr, torch.empty(111, dtype=torch.int32)),
                     (torch.empty(65, 30, 30), torch.empty(1, 65, dtype=torch.int32))):
            with pytest.raises(ValueError):
                torch.ops.probav.frame_windows_reduce(args[0], args[1], 0.0, HI)
        with pytest.raises(ValueError, match="lo"):
            torch.ops.probav.frame_windows_reduce(sr, w, 1.0, 0.0)
    with pytest.raises(NotImplementedError, match="CPU"):            # real CPU tensors: no CPU kernel, the dispatcher refuses
        torch.ops.probav.frame_windows_gather(torch.zeros(1, 3, 5, 5), torch.zeros(1, 3, dtype=torch.int32), 3, 4, 1, 1, "clear")
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.probav.frame_windows_reduce(torch.zeros(2, 6, 6), torch.ones(1, 2, dtype=torch.int32), 0.0, HI)


def test_resolve_windowed_refuses_a_cpu_model():
    from probav_amd import testClass
    from probav_amd.modelsTF import WDSRConv3D
    model = WDSRConv3D("t", "NIR", 8075.2045, 3160.7272, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        testClass.resolve_windowed(model, torch.zeros(1, 4, 13, 22, 22), torch.zeros(1, 4, 13, dtype=torch.int32), FrameWindowSpec(3, threshold=0.85))


# ---- the CLIs -----------------------------------------------------------------------------------------------------------------------
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
num_low_res_imgs_pre={pre}
low_res_patch_thresholds={thr}
"""


def _load(name):
    spec = importlib.util.spec_from_file_location("probav_cli_fw_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cfg(tmp_path, name, pre=19, thr="0.85"):
    path = str(tmp_path / name)
    with open(path, "w") as fh:
        fh.write(CFG.format(pre=pre, thr=thr))
    return path


def test_cli_frame_window_flags(tmp_path, capsys):
    test_py, evaluate_py = _load("test"), _load("evaluate")
    cfg, cfg2 = _cfg(tmp_path, "c.cfg"), _cfg(tmp_path, "two.cfg", thr="0.85,0.7")
    opt = test_py.parser(["--cfg", "x.cfg", "--band", "NIR"])        # the default reads nothing: today's path
    assert opt.frame_windows == 0 and opt.frame_window_step is None and opt.frame_window_weights is None and opt.windows is None
    opt = test_py.parser(["--cfg", cfg, "--frame-windows", "3"])
    assert (opt.windows.windows, opt.windows.step, opt.windows.weights) == (3, 1, "clear") and (opt.frame_window_step, opt.frame_window_weights) == (1, "clear")
    opt = test_py.parser(["--cfg", cfg, "--frame-windows", "3", "--frame-window-step", "5", "--frame-window-weights", "uniform", "--tile-stride", "8",
                          "--ensemble", "d8", "--weights", "ema"])
    assert (opt.windows.windows, opt.windows.step, opt.windows.weights) == (3, 5, "uniform")
    assert opt.inference.tiles.stride == 8 and opt.inference.ensemble.V == 8
    assert test_py.parser(["--cfg", cfg, "--frame-windows", "11"]).windows.windows == 11       # 10 + 9 == 19
    for bad in (["--cfg", cfg, "--frame-window-step", "2"], ["--cfg", cfg, "--frame-window-weights", "clear"], ["--cfg", cfg, "--frame-windows", "65"],
                ["--cfg", cfg, "--frame-windows", "-1"], ["--cfg", cfg, "--frame-windows", "12"], ["--cfg", cfg, "--frame-windows", "3", "--frame-window-step", "6"],
                ["--cfg", cfg, "--frame-windows", "3", "--frame-window-step", "0"], ["--cfg", cfg, "--frame-windows", "3", "--frame-window-weights", "hat"],
                ["--cfg", cfg, "--frame-windows", "3", "--reference-loop"], ["--cfg", cfg, "--frame-windows", "3", "--method", "baseline"],
                ["--cfg", cfg2, "--frame-windows", "3"], ["--cfg", str(tmp_path / "none.cfg"), "--frame-windows", "3"]):
        with pytest.raises(SystemExit):
            test_py.parser(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        test_py.parser(["--cfg", cfg, "--frame-windows", "4", "--frame-window-step", "5"])
    err = capsys.readouterr().err
    assert "24" in err and "19" in err and "largest valid W at this step is 3" in err      # both numbers and the largest valid W
    with pytest.raises(SystemExit):
        test_py.parser(["--cfg", cfg2, "--frame-windows", "3"])
    assert "one patch threshold" in capsys.readouterr().err

    opt = evaluate_py.parser(["--cfg", cfg, "--model", "--band", "NIR"])
    assert opt.frame_windows == 0 and opt.windows is None
    opt = evaluate_py.parser(["--cfg", cfg, "--model", "--band", "NIR", "--frame-windows", "3", "--frame-window-step", "2", "--tile-stride", "8", "--ensemble", "d8"])
    assert (opt.windows.windows, opt.windows.step, opt.windows.weights, opt.tile_stride) == (3, 2, "clear", 8)
    for bad in (["--cfg", cfg, "--model", "--frame-window-step", "2"], ["--cfg", cfg, "--model", "--frame-windows", "12"],
                ["--cfg", cfg, "--toCompare", str(tmp_path), "--frame-windows", "3"], ["--cfg", cfg, "--baseline", "--frame-windows", "3"],
                ["--cfg", cfg2, "--model", "--frame-windows", "3"], ["--cfg", cfg, "--model", "--frame-windows", "65"]):
        with pytest.raises(SystemExit):
            evaluate_py.parser(bad)
