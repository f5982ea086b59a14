"""Overlapped-tile inference, the host half (probav_amd/tiles.py): the tile grid and the windows, the numpy int64 statement of the blend, the
frame selection of the tile builder against the dataset builder's own functions, the op's schema on fake tensors, the CLI flags.
Every comparison is an equality: the feature has no tolerances."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from probav_amd import tiles
from probav_amd.testClass import reconstruct_from_patches
from probav_amd.tiles import TileSpec, tile_blend_numpy

from tests.tiles_helpers import CONFIG, HI, cloudy_frames, masked_patches, numpy_unfold, synthetic_members, tile_inputs_by_the_builder, torch_unfold_seam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- TileSpec -----------------------------------------------------------------------------------------------------------------------
def test_valid_strides_and_the_grid():
    assert tiles.valid_strides(16, 128) == [1, 2, 4, 7, 8, 14, 16]
    for s in (1, 2, 4, 7, 8, 14, 16):
        assert TileSpec(s).validate(16, 128).n(16, 128) == 112 // s + 1
    for s in (3, 0, 17, 32, -8):
        with pytest.raises(ValueError, match=r"valid strides: \[1, 2, 4, 7, 8, 14, 16\]"):
            TileSpec(s).validate(16, 128)
        with pytest.raises(ValueError):
            TileSpec(s).n(16, 128)
    assert TileSpec(8).n(16, 128) == 15 and TileSpec(16).n(16, 128) == 8 and TileSpec(1).n(16, 128) == 113
    o = TileSpec(8).origins(16, 128, scale=3)
    assert o.shape == (225, 2)
    assert o[:3].tolist() == [[0, 0], [0, 24], [0, 48]] and o[15].tolist() == [24, 0] and o[-1].tolist() == [336, 336]      # row-major
    assert TileSpec(8).origins(16, 128)[16].tolist() == [8, 8]
    assert 336 + 48 == 384


def test_windows():
    w = TileSpec(8, "hat").weights(48)
    assert w.dtype == np.int32 and w.tolist() == list(range(1, 25)) + list(range(24, 0, -1))
    assert TileSpec(8, "hat").weights(5).tolist() == [1, 2, 3, 2, 1]
    b = TileSpec(8, "box").weights(48)
    assert b.dtype == np.int32 and b.tolist() == [1] * 48
    assert TileSpec(8).window == "hat"
    with pytest.raises(ValueError):
        TileSpec(8, "gauss")
    assert TileSpec(8, np.full(48, 1024)).weights(48).tolist() == [1024] * 48
    for bad in (np.full(48, 1025), np.zeros(48, np.int64), np.r_[np.ones(47, np.int64), -1], np.ones(47, np.int64), np.ones(48)):
        with pytest.raises(ValueError):
            TileSpec(8, bad).weights(48)
        with pytest.raises(ValueError):
            tile_blend_numpy(np.zeros((4, 48, 48), np.float32), bad, 2, 24)
    with pytest.raises(ValueError):                               # hat for S = 2050 peaks at 1025
        TileSpec(8, "hat").weights(2050)


# ---- tile_blend_numpy ---------------------------------------------------------------------------------------------------------------
def test_stride_of_a_whole_tile_is_the_plain_stitch():
    rng = np.random.default_rng(0)
    raw = synthetic_members(rng, 2 * 64, 48)
    members = np.rint(np.clip(raw, 0, HI))
    for window in ("hat", "box"):
        w = TileSpec(16, window).weights(48)
        out = tile_blend_numpy(raw, w, 8, 48)
        assert out.shape == (2, 384, 384) and out.dtype == np.float32
        for i in range(2):
            want = reconstruct_from_patches(members[i * 64:(i + 1) * 64, :, :, None])
            np.testing.assert_array_equal(out[i].astype(np.float64), want[:, :, 0])
        np.testing.assert_array_equal(tile_blend_numpy(members[..., None], w, 8, 48), out)          # idempotent on rounded members, [..., 1] accepted


def test_constant_members_give_the_constant():
    for window in ("hat", "box"):
        for S, hs, n in ((48, 24, 15), (48, 21, 17), (30, 15, 5), (90, 3, 4)):
            w = TileSpec(1, window).weights(S)
            for v in (0.0, 1.0, 12345.0, HI):
                out = tile_blend_numpy(np.full((n * n, S, S), v, np.float32), w, n, hs)
                assert out.shape == (1, (n - 1) * hs + S, (n - 1) * hs + S)
                assert (out == v).all(), (window, S, hs, n, v)


def test_hat_weights_of_two_tiles_sum_to_25():
    S, hs, n = 48, 24, 15
    w = TileSpec(8, "hat").weights(S).astype(np.int64)
    G = (n - 1) * hs + S
    D1 = np.zeros(G, np.int64)
    for a in range(n):
        D1[a * hs:a * hs + S] += w
    assert (D1[hs:G - hs] == 25).all() and D1[:hs].tolist() == list(range(1, 25))
    # ... and the blend's D is its outer product: a member that is 25 * 25 in one tile and 0 elsewhere comes back as that tile's W2 in the interior
    members = np.zeros((n * n, S, S), np.float32)
    members[7 * n + 7] = 625.0
    out = tile_blend_numpy(members, w, n, hs)
    np.testing.assert_array_equal(out[0, 7 * hs:7 * hs + S, 7 * hs:7 * hs + S], np.outer(w, w).astype(np.float32))
    assert out.sum() == np.outer(w, w).sum()


def test_exact_halves_go_to_the_even_value():
    S, hs, n = 4, 2, 2                                            # box: pixels under two tiles average two members, the centre four
    w = np.ones(S, np.int64)
    for lo_first in (True, False):
        for base in (10.0, 11.0, 0.0, 65535.0):
            m = np.full((4, S, S), base, np.float32)
            m[1 if lo_first else 0] += 1.0                         # tiles (0, 0) and (0, 1) differ by one: their overlap is an exact half
            m[2:] = m[:2]
            out = tile_blend_numpy(m, w, n, hs)
            even = base if base % 2 == 0 else base + 1
            assert (out[0, :, 2:4] == even).all(), (lo_first, base, out[0, 0])
            assert (out[0, :, :2] == m[0, 0, 0]).all() and (out[0, :, 4:] == m[1, 0, 0]).all()
    # three quarters and one quarter are not ties
    m = np.zeros((4, S, S), np.float32)
    m[0] = 1.0
    assert (tile_blend_numpy(m, w, n, hs)[0, 2:4, 2:4] == 0.0).all()
    m[1], m[2] = 1.0, 1.0
    assert (tile_blend_numpy(m, w, n, hs)[0, 2:4, 2:4] == 1.0).all()


def test_largest_values_do_not_overflow():
    S, hs, n = 90, 3, 4
    rng = np.random.default_rng(5)
    w = np.full(S, 1024, np.int64)
    w[::7] = rng.integers(1, 1025, len(w[::7]))
    m = np.full((n * n, S, S), HI, np.float32)
    m[rng.integers(0, n * n, 40), rng.integers(0, S, 40), rng.integers(0, S, 40)] = 65535.0
    out = tile_blend_numpy(m, w, n, hs)
    G = (n - 1) * hs + S
    assert out.shape == (1, G, G)
    for y, x in [(0, 0), (G - 1, G - 1), (45, 50), (9, 91), (50, 8), (89, 89), (12, 12)] + [tuple(rng.integers(0, G, 2)) for _ in range(12)]:
        N = D = 0                                                  # Python integers: no width at all
        for a in range(n):
            for c in range(n):
                dy, dx = int(y) - a * hs, int(x) - c * hs
                if 0 <= dy < S and 0 <= dx < S:
                    N += int(w[dy]) * int(w[dx]) * int(m[a * n + c, dy, dx])
                    D += int(w[dy]) * int(w[dx])
        q, r = divmod(N, D)
        q += 2 * r > D or (2 * r == D and q % 2 == 1)
        assert out[0, y, x] == float(q), (y, x, N, D)
    assert (tile_blend_numpy(np.full((n * n, S, S), 1e9, np.float32), np.full(S, 1024), n, hs) == HI).all()


def test_blend_arguments():
    m = np.zeros((8, 6, 6), np.float32)
    w = np.ones(6, np.int64)
    for args in ((m, w, 2, 0), (m, w, 2, 7), (m, w, 3, 3), (m[:, :, :5], w, 2, 3), (m[:0], w, 2, 3)):
        with pytest.raises(ValueError):
            tile_blend_numpy(*args)
    assert tile_blend_numpy(m, w, 2, 6).shape == (2, 12, 12) and tile_blend_numpy(m, w, 2, 1).shape == (2, 7, 7)
    np.testing.assert_array_equal(tile_blend_numpy(np.full((4, 6, 6), 77.0), w, 2, 3, lo=100.0, hi=200.0), np.full((1, 9, 9), 100.0, np.float32))


# ---- the host half of the tile builder ----------------------------------------------------------------------------------------------
def _kinds(counts, pixels, thr):
    passing = (counts / pixels < (1 - thr)).sum(-1)
    return (passing == 0).sum(), ((passing > 0) & (passing < counts.shape[-1])).sum(), (passing == counts.shape[-1]).sum()


@pytest.mark.parametrize("stride,thresholds", [(16, [0.85]), (8, [0.85]), (16, [0.85, 0.7]), (14, [0.6, 0.85])],
                         ids=["s16", "s8", "s16-two-thresholds", "s14-two-thresholds"])
def test_selection_path_equals_the_dataset_builders(stride, thresholds):
    frames = cloudy_frames()
    assert frames.shape == (3, 9, 1, 128, 128)
    config = dict(CONFIG, low_res_patch_thresholds=thresholds)
    data, mask = np.ma.getdata(frames).reshape(3, 9, 128, 128), np.ma.getmaskarray(frames).reshape(3, 9, 128, 128)
    unfolded = numpy_unfold(data, mask, 3, 22, stride)
    n = 112 // stride + 1
    assert unfolded[0].shape == (3, n * n, 9, 22, 22)
    none, some, every = _kinds(unfolded[2], 22 * 22, 0.85)
    assert none > 0 and some > 0 and every > 0, (none, some, every)          # tiles with 0, with 1..8 and with all 9 frames passing
    want = tile_inputs_by_the_builder(masked_patches(unfolded), config)
    assert want.shape == (3, n * n, 22, 22, 9, 1) and want.dtype == np.float32
    got = tiles.build_tiles(frames, TileSpec(stride), config, device="cpu", unfold=torch_unfold_seam)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.is_contiguous()
    np.testing.assert_array_equal(got.numpy(), want)
    # the selection moved frames: the tiles are not simply the unfold in frame order
    assert not np.array_equal(want, unfolded[0].transpose(0, 1, 3, 4, 2)[..., None])


def test_selection_with_more_frames_than_the_network_takes():
    frames = cloudy_frames(images=2, T=11, seed=3)
    config = dict(CONFIG, num_low_res_imgs_pre=11, low_res_patch_thresholds=[0.85, 0.85])
    data, mask = np.ma.getdata(frames).reshape(2, 11, 128, 128), np.ma.getmaskarray(frames).reshape(2, 11, 128, 128)
    want = tile_inputs_by_the_builder(masked_patches(numpy_unfold(data, mask, 3, 22, 16)), config)
    got = tiles.build_tiles(frames, TileSpec(16), config, device="cpu", unfold=torch_unfold_seam)
    assert tuple(got.shape) == (2, 64, 22, 22, 9, 1)
    np.testing.assert_array_equal(got.numpy(), want)


def test_chunks_hold_whole_images_within_the_budget():
    per8 = tiles.images_per_chunk(TileSpec(8), CONFIG, 128, 9)
    assert per8 == (1 << 30) // (4 * 225 * 9 * 22 * 22)             # the unfolded tile (9 * 22 * 22 floats) outweighs its prediction (48 * 48)
    assert tiles.images_per_chunk(TileSpec(1), CONFIG, 128, 9) == (1 << 30) // (4 * 12769 * 9 * 22 * 22) == 4
    assert tiles.images_per_chunk(TileSpec(8), CONFIG, 128, 2) == (1 << 30) // (4 * 225 * 48 * 48)
    assert tiles.images_per_chunk(TileSpec(8), CONFIG, 128, 9, budget=1) == 1
    assert tiles.images_per_chunk(TileSpec(8), CONFIG, 128, 30, budget=1 << 26) == (1 << 26) // (4 * 225 * 30 * 484)
    with pytest.raises(ValueError):
        tiles.images_per_chunk(TileSpec(3), CONFIG, 128, 9)


# ---- the op, without a device -------------------------------------------------------------------------------------------------------
def test_op_on_fake_tensors_and_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import probav_amd.ops  # noqa: F401
    assert str(torch.ops.probav.tile_blend.default._schema).endswith(
        "(Tensor sr, Tensor w, SymInt n_images, SymInt n, SymInt hr_stride, float lo, float hi) -> Tensor")
    with FakeTensorMode():
        w = torch.empty(48, dtype=torch.int32)
        for sr in (torch.empty(3 * 225, 48, 48), torch.empty(3 * 225, 48, 48, 1)):
            out = torch.ops.probav.tile_blend(sr, w, 3, 15, 24, 0.0, HI)
            assert tuple(out.shape) == (3, 384, 384) and out.dtype == torch.float32
        assert tuple(torch.ops.probav.tile_blend(torch.empty(64, 48, 48), w, 1, 8, 48, 0.0, HI).shape) == (1, 384, 384)
        assert tuple(torch.ops.probav.tile_blend(torch.empty(32, 90, 90), torch.empty(90, dtype=torch.int32), 2, 4, 3, 0.0, HI).shape) == (2, 99, 99)
        sr = torch.empty(225, 48, 48)
        for args in ((sr, w, 1, 15, 0), (sr, w, 1, 15, 49), (sr, w, 1, 14, 24), (sr, w, 2, 15, 24), (sr, w.long(), 1, 15, 24), (sr.double(), w, 1, 15, 24),
                     (sr, torch.empty(47, dtype=torch.int32), 1, 15, 24), (torch.empty(225, 48, 47), w, 1, 15, 24), (sr, w, 0, 15, 24)):
            with pytest.raises(ValueError):
                torch.ops.probav.tile_blend(args[0], args[1], args[2], args[3], args[4], 0.0, HI)
        with pytest.raises(ValueError, match="lo"):
            torch.ops.probav.tile_blend(sr, w, 1, 15, 24, 1.0, 0.0)
    with pytest.raises(NotImplementedError, match="CPU"):            # real CPU tensors: no CPU kernel, the dispatcher refuses
        torch.ops.probav.tile_blend(torch.zeros(4, 6, 6), torch.ones(6, dtype=torch.int32), 1, 2, 3, 0.0, HI)


def test_resolve_tiled_refuses_a_cpu_model():
    from probav_amd import testClass
    from probav_amd.modelsTF import WDSRConv3D
    model = WDSRConv3D("t", "NIR", 8075.2045, 3160.7272, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        testClass.resolve_tiled(model, np.zeros((1, 4, 22, 22, 9, 1), np.float32), TileSpec(8))


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
patch_size={P}
low_res_patch_thresholds=0.85
"""


def _load(name):
    spec = importlib.util.spec_from_file_location("probav_cli_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_tile_flags(tmp_path):
    test_py, evaluate_py = _load("test"), _load("evaluate")
    cfg, cfg32 = str(tmp_path / "c.cfg"), str(tmp_path / "c32.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(P=16))
    with open(cfg32, "w") as fh:
        fh.write(CFG.format(P=32))
    opt = test_py.parser(["--cfg", "x.cfg", "--band", "NIR"])       # the default reads nothing: today's path
    assert opt.tile_stride == 0 and opt.tile_window is None and opt.inference.tiles is None
    opt = test_py.parser(["--cfg", cfg, "--tile-stride", "8"])
    spec = opt.inference.tiles
    assert (spec.stride, spec.window) == (8, "hat") and opt.tile_window == "hat"
    opt = test_py.parser(["--cfg", cfg, "--tile-stride", "4", "--tile-window", "box", "--ensemble", "d8"])
    assert (opt.inference.tiles.stride, opt.inference.tiles.window, opt.inference.ensemble.V) == (4, "box", 8)
    assert test_py.parser(["--cfg", cfg32, "--tile-stride", "32"]).inference.tiles.stride == 32      # valid for THAT cfg: (128 - 32) % 32 == 0
    for bad in (["--cfg", cfg, "--tile-window", "hat"], ["--cfg", cfg, "--tile-stride", "8", "--reference-loop"], ["--cfg", cfg, "--tile-stride", "3"],
                ["--cfg", cfg, "--tile-stride", "32"], ["--cfg", cfg, "--tile-stride", "-8"], ["--cfg", cfg, "--tile-stride", "8", "--tile-window", "gauss"],
                ["--cfg", cfg32, "--tile-stride", "7"], ["--cfg", str(tmp_path / "none.cfg"), "--tile-stride", "8"]):
        with pytest.raises(SystemExit):
            test_py.parser(bad)
    opt = evaluate_py.parser(["--cfg", cfg, "--model", "--band", "NIR"])
    assert opt.tile_stride == 0 and opt.tile_window is None
    opt = evaluate_py.parser(["--cfg", cfg, "--model", "--band", "NIR", "--tile-stride", "8", "--ensemble", "d8"])
    assert (opt.tile_stride, opt.tile_window, opt.ensemble) == (8, "hat", "d8")
    for bad in (["--cfg", cfg, "--model", "--tile-window", "box"], ["--cfg", cfg, "--model", "--tile-stride", "5"],
                ["--cfg", cfg, "--toCompare", str(tmp_path), "--tile-stride", "8"]):
        with pytest.raises(SystemExit):
            evaluate_py.parser(bad)


def test_cli_error_lists_the_valid_strides(tmp_path, capsys):
    test_py = _load("test")
    cfg = str(tmp_path / "c.cfg")
    with open(cfg, "w") as fh:
        fh.write(CFG.format(P=16))
    with pytest.raises(SystemExit):
        test_py.parser(["--cfg", cfg, "--tile-stride", "3"])
    assert "[1, 2, 4, 7, 8, 14, 16]" in capsys.readouterr().err
