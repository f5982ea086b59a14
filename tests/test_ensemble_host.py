"""The test-time self-ensemble on the host (probav_amd/ensemble.py, the fake kernels of its two ops, the CLI flags): the variant tables, the
group property the device equivariance test rests on, the numpy statement of the reduction against a line-by-line fp64 restatement, what
is refused.  tests/test_gpu_ensemble.py holds the kernels and the whole path to this statement bit for bit."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from probav_amd import augment, ensemble
from probav_amd.ensemble import EnsembleSpec, ensemble_reduce_numpy, validate_ensemble_recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _G(q, f, k):
    return np.rot90(np.flip(q, augment.FLIP_AXES[f]), k, axes=(0, 1))


def test_tables():
    tab = EnsembleSpec("d8").table(9)
    assert tab.dtype == np.int32 and tab.shape == (8, 11)
    assert [tuple(r[:2]) for r in tab] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]
    np.testing.assert_array_equal(tab[:, 2:], np.broadcast_to(np.arange(9), (8, 9)))
    assert EnsembleSpec("d8").V == 8 and EnsembleSpec(None).V == 1 and EnsembleSpec(None, permute=4, seed=1).V == 5
    np.testing.assert_array_equal(EnsembleSpec(None).table(9), [[0, 0] + list(range(9))])
    np.testing.assert_array_equal(EnsembleSpec("none").table(7), [[0, 0] + list(range(7))])

    a, b, c = (EnsembleSpec("d8", permute=2, seed=s).table(9) for s in (11, 11, 12))
    assert a.shape == (24, 11)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a[:, 2:], c[:, 2:])
    # documented row order: frame order outermost, v = 8 p + 4 f + k; order 0 is the identity, the others are augment.draw_perms' draws
    perms = augment.draw_perms(2, 9, np.random.RandomState(11))
    for v, row in enumerate(a):
        assert tuple(row[:2]) == ((v % 8) // 4, v % 4)
        np.testing.assert_array_equal(row[2:], perms[v // 8])
    only = EnsembleSpec(None, permute=3, seed=5).table(9)
    assert only.shape == (4, 11) and not only[:, :2].any()
    np.testing.assert_array_equal(only[:, 2:], augment.draw_perms(3, 9, np.random.RandomState(5)))

    spec = EnsembleSpec("d8", permute=2, seed=11)
    rec = spec.recipe(5, 9)
    assert rec.dtype == np.int32 and rec.shape == (5 * 24, 12)
    augment.validate_recipe(rec, 5, 9)
    validate_ensemble_recipe(rec, 5, 24, 9)
    np.testing.assert_array_equal(rec[:, 0], np.repeat(np.arange(5), 24))
    np.testing.assert_array_equal(rec[24 * 3: 24 * 4, 1:], a)
    # a spec without a seed still answers with ONE table (expand and reduce must see the same rows)
    free = EnsembleSpec("d8", permute=1)
    np.testing.assert_array_equal(free.table(9), free.table(9))


def test_d8_is_eight_distinct_maps_closed_under_every_code():
    """On an index image: the eight G_v differ pairwise, and G_(f, k) after any G_v of the table is again a G_w of the table -- so the member
    set of E(A(x)) is the member set of E(x), which with an exact sum makes the ensemble equivariant although the network is not."""
    q = np.arange(7 * 7).reshape(7, 7)
    d8 = [tuple(r[:2]) for r in EnsembleSpec("d8").table(3)]
    images = [_G(q, f, k) for f, k in d8]
    for i in range(8):
        for j in range(i):
            assert not np.array_equal(images[i], images[j]), (d8[i], d8[j])
    for f in range(4):
        for k in range(4):
            hits = sorted(next(w for w in range(8) if np.array_equal(_G(m, f, k), images[w])) for m in images)
            assert hits == list(range(8)), (f, k, hits)
    # and G^-1 as the kernel applies it undoes G, for all 16 codes
    for f in range(4):
        for k in range(4):
            np.testing.assert_array_equal(ensemble.inverse_geometry(_G(q, f, k), f, k), q)


def _restate(sr, recipe, V, lo, hi, final):
    """E, pixel by pixel in Python floats (fp64), rounding to fp32 only where the definition does."""
    N, S = sr.shape[0] // V, sr.shape[1]
    out = np.empty((N, S, S), np.float32)
    n1 = S - 1
    for n in range(N):
        for y in range(S):
            for x in range(S):
                total = 0.0
                for v in range(V):
                    f, k = int(recipe[n * V + v, 1]), int(recipe[n * V + v, 2])
                    a, b = (n1 - y if f & 1 else y), (n1 - x if f & 2 else x)
                    yy, xx = ((a, b), (n1 - b, a), (n1 - a, n1 - b), (b, n1 - a))[k]
                    val = min(max(float(sr[n * V + v, yy, xx]), lo), hi)
                    total += float(np.round(val))               # half to even; every term and the running total are integers below 2**53
                e = np.float32(np.float64(total) / np.float64(V))          # one rounding of the exact quotient's fp64 value: the fp32 division
                out[n, y, x] = np.rint(e) if final == "round" else e
    return out


def test_reduce_numpy_recovers_the_image_and_matches_the_restatement():
    rng = np.random.default_rng(3)
    for spec in (EnsembleSpec("d8"), EnsembleSpec("d8", permute=2, seed=1), EnsembleSpec(None)):
        N, S, V = 3, 12, spec.V
        rec = spec.recipe(N, 5)
        q = rng.integers(0, 2 ** 16 + 1, (N, S, S)).astype(np.float32)
        members = np.stack([_G(q[r[0]], r[1], r[2]) for r in rec])
        for final in ("mean", "round"):
            got = ensemble_reduce_numpy(members, rec, V, final=final)
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, q)
            np.testing.assert_array_equal(ensemble_reduce_numpy(members[..., None], rec, V, final=final), q)
    # hand-made members: ties at x.5 (even and odd x), negatives, values beyond 2**16, a NaN-free mix; V that does not divide the sums
    for V, spec in ((3, EnsembleSpec(None, permute=2, seed=4)), (8, EnsembleSpec("d8")), (24, EnsembleSpec("d8", permute=2, seed=9))):
        N, S = 2, 6
        rec = spec.recipe(N, 4)
        sr = rng.integers(-40, 2 ** 16 + 40, (N * V, S, S)).astype(np.float32)
        sr[:, 0, :] += np.float32(0.5)                                                       # ties
        sr[:, 1, :3] = np.array([0.5, 1.5, 2.5], np.float32)
        sr[:, 2, :3] = np.array([-0.5, -7.25, 65535.5], np.float32)
        sr[:, 3, :3] = np.array([65536.5, 70000.0, 65536.0], np.float32)
        sr[:, 4] = rng.random((N * V, S)).astype(np.float32) * 7 + rng.integers(0, 3, (N * V, S)) * np.float32(0.5)
        for final in ("mean", "round"):
            got = ensemble_reduce_numpy(sr, rec, V, final=final)
            want = _restate(sr, rec, V, 0.0, 65536.0, final)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
            if final == "mean" and V == 3:
                assert np.any(got != np.rint(got))                                           # thirds: the two forms really differ
        # other clip bounds
        np.testing.assert_array_equal(ensemble_reduce_numpy(sr, rec, V, lo=10.0, hi=300.0), _restate(sr, rec, V, 10.0, 300.0, "mean"))
    # the stitched form is the row-major block layout of test.py:149-160
    spec = EnsembleSpec("d8")
    rec = spec.recipe(8, 4)
    sr = rng.integers(0, 2 ** 16, (64, 6, 6)).astype(np.float32)
    patches = ensemble_reduce_numpy(sr, rec, 8)
    img = ensemble_reduce_numpy(sr, rec, 8, sets=2, grid=2)
    assert img.shape == (2, 12, 12)
    for s in range(2):
        for i in range(2):
            for j in range(2):
                np.testing.assert_array_equal(img[s, 6 * i:6 * i + 6, 6 * j:6 * j + 6], patches[4 * s + 2 * i + j])


def test_fp32_division_equals_the_fp64_route():
    """What lets the GPU test compare a float64 composition with the fp32 kernel bit for bit: for integer sums up to 2**24 and V <= 256 the
    fp64 quotient rounded to fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2)."""
    rng = np.random.default_rng(0)
    s = rng.integers(0, 2 ** 24 + 1, 200000)
    v = rng.integers(1, 257, 200000)
    s = np.minimum(s, v * 65536)
    np.testing.assert_array_equal((s.astype(np.float64) / v).astype(np.float32), s.astype(np.float32) / v.astype(np.float32))


def test_what_is_refused():
    with pytest.raises(ValueError, match="2\\*\\*24"):
        EnsembleSpec("d8", permute=32)                              # 8 x 33 = 264 members
    EnsembleSpec("d8", permute=31)                                  # 256: the bound itself is allowed
    with pytest.raises(ValueError, match="2\\*\\*24"):
        EnsembleSpec(None, permute=256)                             # 257
    with pytest.raises(ValueError):
        EnsembleSpec("d4")
    with pytest.raises(ValueError):
        EnsembleSpec("d8", permute=-1)
    spec = EnsembleSpec("d8")
    rec = spec.recipe(4, 9)
    validate_ensemble_recipe(rec, 4, 8, 9)
    sr = np.zeros((32, 6, 6), np.float32)
    ensemble_reduce_numpy(sr, rec, 8)
    swapped = rec.copy()
    swapped[[7, 8]] = swapped[[8, 7]]                               # every row valid, but row 7 now belongs to patch 1
    augment.validate_recipe(swapped, 4, 9)
    for bad in (swapped, rec[::-1].copy(), np.tile(spec.table(9), (4, 1)).astype(np.int32)[:, [0] + list(range(11))]):
        with pytest.raises(ValueError):
            validate_ensemble_recipe(bad, 4, 8, 9)
    with pytest.raises(ValueError, match="grouped"):
        ensemble_reduce_numpy(sr, swapped, 8)
    with pytest.raises(ValueError, match="2\\*\\*24"):
        validate_ensemble_recipe(np.zeros((257, 12), np.int32), 1, 257, 9)
    with pytest.raises(ValueError, match="2\\*\\*24"):
        ensemble_reduce_numpy(np.zeros((257, 6, 6), np.float32), np.zeros((257, 12), np.int32), 257)
    with pytest.raises(ValueError):
        ensemble_reduce_numpy(sr, rec, 8, final="floor")
    with pytest.raises(ValueError):
        ensemble_reduce_numpy(sr, rec, 8, sets=3, grid=1)
    bad_code = rec.copy()
    bad_code[5, 2] = 4
    with pytest.raises(ValueError):
        ensemble_reduce_numpy(sr, bad_code, 8)


def test_ops_on_fake_tensors_and_cpu_tensors(built_lib):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import probav_amd.ops  # noqa: F401
    assert str(torch.ops.probav.ensemble_expand.default._schema).endswith("(Tensor lr, Tensor recipe) -> Tensor")
    assert str(torch.ops.probav.ensemble_reduce.default._schema).endswith(
        "(Tensor sr, Tensor recipe, SymInt V, float lo, float hi, bool final_round, SymInt sets, SymInt grid) -> Tensor")
    with FakeTensorMode():
        lr, rec = torch.empty(6, 22, 22, 9, 1), torch.empty(48, 12, dtype=torch.int32)
        out = torch.ops.probav.ensemble_expand(lr, rec)
        assert tuple(out.shape) == (48, 22, 22, 9, 1) and out.dtype == torch.float32
        assert tuple(torch.ops.probav.ensemble_expand(torch.empty(6, 30, 30, 7, 3), torch.empty(5, 10, dtype=torch.int32)).shape) == (5, 30, 30, 7, 3)
        for bad in ((torch.empty(6, 22, 21, 9, 1), rec), (lr, torch.empty(48, 11, dtype=torch.int32)), (lr, rec.long()), (lr.double(), rec),
                    (torch.empty(6, 22, 22, 9), rec)):
            with pytest.raises(ValueError):
                torch.ops.probav.ensemble_expand(*bad)
        for sr in (torch.empty(128 * 8, 48, 48), torch.empty(128 * 8, 48, 48, 1)):
            rec = torch.empty(128 * 8, 12, dtype=torch.int32)
            p = torch.ops.probav.ensemble_reduce(sr, rec, 8, 0.0, 65536.0, False, 0, 0)
            assert tuple(p.shape) == (128, 48, 48) and p.dtype == torch.float32
            im = torch.ops.probav.ensemble_reduce(sr, rec, 8, 0.0, 65536.0, True, 2, 8)
            assert tuple(im.shape) == (2, 384, 384) and im.dtype == torch.float32
        sr, rec = torch.empty(64, 30, 30), torch.empty(64, 12, dtype=torch.int32)
        assert tuple(torch.ops.probav.ensemble_reduce(sr, rec, 1, 0.0, 65536.0, False, 0, 0).shape) == (64, 30, 30)
        assert tuple(torch.ops.probav.ensemble_reduce(sr, rec, 4, 0.0, 65536.0, False, 4, 2).shape) == (4, 60, 60)
        for args in ((sr, rec, 0, 0, 0), (sr, rec, 3, 0, 0), (sr, rec, 4, 3, 2), (sr, rec, 4, 0, 2), (sr, rec, 4, 4, 0),
                     (sr, torch.empty(63, 12, dtype=torch.int32), 1, 0, 0), (sr.double(), rec, 4, 0, 0), (torch.empty(64, 30, 29), rec, 4, 0, 0)):
            with pytest.raises(ValueError):
                torch.ops.probav.ensemble_reduce(args[0], args[1], args[2], 0.0, 65536.0, False, args[3], args[4])
        with pytest.raises(ValueError, match="sum exactly in fp32"):
            torch.ops.probav.ensemble_reduce(torch.empty(257, 30, 30), torch.empty(257, 12, dtype=torch.int32), 257, 0.0, 65536.0, False, 0, 0)
    with pytest.raises(NotImplementedError, match="CPU"):            # real CPU tensors: no CPU kernel, the dispatcher refuses
        torch.ops.probav.ensemble_expand(torch.zeros(2, 6, 6, 4, 1), torch.zeros(2, 7, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.probav.ensemble_reduce(torch.zeros(8, 6, 6), torch.zeros(8, 7, dtype=torch.int32), 8, 0.0, 65536.0, False, 0, 0)


def test_resolve_ensemble_refuses_a_cpu_model(built_lib):
    from probav_amd import testClass
    from probav_amd.modelsTF import WDSRConv3D
    model = WDSRConv3D("t", "NIR", 8075.2045, 3160.7272, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        testClass.resolve_ensemble(model, np.zeros((2, 22, 22, 9, 1), np.float32), EnsembleSpec("d8"))
    with pytest.raises(ValueError):
        testClass.resolve_ensemble(model, np.zeros((2, 22, 22, 9, 1), np.float32), EnsembleSpec("d8"), final="floor")


def _load(name):
    spec = importlib.util.spec_from_file_location("probav_cli_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_default_to_the_plain_path(tmp_path):
    test_py, evaluate_py = _load("test"), _load("evaluate")
    opt = test_py.parser(["--cfg", "x.cfg", "--band", "NIR"])
    assert (opt.ensemble, opt.ensemble_permute, opt.ensemble_seed) == ("none", 0, 0)
    assert opt.inference.ensemble is None
    opt = test_py.parser(["--ensemble", "d8", "--ensemble-permute", "1", "--ensemble-seed", "3"])
    spec = opt.inference.ensemble
    assert (spec.geometry, spec.permute, spec.seed, spec.V) == ("d8", 1, 3, 16)
    for bad in (["--ensemble", "d4"], ["--ensemble-permute", "2"], ["--ensemble", "d8", "--reference-loop"]):
        with pytest.raises(SystemExit):
            test_py.parser(bad)
    cfg = tmp_path / "c.cfg"
    cfg.write_text("")
    opt = evaluate_py.parser(["--cfg", str(cfg), "--model", "--band", "NIR"])
    assert (opt.ensemble, opt.ensemble_permute, opt.ensemble_seed) == ("none", 0, 0)
    opt = evaluate_py.parser(["--cfg", str(cfg), "--model", "--ensemble", "d8", "--ensemble-permute", "2", "--ensemble-seed", "7"])
    assert (opt.ensemble, opt.ensemble_permute, opt.ensemble_seed) == ("d8", 2, 7)
    with pytest.raises(SystemExit):
        evaluate_py.parser(["--cfg", str(cfg), "--toCompare", str(tmp_path), "--ensemble", "d8"])
