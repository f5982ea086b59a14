"""Host tables and the cfg reader (no GPU)."""
import os

import pytest

from probav_amd.arch import layer_table, reducer_plan
from probav_amd.parseConfig import parseConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_variable_inventory_matches_reference_checkpoint():
    """modelInfo/ckpt_p16t9c85r12/NIR/ckpt-124.index: 44 weight-normalised layers, 535 267 fp32
    (SURVEY.md F3, A.1), in Keras topological order."""
    layers, total = layer_table()
    assert len(layers) == 44 and total == 535267 and total * 4 == 2141068
    names = [L.name for L in layers]
    assert names[0] == "mainConv1"
    assert names[1:4] == ["expConv_0", "decConv_0", "normConv_0"]
    assert names[37:] == ["convReducer_1", "convReducer_2", "convReducer_3", "residConv1", "upscaleConv1", "residConv2", "residConv3"]
    per = {L.name: 2 * L.cout + (L.b_off - L.v_off) for L in layers}
    assert per["mainConv1"] == 928 and per["expConv_3"] == 8704 and per["decConv_3"] == 6450
    assert per["normConv_3"] == 21664 and per["convReducer_2"] == 27712 and per["residConv1"] == 99
    assert per["upscaleConv1"] == 7794 and per["residConv2"] == 747
    assert layers[2].vshape == (1, 1, 1, 256, 25) and layers[40].vshape == (3, 3, 1, 9)
    # contiguous, non-overlapping flat layout
    off = 0
    for L in layers:
        assert (L.g_off, L.v_off) == (off, off + L.cout)
        off = L.b_off + L.cout
    assert off == total


def test_three_channel_branch_and_kernel_size():
    """isGrayScale=False touches the two input-facing layers only (models/modelsTF.py:19-20); kernelSize != 3 is refused like the reference's
    own graph refuses it (its valid reducers and residual path only close for 3: the docstring of WDSRConv3D.build)."""
    from probav_amd.modelsTF import WDSRConv3D
    layers, total = layer_table(inChannels=3)
    assert total == 535267 + 27 * 2 * 32 + 9 * 2 * 9
    assert layers[0].vshape == (3, 3, 3, 3, 32) and layers[40].vshape == (3, 3, 3, 9) and layers[1].vshape == (1, 1, 1, 32, 256)
    b = WDSRConv3D("t", "NIR", 8075.2045, 3160.7272, 6)
    m = b.build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, False, seed=0)
    assert m.inChannels == 3 and m.flat.numel() == total and len(m.trainable_variables) == 132
    assert b.build(3, 32, 3, 12, 8, 0.8, 9, 16, True, seed=0).inChannels == 1
    with pytest.raises(ValueError):
        b.build(3, 32, (5, 5, 5), 12, 8, 0.8, 9, 16, True)
    # why: the reference's 9-frame graph with k = 5 -- depth 9 -> 5 -> 1 -> negative at the third valid reducer (models/modelsTF.py:152-164)
    t = 9
    for _ in range(3):
        t -= 5 - 1
    assert t < 1


def test_reducer_plans():
    a, b = (3, 1, 0), (3, 0, 0)                              # (kernel, mirrored H/W pad, mirrored depth pad)
    assert reducer_plan(9) == (a, b, b)                      # models/modelsTF.py:152-164
    assert reducer_plan(13) == (a, a, a, b, b)               # :123-150
    assert reducer_plan(7) == (b, b)                         # :166-175
    assert reducer_plan(19) == ((5, 2, 2), (3, 2, 1), (3, 2, 0), (3, 2, 0), a, b, b, b, b, b)   # :76-121
    with pytest.raises(ValueError):
        reducer_plan(12)                                     # a literal 12-frame net is undefined
    assert layer_table(numImgLR=13)[1] == 535267 + 2 * 27712
    # 19 frames: seven more reducers than t9, the first with a 5x5x5 kernel (125*32*32 weights + g + bias)
    assert layer_table(numImgLR=19)[1] == 535267 + 6 * 27712 + (125 * 32 * 32 + 64)
    h, t = 22, 19                                            # the 19-frame chain must end at P x P x 1 before the Reshape (:71)
    for k, p, pt in reducer_plan(19) + ((3, 0, 0),):
        h, t = h + 2 * p - k + 1, t + 2 * pt - k + 1
    assert (h, t) == (16, 1)


@pytest.mark.parametrize("name", ["p16t9c85r12", "p16t12c85r12"])
def test_shipped_cfgs_parse(name):
    cfg = parseConfig(os.path.join(ROOT, "cfg", name + ".cfg"))
    assert cfg["num_low_res_imgs"] == 9 and cfg["num_res_blocks"] == 12 and cfg["num_filters"] == 32
    assert cfg["batch_size"] == 128 and cfg["learning_rate"] == 0.0005 and cfg["optimizer"] == "nadam" and cfg["loss"] == "l1"
    assert cfg["decay_rate"] == 0.8 and cfg["is_grayscale"] is True and cfg["max_shift"] == 6 and cfg["patch_size"] == 16
    assert cfg["ckpt"] == [1, 2, 3, 4, 5] and cfg["to_flip"] is False and isinstance(cfg["model_out"], str)
    assert "type" not in cfg


def test_cfg_typing_rules_and_whitelist(tmp_path):
    p = tmp_path / "x.cfg"
    p.write_text("# comment\n[Directories]\nanything_goes=here\nmodel_out = out dir \n\n[Train]\nbatch_size= 8\nsplit=0.2\nloss= l2 \n"
                 "[Net]\ndecay_rate=0.5\nscale=3\n[Preprocessing]\nlow_res_patch_thresholds=0.85,0.9\nhigh_res_threshold=0.85\nto_rotate=1\nckpt=2,3\n")
    cfg = parseConfig(str(p)[:-4])                       # '.cfg' is appended when missing
    assert cfg["anything_goes"] == "here" and cfg["model_out"] == "out dir"      # first section is not whitelisted
    assert cfg["batch_size"] == 8 and cfg["split"] == 0.2 and cfg["loss"] == "l2"
    assert cfg["low_res_patch_thresholds"] == [0.85, 0.9] and cfg["to_rotate"] is True and cfg["ckpt"] == [2, 3]
    bad = tmp_path / "bad.cfg"
    bad.write_text("[Directories]\nraw_data=x\n[Train]\nbatch_sizes=8\n")
    with pytest.raises(AssertionError, match="Unsupported fields"):
        parseConfig(str(bad))


# ---- pinned by the reference itself: tests/golden/cfg_cases.json holds what /root/reference/utils/parseConfig.py returned (or raised) for
# each cfg text when tests/golden/make_cfg_fixture.py ran it in the build container -- the one piece of the reference that imports here
def _cfg_cases():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "cfg_cases.json")) as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("case", _cfg_cases(), ids=lambda c: c["name"])
def test_parseConfig_matches_the_reference_parser(case, tmp_path):
    import builtins
    p = tmp_path / (case["name"] + ".cfg")
    p.write_text(case["text"])
    if "error" in case:
        with pytest.raises(getattr(builtins, case["error"])):
            parseConfig(str(p))
        return
    got = parseConfig(str(p))
    assert got == case["result"]
    for k, v in case["result"].items():                  # == lets True == 1 and 3 == 3.0 through: the types must agree too
        assert type(got[k]) is type(v), (k, got[k], v)
        if isinstance(v, list):
            assert [type(a) for a in got[k]] == [type(a) for a in v], k


def test_repo_cfgs_equal_the_reference_cfgs_outside_the_directory_paths():
    """cfg/*.cfg of this repo parse to the same dict as the reference's shipped files, except for the site-local [Directories] paths."""
    cases = {c["name"]: c for c in _cfg_cases()}
    for name in ("p16t9c85r12", "p16t12c85r12"):
        ours = parseConfig(os.path.join(ROOT, "cfg", name + ".cfg"))
        ref = cases["shipped_" + name]["result"]
        dirs = {"raw_data", "preprocessing_out", "model_out", "test_out", "train_out"}
        assert set(ours) == set(ref)
        assert {k: v for k, v in ours.items() if k not in dirs} == {k: v for k, v in ref.items() if k not in dirs}


# ---- cfg values beside the shipped ones (tests/cfg_grid.py; held to the oracle on the device by tests/test_gpu_cfg_values.py) -------------------------
def _grid_cases():
    from tests.cfg_grid import GRID, VARIANTS
    return [(row, 9, True) for row, _ in GRID] + [(row, T, gray) for row, T, gray, _ in VARIANTS]


def _grid_id(c):
    from tests.cfg_grid import case_id
    return case_id(*c)


@pytest.mark.parametrize("case", _grid_cases(), ids=_grid_id)
def test_grid_configuration_builds_and_the_tables_agree(built_lib, case):
    """probav_engine_create takes every configuration of the grid (it touches no device), the host's and the native library's layer tables agree -- names,
    offsets, shapes, parameter count --, and the workspace, scratch and weight-cache size queries answer with consistent positive sizes."""
    import ctypes
    from probav_amd import _lib
    from probav_amd.modelsTF import WDSRConv3D
    from tests.cfg_grid import arch_of
    row, T, gray = case
    F, R, E, decay, D = row
    m = WDSRConv3D("t", "NIR", 8075.2045, 3160.7272, 6).build(3, F, (3, 3, 3), R, E, decay, T, 16, gray, seed=0)
    layers, total = layer_table(**arch_of(row, T, gray))
    assert int(F * decay) == D and m.flat.numel() == total and len(m.trainable_variables) == 3 * len(layers)
    nred = len(reducer_plan(T))
    assert len(layers) == 1 + 3 * R + nred + 4
    L, h = _lib.lib(), m._handle()                       # probav_engine_create; raises unless the parameter counts agree
    assert L.probav_param_count(h) == total and L.probav_num_layers(h) == len(layers)
    native = m.native_layer_table()
    nweff = ncout = 0
    for (name, g, v, b, shape), Lh in zip(native, layers):
        vs = Lh.vshape if len(Lh.vshape) == 5 else Lh.vshape[:2] + (1,) + Lh.vshape[2:]          # 2-D layers: [kh, kw, Cin, Cout]
        assert (name, g, v, b, shape) == (Lh.name, Lh.g_off, Lh.v_off, Lh.b_off, vs)
        nweff += Lh.b_off - Lh.v_off
        ncout += Lh.cout
    by_name = {Lh.name: Lh.vshape for Lh in layers}
    C = 1 if gray else 3
    assert by_name["mainConv1"] == (3, 3, 3, C, F) and by_name["upscaleConv1"] == (3, 3, 3, F, 9) and by_name["convReducer_1"][-2:] == (F, F)
    if R:
        assert by_name["expConv_0"] == (1, 1, 1, F, F * E) and by_name["decConv_%d" % (R - 1)] == (1, 1, 1, F * E, D) and by_name["normConv_0"] == (3, 3, 3, D, F)
    assert L.probav_weff_count(h) == nweff and L.probav_cout_total(h) == ncout
    wc = L.probav_weight_cache_bytes(h)
    assert wc >= 4 * (2 * nweff + ncout) and wc % 4 == 0             # both layouts of the effective weights and the inverse norms, at least
    for impl in range(5):
        m.set_impl(impl)
        sizes = {}
        for B in (1, 2, 5):
            infer, train = L.probav_workspace_bytes(h, B, 0), L.probav_workspace_bytes(h, B, 1)
            saved, scratch = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(L.probav_workspace_split(h, B, ctypes.byref(saved), ctypes.byref(scratch)), "probav_workspace_split")
            assert saved.value > 0 and scratch.value > 0 and saved.value + scratch.value == train
            hin = 22
            acts = 4 * B * hin * hin * T * ((R + 1) * F + R * D)     # the saved block inputs and decay outputs of a training pass
            assert infer >= 4 * 2 * nweff and saved.value >= acts + 4 * 2 * nweff
            for kind, idx, count in ((0, R, B * hin * hin * T * F), (3, 0, B * 20 * 20 * 9)) + (((1, R - 1, B * hin * hin * T * D),) if R else ()):
                off, cnt = ctypes.c_int64(), ctypes.c_int64()
                _lib.check(L.probav_workspace_view(h, B, 1, kind, idx, ctypes.byref(off), ctypes.byref(cnt)), "probav_workspace_view")
                assert cnt.value == count and 0 <= off.value and 4 * (off.value + cnt.value) <= saved.value
            off, cnt = ctypes.c_int64(), ctypes.c_int64()
            assert L.probav_workspace_view(h, B, 1, 0, R + 1, ctypes.byref(off), ctypes.byref(cnt)) == _lib.PROBAV_EINVAL
            assert L.probav_workspace_view(h, B, 1, 2, nred, ctypes.byref(off), ctypes.byref(cnt)) == _lib.PROBAV_EINVAL
            sizes[B] = (infer, train)
        assert sizes[1][0] < sizes[2][0] < sizes[5][0] and sizes[1][1] < sizes[2][1] < sizes[5][1]


def test_engine_refuses_what_the_graph_cannot_close_for(built_lib):
    import ctypes
    from probav_amd import _lib
    L = _lib.lib()
    for kw in (dict(num_filters=0), dict(num_res_blocks=-1), dict(exp_rate=0), dict(dec_channels=0), dict(num_img_lr=12), dict(in_channels=2)):
        c = dict(scale=3, num_filters=32, num_res_blocks=12, exp_rate=8, dec_channels=25, num_img_lr=9, patch_size_lr=16, max_shift=6,
                 mean=8075.2045, std=3160.7272, in_channels=1)
        c.update(kw)
        cfg, h = _lib.NetCfg(*[c[f[0]] for f in _lib.NetCfg._fields_]), ctypes.c_void_p()
        assert L.probav_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.PROBAV_EINVAL, kw


def test_backward_filter_predicates_by_channel_count(built_lib):
    """probav_conv3d_wgrad_scratch_bytes answers on the host: which 3x3x3 'same' layers on 22 x 22 x 9 the backward-filter kernels of each family take (0 = declined; the
    engine then runs the direct kernel).  The fp32-MFMA kernel (impl 1) takes 25, 32 or 1 input channels with at most 32 filters, the split-operand kernel (impl 3 / 4) 25 or
    32 input channels with exactly 32 filters -- no channel count beside the shipped ones -- and the direct kernels (impl 0) everything.  tests/test_gpu_parity.py runs a
    case for every 'yes' at a channel count that no shipped layer has."""
    import ctypes
    from probav_amd import _lib
    L = _lib.lib()

    def nbytes(cin, cout, impl):
        g = (ctypes.c_int32 * 17)(2, 22, 22, 9, cin, 22, 22, 9, cout, 3, 3, 3, 1, 1, 1, 0, 0)
        return L.probav_conv3d_wgrad_scratch_bytes(ctypes.byref(g), impl)
    pairs = [(1, 32), (25, 32), (32, 32), (32, 9), (1, 16), (1, 20), (32, 16), (32, 28), (32, 12), (32, 1), (1, 64), (16, 32), (16, 16), (28, 32), (26, 32), (12, 16),
             (48, 48), (64, 64), (51, 64), (20, 20), (10, 20), (32, 64)]
    for cin, cout in pairs:
        assert nbytes(cin, cout, 0) > 0 and nbytes(cin, cout, 2) == nbytes(cin, cout, 0), (cin, cout)
        assert (nbytes(cin, cout, 1) > 0) == (cin in (1, 25, 32) and cout <= 32), (cin, cout)
        assert (nbytes(cin, cout, 3) > 0) == (cin in (25, 32) and cout == 32) and nbytes(cin, cout, 3) == nbytes(cin, cout, 4), (cin, cout)
        for impl in (1, 3):
            n = nbytes(cin, cout, impl)
            assert n % (4 * (27 * cin * cout + cout)) == 0                      # whole slabs of [27 Cin Cout | Cout]
