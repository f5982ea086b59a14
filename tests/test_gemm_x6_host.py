"""The general matrix route on the 16-bit matrix pipe (csrc/kernels_gemm_x6.hip; include/probav_hip.h, 'the route on the 16-bit matrix pipe') on the host: the
built library, no device.

(a) the wish is off by default, PROBAV_GEMM_X6 sets it, probav_engine_set_impl / set_gemm_route / set_gemm_pair keep it, a null engine answers -1 / 0;
(b) probav_engine_gemm_arith is 1 exactly when the family is >= 1, the route is on and the wish is set: 0 at family 0, with the route off, for the wish alone;
(c) no size and no census count moves with the switch: probav_workspace_bytes / probav_workspace_split / probav_engine_route_counts of the shipped and the
    64-filter network at batch 2 and 128, every family, route and pair on or off;
(d) probav_plan_conv_gemm_x6: the tiles cover every output voxel and channel exactly once, the K chunks a tap's channels; it is the fp32 route's plan under
    the x6 kernel's name (test_gpu_gemm_route.EXTRA plus Cin = 17 and Cout = 33); the backward-filter has no x6 kernel and reports none;
(e) --gemm-x6 parses, needs --gemm-route, combines with --gemm-pair and reaches set_gemm_x6; the model methods exist."""
import ctypes
import os

import pytest

from tests import plan_cases as pc
from tests.test_gemm_route_host import _load, make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPLS = (0, 1, 2, 3, 4)
SHIPPED = (32, 12, 8, 25)                   # F, R, E, D
F64 = (64, 12, 8, 51)
GEMM, WGRAD_GEMM, GEMM_X6 = 11, 12, 13


@pytest.fixture(scope="module")
def lib(built_lib):
    from probav_amd import _lib as L
    return L.lib()


def _engine(lib, shape=F64, T=9):
    F, R, E, D = shape
    return make_engine(lib, F, R, E, D, T)


def test_off_by_default_and_who_keeps_the_wish(lib, monkeypatch):
    for name in ("PROBAV_GEMM_X6", "PROBAV_GEMM_ROUTE", "PROBAV_GEMM_PAIR", "PROBAV_IMPL"):
        monkeypatch.delenv(name, raising=False)
    h = _engine(lib)
    try:
        assert lib.probav_engine_gemm_x6(h) == 0 and lib.probav_engine_gemm_arith(h) == 0              # off by default
        assert lib.probav_engine_set_gemm_x6(h, 1) == 0 and lib.probav_engine_gemm_x6(h) == 1
        assert lib.probav_engine_gemm_arith(h) == 0                                                    # the wish alone: no route, fp32 nowhere to change
        for impl in (1, 4, 0, 2):
            assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_gemm_x6(h) == 1
        for route in (1, 0, 1):
            assert lib.probav_engine_set_gemm_route(h, route) == 0 and lib.probav_engine_gemm_x6(h) == 1
            assert lib.probav_engine_gemm_arith(h) == route
        for pair in (1, 0):
            assert lib.probav_engine_set_gemm_pair(h, pair) == 0 and lib.probav_engine_gemm_x6(h) == 1 and lib.probav_engine_gemm_arith(h) == 1
            assert lib.probav_engine_pair_kind(h) == 2 * pair
        assert lib.probav_engine_set_gemm_pair(h, 1) == 0
        assert lib.probav_engine_set_gemm_x6(h, 0) == 0 and lib.probav_engine_gemm_x6(h) == 0 and lib.probav_engine_gemm_arith(h) == 0
        assert lib.probav_engine_gemm_route(h) == 1 and lib.probav_engine_gemm_pair(h) == 1              # ... and its setter keeps the other two
    finally:
        lib.probav_engine_destroy(h)
    assert lib.probav_engine_set_gemm_x6(None, 1) == -1 and lib.probav_engine_gemm_x6(None) == 0 and lib.probav_engine_gemm_arith(None) == 0
    for value, want in (("1", 1), ("0", 0), ("7", 1), ("", 0)):
        monkeypatch.setenv("PROBAV_GEMM_X6", value)
        h = _engine(lib)
        assert lib.probav_engine_gemm_x6(h) == want and lib.probav_engine_gemm_route(h) == 0 and lib.probav_engine_gemm_arith(h) == 0, value
        lib.probav_engine_destroy(h)
    monkeypatch.setenv("PROBAV_GEMM_ROUTE", "1")
    monkeypatch.setenv("PROBAV_GEMM_X6", "1")
    h = _engine(lib)
    assert lib.probav_engine_gemm_arith(h) == 1 and lib.probav_engine_pair_kind(h) == 0                 # the default family, both from the environment
    lib.probav_engine_destroy(h)
    assert lib.probav_abi_version() == 7


def _set(lib, h, impl, route, pair, x6):
    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, route) == 0
    assert lib.probav_engine_set_gemm_pair(h, pair) == 0 and lib.probav_engine_set_gemm_x6(h, x6) == 0


@pytest.mark.parametrize("shape", [F64, SHIPPED], ids=["f64", "shipped"])
def test_gemm_arith(lib, shape):
    h = _engine(lib, shape)
    try:
        for impl in IMPLS:
            for route in (0, 1):
                for pair in (0, 1):
                    for x6 in (0, 1):
                        _set(lib, h, impl, route, pair, x6)
                        assert lib.probav_engine_gemm_arith(h) == (1 if impl >= 1 and route and x6 else 0), (impl, route, pair, x6)
                        assert lib.probav_engine_gemm_x6(h) == x6
    finally:
        lib.probav_engine_destroy(h)


def _state(lib, h):
    out = []
    for b in (2, 128):
        out += [int(lib.probav_workspace_bytes(h, b, t)) for t in (0, 1)]
        saved, scr = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.probav_workspace_split(h, b, ctypes.byref(saved), ctypes.byref(scr)) == 0
        c = (ctypes.c_int32 * 4)()
        assert lib.probav_engine_route_counts(h, b, ctypes.byref(c)) == 0
        out += [int(saved.value), int(scr.value)] + list(c)
    assert min(out[:4]) > 0
    return out


@pytest.mark.parametrize("shape", [F64, SHIPPED], ids=["f64", "shipped"])
def test_no_size_and_no_count_moves_with_the_switch(lib, shape):
    h = _engine(lib, shape)
    try:
        n_on = 0
        for impl in IMPLS:
            for route in (0, 1):
                for pair in (0, 1):
                    _set(lib, h, impl, route, pair, 0)
                    off = _state(lib, h)
                    _set(lib, h, impl, route, pair, 1)
                    n_on += lib.probav_engine_gemm_arith(h)
                    assert _state(lib, h) == off, (shape, impl, route, pair)
        assert n_on == 4 * 2
        if shape == F64:                                                # the launches that change hands are there to be counted: slots 1 and 3
            _set(lib, h, 4, 1, 0, 1)
            c = (ctypes.c_int32 * 4)()
            assert lib.probav_engine_route_counts(h, 128, ctypes.byref(c)) == 0
            assert c[0] == 0 and c[2] == 0 and c[1] > 0 and c[3] > 0, tuple(c)
    finally:
        lib.probav_engine_destroy(h)


def _plan_rows():
    """(name, N, (Hi, Wi, Ti), Cin, Cout, k, pad, reflect, relu, gate, skip): the hazard rows of the fp32 route's device tests, and the two counts one past a tile."""
    from tests.test_gpu_gemm_route import EXTRA
    return EXTRA + [("gemm x6: same 17->20 (one channel into the second K chunk)", 2, (6, 5, 3), 17, 20, (3, 3, 3), (1, 1, 1), 0, 1, 0, 0),
                    ("gemm x6: 1x1x1 20->33 (one channel into the second N tile)", 2, (6, 5, 9), 20, 33, (1, 1, 1), (0, 0, 0), 0, 0, 1, 1),
                    ("gemm x6: same 65->65, 2 x 1089 voxels (two tiles each way, three slabs)", 2, (11, 11, 9), 65, 65, (3, 3, 3), (1, 1, 1), 0, 0, 0, 0)]


def _report(lib, fn, g, gate, skip, op, impl=None):
    rep = (ctypes.c_int32 * 8)()
    args = [ctypes.byref(g)] + ([impl] if impl is not None else []) + [int(bool(gate)), int(bool(skip)), pc.OPS[op], ctypes.byref(rep)]
    assert getattr(lib, fn)(*args) == 0
    return list(rep)


def test_plan_covers_the_problem_once(lib):
    seen_n_tiles = False
    for name, N, hwt, Cin, Cout, k, pad, reflect, relu, gate, skip in _plan_rows():
        g = pc.geom(N, hwt, Cin, Cout, pad, reflect, relu, k)
        ho = tuple(hwt[i] + 2 * pad[i] - k[i] + 1 for i in range(3))
        nvox, taps = N * ho[0] * ho[1] * ho[2], k[0] * k[1] * k[2]
        for op in ("fwd", "bwd"):
            rep = kern, ntn, ntm, tm, tn, grid, kc, chunks = _report(lib, "probav_plan_conv_gemm_x6", g, gate, skip, op)
            assert kern == GEMM_X6, (name, rep)
            assert tm == 128 and tn in (32, 64, 128) and kc == 16 and grid == ntn * ntm
            assert (ntm - 1) * tm < nvox <= ntm * tm, (name, rep)                # the voxel tiles cover M once, none is empty
            assert (ntn - 1) * tn < Cout <= ntn * tn, (name, rep)                # ... and the channel tiles N
            assert (chunks - 1) * kc < Cin <= chunks * kc, (name, rep)            # the K chunks cover a tap's channels
            assert rep == _report(lib, "probav_plan_conv_gemm_x6", g, not gate, not skip, op)      # one plan for every operand set
            seen_n_tiles |= ntn > 1
            # the fp32 route's launch of the same geometry: the same integers (an engine's launch that the route takes; others answer another kernel there)
            fp32 = _report(lib, "probav_plan_conv_gemm", g, gate, skip, op, 1)
            if fp32[0] == GEMM:
                assert fp32[1:] == rep[1:], (name, fp32, rep)
        # the backward-filter stays the fp32 route's: no x6 kernel, whatever the geometry -- and the fp32 plan of the same geometry is still reported where it was
        assert _report(lib, "probav_plan_conv_gemm_x6", g, relu, 0, "wgrad") == [0] * 8, name
        if max(pad) <= 1:
            assert _report(lib, "probav_plan_conv_gemm", g, relu, 0, "wgrad", 1)[0] in (WGRAD_GEMM, 6, 10), name
    assert seen_n_tiles
    from probav_amd import _lib as L
    g5 = pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 2), 0, 0, (5, 5, 5))
    assert _report(lib, "probav_plan_conv_gemm_x6", g5, 0, 0, "fwd") == [0] * 8 and _report(lib, "probav_plan_conv_gemm_x6", g5, 0, 0, "wgrad") == [0] * 8
    rep = (ctypes.c_int32 * 8)()
    assert lib.probav_plan_conv_gemm_x6(None, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv_gemm_x6(ctypes.byref(g5), 0, 0, 3, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv_gemm_x6(ctypes.byref(g5), 0, 0, 0, None) == L.PROBAV_EINVAL


class _Stub:
    def __init__(self):
        self.calls = []

    def set_gemm_route(self, on):
        self.calls.append(("route", on))

    def set_gemm_pair(self, on):
        self.calls.append(("pair", on))

    def set_gemm_x6(self, on):
        self.calls.append(("x6", on))


def test_the_flags_parse_and_reach_the_model(built_lib, monkeypatch):
    from probav_amd import inference
    cfg = os.path.join(ROOT, "cfg", "p16t9c85r12f64.cfg")
    train_py, test_py, evaluate_py = _load("train"), _load("test"), _load("evaluate")
    both, three = ["--gemm-route", "--gemm-x6"], ["--gemm-route", "--gemm-pair", "--gemm-x6"]
    for parse, base in ((train_py.parser, ["--cfg", cfg]), (test_py.parser, ["--cfg", cfg]), (evaluate_py.parser, ["--cfg", cfg, "--model"])):
        assert parse(base).gemm_x6 is False and parse(base + ["--gemm-route"]).gemm_x6 is False and parse(base + ["--gemm-route", "--gemm-pair"]).gemm_x6 is False
        assert parse(base + both).gemm_x6 is True and parse(base + both).gemm_pair is False
        opt = parse(base + three)
        assert opt.gemm_x6 is True and opt.gemm_pair is True and opt.gemm_route is True          # it combines freely with the pair
        with pytest.raises(SystemExit):
            parse(base + ["--gemm-x6"])                                           # the switch is the route's: alone it is an error
        with pytest.raises(SystemExit):
            parse(base + ["--gemm-pair", "--gemm-x6"])
    with pytest.raises(SystemExit):
        train_py.parser(["--cfg", cfg, "--modelType", "fusionNet", "--fusion-input", ROOT] + both)
    with pytest.raises(SystemExit):
        evaluate_py.parser(["--cfg", cfg, "--toCompare", ROOT] + both)
    for argv, want in ((["--cfg", cfg], []), (["--cfg", cfg, "--gemm-route"], [("route", True)]), (["--cfg", cfg] + both, [("route", True), ("x6", True)]),
                       (["--cfg", cfg] + three, [("route", True), ("pair", True), ("x6", True)])):
        stub = _Stub()
        train_py.apply_engine_options(stub, train_py.parser(argv))
        assert stub.calls == want
    assert test_py.parser(["--cfg", cfg] + both).inference == inference.InferenceOptions()            # a switch of the engine, no option of the prediction
    import probav_amd.modelsTF as modelsTF
    import probav_amd.trainClass as trainClass
    stub = _Stub()
    stub.to = lambda dev: stub

    class Builder:
        def __init__(self, **kw):
            pass

        def build(self, **kw):
            return stub

    monkeypatch.setattr(modelsTF, "WDSRConv3D", Builder)
    monkeypatch.setattr(trainClass, "ModelTrainer", lambda *a, **kw: "trainer")
    from probav_amd.parseConfig import parseConfig
    config = parseConfig(cfg)
    assert inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_x6=True) == (stub, "trainer")
    assert stub.calls == [("route", True), ("x6", True)]
    stub.calls.clear()
    inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_pair=True, gemm_x6=True)
    assert stub.calls == [("route", True), ("pair", True), ("x6", True)]
    stub.calls.clear()
    inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_pair=True)
    assert stub.calls == [("route", True), ("pair", True)]


def test_model_methods_exist():
    from probav_amd.modelsTF import WDSRModel
    assert callable(WDSRModel.set_gemm_x6) and isinstance(WDSRModel.gemm_x6, property)
