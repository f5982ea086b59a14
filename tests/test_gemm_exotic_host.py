"""The general matrix route's exotic launches (include/probav_hip.h, 'the route's exotic launches'; csrc/engine.hip: conv_route / wgrad_route, csrc/kernels_gemm.h:
the wide predicates) on the host: the built library, no device.

(a) switch off: probav_engine_route_counts and probav_workspace_bytes answer what they answered before the switch existed -- tests/golden/gemm_exotic_parent.json holds
    them for T in {7, 9, 13, 19}, 32 and 64 filters, impl 0..4, the route off and on, batch 2 and 128, generated on the commit before it by parent_census() below;
(b) switch on, route on, 19 frames: no launch is left on the generic direct kernels -- exactly five convolution and four backward-filter launches change hands; any
    other engine, family 0 and an engine with the route off are untouched;
(c) the plans of the wide geometries tile the problem exactly once, the backward-filter's scratch is slabs x 4 x (taps Cin Cout + Cout) bytes with 1 <= slabs <= 32,
    whatever is outside the wide predicates is refused, and the old entry points still refuse what they refused;
(d) the wish survives the other setters, PROBAV_GEMM_EXOTIC sets it at creation, --gemm-exotic parses on the three CLIs, needs --gemm-route and reaches
    set_gemm_exotic."""
import ctypes
import json
import os

import pytest

from tests import plan_cases as pc
from tests.test_gemm_route_host import _counts, _load, make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_exotic_parent.json")
FRAMES = (7, 9, 13, 19)
CHANNELS = ((32, 25), (64, 51))             # (num_filters, channels behind the decay convolution): the shipped counts and the 64-filter network's
IMPLS = (0, 1, 2, 3, 4)
BATCHES = (2, 128)
GEMM, WGRAD_GEMM, GEMM_X6 = 11, 12, 13


def _key(T, F, impl, route, batch):
    return "T%d F%d impl%d route%d B%d" % (T, F, impl, route, batch)


def parent_census(lib):
    """What the fixture holds: {key: [the four route counts, workspace bytes for inference, for training]}.  Run on the commit BEFORE the switch (any library
    that exports probav_engine_create, probav_engine_set_impl, probav_engine_set_gemm_route, probav_engine_route_counts and probav_workspace_bytes)."""
    out = {}
    for T in FRAMES:
        for F, D in CHANNELS:
            h = make_engine(lib, F, 12, 8, D, T)
            for impl in IMPLS:
                for route in (0, 1):
                    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, route) == 0
                    for batch in BATCHES:
                        out[_key(T, F, impl, route, batch)] = [list(_counts(lib, h, batch)), int(lib.probav_workspace_bytes(h, batch, 0)),
                                                               int(lib.probav_workspace_bytes(h, batch, 1))]
            lib.probav_engine_destroy(h)
    return out


@pytest.fixture(scope="module")
def lib(built_lib):
    from probav_amd import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(autouse=True)
def _no_switches_in_the_environment(monkeypatch):
    for name in ("PROBAV_GEMM_EXOTIC", "PROBAV_GEMM_X6", "PROBAV_GEMM_ROUTE", "PROBAV_GEMM_PAIR", "PROBAV_IMPL"):
        monkeypatch.delenv(name, raising=False)


def test_switch_off_the_census_and_the_sizes_are_the_parents(lib, parent):
    h = make_engine(lib, 32, 1, 8, 25, 19)
    assert lib.probav_engine_gemm_exotic(h) == 0                                                # off by default
    lib.probav_engine_destroy(h)
    now = parent_census(lib)
    assert set(now) == set(parent) and len(parent) == len(FRAMES) * len(CHANNELS) * len(IMPLS) * 2 * len(BATCHES)
    for key, was in parent.items():
        assert now[key] == was, key
    assert parent[_key(19, 64, 4, 1, 2)][0] == [5, 101, 4, 44]                                  # the row the switch exists for


def _state(lib, h, batch):
    split = (ctypes.c_size_t(), ctypes.c_size_t())
    assert lib.probav_workspace_split(h, batch, ctypes.byref(split[0]), ctypes.byref(split[1])) == 0
    return (_counts(lib, h, batch), lib.probav_workspace_bytes(h, batch, 0), lib.probav_workspace_bytes(h, batch, 1), split[0].value, split[1].value)


@pytest.mark.parametrize("F,D", CHANNELS)
def test_switch_on_nineteen_frames_leave_the_direct_kernels(lib, F, D):
    h = make_engine(lib, F, 12, 8, D, 19)
    try:
        assert lib.probav_engine_set_gemm_route(h, 1) == 0
        for impl in (1, 2, 3, 4):
            assert lib.probav_engine_set_impl(h, impl) == 0
            for pair, x6 in ((0, 0), (1, 1)):
                assert lib.probav_engine_set_gemm_pair(h, pair) == 0 and lib.probav_engine_set_gemm_x6(h, x6) == 0
                assert lib.probav_engine_set_gemm_exotic(h, 0) == 0
                off, ws_off = _counts(lib, h), _state(lib, h, 64)
                assert lib.probav_engine_set_gemm_exotic(h, 1) == 0 and lib.probav_engine_gemm_exotic(h) == 1
                on, ws_on = _counts(lib, h), _state(lib, h, 64)
                print("%d filters, 19 frames, impl %d, pair %d x6 %d: off %s on %s; workspace at batch 64: %d -> %d bytes" % (F, impl, pair, x6, off, on, ws_off[2], ws_on[2]))
                assert on[0] == 0 and on[2] == 0, on
                assert on[0] + on[1] == off[0] + off[1] and on[2] + on[3] == off[2] + off[3]      # the same launches, other hands
                assert off[0] - on[0] == 5 and off[2] - on[2] == 4, (off, on)                      # reducers 1-4 each way, and the 5x5x5 layer's backward-data
                assert _counts(lib, h, 128) == on                                                   # (the batch size moves nothing)
                assert ws_on[1] == ws_off[1] and ws_on[3] == ws_off[3]                              # inference and the saved state: no slab regions
                assert ws_on[2] != ws_off[2] and ws_on[4] != ws_off[4]                              # the reverse scratch: four slab regions of another size
        # family 0 never sees the switch; with the route off it does nothing
        assert lib.probav_engine_set_gemm_pair(h, 0) == 0 and lib.probav_engine_set_gemm_x6(h, 0) == 0
        for impl, route in ((0, 1), (0, 0), (1, 0), (4, 0)):
            assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, route) == 0
            assert lib.probav_engine_set_gemm_exotic(h, 0) == 0
            off = _state(lib, h, 2)
            assert lib.probav_engine_set_gemm_exotic(h, 1) == 0
            assert _state(lib, h, 2) == off and off[0][1] == 0 and off[0][3] == 0, (impl, route)
    finally:
        lib.probav_engine_destroy(h)


@pytest.mark.parametrize("T", [7, 9, 13])
def test_switch_on_other_frame_counts_do_not_move(lib, parent, T):
    for F, D in CHANNELS:
        h = make_engine(lib, F, 12, 8, D, T)
        try:
            assert lib.probav_engine_set_gemm_exotic(h, 1) == 0
            for impl in IMPLS:
                for route in (0, 1):
                    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, route) == 0
                    for batch in BATCHES:
                        got = [list(_counts(lib, h, batch)), lib.probav_workspace_bytes(h, batch, 0), lib.probav_workspace_bytes(h, batch, 1)]
                        assert got == parent[_key(T, F, impl, route, batch)], (T, F, impl, route, batch)
        finally:
            lib.probav_engine_destroy(h)


def reducer_geometries(row, T, gray, B, P):
    """(name, N, (Hi, Wi, Ti), Cin, Cout, pad, reflect_hw, reflect_t, k) of the launches the switch moves, on the 19-frame engine of a row of
    tests/test_gpu_gemm_exotic.py: forward (= backward-filter) geometry of reducers 1-4, and the backward-data of the 5x5x5 layer."""
    F = row[0]
    assert T == 19
    h, t, out = P + 6, T, []
    for i, (k, p, pt, rt) in enumerate(((5, 2, 2, 1), (3, 2, 1, 1), (3, 2, 0, 0), (3, 2, 0, 0))):
        out.append(("F%d B%d P%d reducer %d" % (F, B, P, i + 1), B, (h, h, t), F, F, (p, p, pt), 1, rt, (k, k, k)))
        h, t = h + 2 * p - k + 1, t + 2 * pt - k + 1
    out.append(("F%d B%d P%d bwd-data of reducer 1" % (F, B, P), B, (P + 6, P + 6, T), F, F, (4, 4, 4), 0, 0, (5, 5, 5)))
    return out


ROWS = {"A": ((9, 1, 2, 0.7, 6), 19, True, 3, 4), "B": ((40, 1, 2, 0.8, 32), 19, True, 2, 4), "C": ((72, 1, 2, 0.8, 57), 19, False, 1, 4),
        "D": ((32, 1, 8, 0.8, 25), 19, True, 2, 16)}


def _wide(lib, g, reflect_t, x6, op):
    rep = (ctypes.c_int32 * 8)()
    assert lib.probav_plan_conv_gemm_wide(ctypes.byref(g), reflect_t, x6, pc.OPS[op], ctypes.byref(rep)) == 0
    return list(rep)


def test_plans_of_the_wide_geometries(lib):
    seen_slabs, seen_tn, seen_tail = set(), set(), False
    for row in ROWS.values():
        for name, N, hwt, Cin, Cout, pad, refl, rt, k in reducer_geometries(*row):
            g = pc.geom(N, hwt, Cin, Cout, pad, refl, 1, k)
            ho = tuple(hwt[i] + 2 * pad[i] - k[i] + 1 for i in range(3))
            nvox, taps = N * ho[0] * ho[1] * ho[2], k[0] * k[1] * k[2]
            for x6 in (0, 1):
                rep = kern, ntn, ntm, tm, tn, grid, kc, chunks = _wide(lib, g, rt, x6, "bwd" if max(pad) == 4 else "fwd")
                assert kern == (GEMM_X6 if x6 else GEMM), (name, rep)
                assert grid == ntn * ntm and tm > 0 and tn > 0
                assert (ntm - 1) * tm < nvox <= ntm * tm, (name, rep, nvox)                         # the voxel tiles cover M once, none is empty
                assert (ntn - 1) * tn < Cout <= ntn * tn, (name, rep)                               # ... and the channel tiles N
                assert (chunks - 1) * kc < Cin <= chunks * kc, (name, rep)                          # the K chunks cover a tap's channels
                assert rep == _wide(lib, g, rt, x6, "fwd")                                          # twice the same; the operator's name decides nothing
                assert rep[1:] == _wide(lib, g, rt, 1 - x6, "fwd")[1:]                              # one report for both arithmetics
                seen_tn.add(tn)
                seen_tail |= nvox % tm != 0
            rep = _wide(lib, g, rt, 0, "wgrad")
            nbytes = lib.probav_gemm_wgrad_wide_scratch_bytes(ctypes.byref(g), rt)
            if max(pad) == 4:                                                                       # the backward-filter takes pads up to 2
                assert rep == [0] * 8 and nbytes == 0, (name, rep)
                continue
            kern, slabs, vps, tci, tco, grid = rep[:6]
            assert kern == WGRAD_GEMM, (name, rep)
            assert nbytes == slabs * 4 * (taps * Cin * Cout + Cout), (name, rep, nbytes)
            assert (slabs - 1) * vps < nvox <= slabs * vps and 1 <= slabs <= 32, (name, rep)       # the slabs cover the voxels once, none is empty
            assert grid == slabs * taps * -(-Cin // tci) * -(-Cout // tco)
            assert rep == _wide(lib, g, rt, 0, "wgrad") == _wide(lib, g, rt, 1, "wgrad")            # twice the same; fp32 whatever the arithmetic
            seen_slabs.add(slabs)
            # the old entry points still refuse these: no plan, no scratch
            assert lib.probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(g)) == 0, name
            for impl in (1, 2, 3, 4):
                old = (ctypes.c_int32 * 8)()
                assert lib.probav_plan_conv_gemm(ctypes.byref(g), impl, 1, 0, pc.OPS["wgrad"], ctypes.byref(old)) == 0
                assert old[0] != WGRAD_GEMM, (name, impl)
            if k == (5, 5, 5):
                old = (ctypes.c_int32 * 8)()
                assert lib.probav_plan_conv_gemm_x6(ctypes.byref(g), 0, 0, 0, ctypes.byref(old)) == 0 and list(old) == [0] * 8
    assert len(seen_slabs) > 1 and max(seen_slabs) > 1 and seen_tn == {32, 64, 128} and seen_tail
    # the slab count is a function of the voxel count alone: not of the taps, the channels or the pads
    a = _wide(lib, pc.geom(2, (9, 9, 19), 8, 8, (2, 2, 2), 1, 1, (5, 5, 5)), 1, 0, "wgrad")
    b = _wide(lib, pc.geom(2, (11, 11, 21), 72, 40, (0, 0, 0), 0, 1, (3, 3, 3)), 0, 0, "wgrad")
    assert a[1] == b[1] and a[2] == b[2] and a[1] > 1


def test_what_the_wide_predicates_refuse(lib):
    def refused(g, rt=0):
        return (all(_wide(lib, g, rt, x6, op) == [0] * 8 for x6 in (0, 1) for op in ("fwd", "bwd", "wgrad"))
                and lib.probav_gemm_wgrad_wide_scratch_bytes(ctypes.byref(g), rt) == 0)

    def taken(g, rt=0, wgrad=True):
        return _wide(lib, g, rt, 0, "fwd")[0] == GEMM and _wide(lib, g, rt, 1, "fwd")[0] == GEMM_X6 and (_wide(lib, g, rt, 0, "wgrad")[0] == WGRAD_GEMM) == wgrad

    assert refused(pc.geom(1, (12, 12, 12), 8, 8, (3, 3, 3), 0, 0, (7, 7, 7)))                      # k = 7
    assert refused(pc.geom(1, (12, 12, 12), 8, 8, (3, 3, 3), 0, 0, (3, 3, 3)))                      # a pad above k - 1
    assert refused(pc.geom(1, (12, 12, 12), 8, 8, (1, 1, 1), 0, 0, (1, 1, 1)))
    assert refused(pc.geom(1, (12, 12, 12), 8, 8, (2, 2, 1), 0, 0, (5, 5, 1)))                      # ... on the depth of a k x k x 1
    assert refused(pc.geom(1, (2, 9, 9), 8, 8, (2, 2, 2), 1, 0, (5, 5, 5)))                          # a mirrored pad that is not below its extent
    assert refused(pc.geom(1, (9, 2, 9), 8, 8, (2, 2, 2), 1, 0, (5, 5, 5)))
    assert refused(pc.geom(1, (9, 9, 2), 8, 8, (2, 2, 2), 1, 0, (5, 5, 5)), rt=1)
    assert refused(pc.geom(1, (9, 9, 9), 8, 8, (3, 3, 2), 1, 0, (5, 5, 5)))                          # a mirrored pad of 3
    assert refused(pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 3), 0, 0, (5, 5, 5)), rt=1)
    assert refused(pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 2), 0, 0, (5, 3, 5)))                          # not k x k x k or k x k x 1
    g = pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 2), 0, 0, (5, 5, 5))
    g[5] += 1                                                                                         # output extents that do not follow from the input's
    assert refused(g)
    assert taken(pc.geom(1, (9, 9, 2), 8, 8, (2, 2, 2), 1, 0, (5, 5, 5)))                            # the same depth pad, not mirrored: a zero pad
    assert taken(pc.geom(1, (3, 3, 3), 8, 8, (2, 2, 2), 1, 0, (5, 5, 5)), rt=1)                      # extent 3 > pad 2
    assert taken(pc.geom(1, (9, 9, 9), 8, 8, (4, 4, 4), 0, 0, (5, 5, 5)), wgrad=False)               # pads of 4 at k = 5: the convolution alone
    assert taken(pc.geom(1, (9, 9, 9), 8, 8, (3, 3, 0), 0, 0, (5, 5, 1)), wgrad=False)
    assert taken(pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 0), 1, 0, (5, 5, 1)))
    rep = (ctypes.c_int32 * 8)()
    from probav_amd import _lib as L
    assert lib.probav_plan_conv_gemm_wide(None, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv_gemm_wide(ctypes.byref(g), 0, 0, 3, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv_gemm_wide(ctypes.byref(g), 0, 0, 0, None) == L.PROBAV_EINVAL
    assert lib.probav_gemm_wgrad_wide_scratch_bytes(None, 0) == 0


def test_the_wish_survives_the_other_setters_and_the_environment_sets_it(lib, monkeypatch):
    h = make_engine(lib, 64, 2, 8, 51, 19)
    try:
        assert lib.probav_engine_gemm_exotic(h) == 0                                            # off by default
        assert lib.probav_engine_set_gemm_exotic(h, 1) == 0 and lib.probav_engine_gemm_exotic(h) == 1
        assert _counts(lib, h)[1] == 0                                                          # the wish alone: the route is off
        for impl in (4, 0, 2, 1):
            assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_gemm_exotic(h) == 1
        for route in (1, 0, 1):
            assert lib.probav_engine_set_gemm_route(h, route) == 0 and lib.probav_engine_gemm_exotic(h) == 1
        for pair in (1, 0):
            assert lib.probav_engine_set_gemm_pair(h, pair) == 0 and lib.probav_engine_gemm_exotic(h) == 1
        for x6 in (1, 0):
            assert lib.probav_engine_set_gemm_x6(h, x6) == 0 and lib.probav_engine_gemm_exotic(h) == 1
        assert _counts(lib, h)[0] == 0 and _counts(lib, h)[2] == 0                               # it took effect with the route
        assert lib.probav_engine_set_gemm_exotic(h, 0) == 0 and lib.probav_engine_gemm_exotic(h) == 0
        assert _counts(lib, h)[0] == 5 and _counts(lib, h)[2] == 4
        assert lib.probav_engine_gemm_route(h) == 1 and lib.probav_engine_gemm_pair(h) == 0 and lib.probav_engine_gemm_x6(h) == 0      # it keeps theirs
    finally:
        lib.probav_engine_destroy(h)
    assert lib.probav_engine_set_gemm_exotic(None, 1) == -1 and lib.probav_engine_gemm_exotic(None) == 0
    for value, want in (("1", 1), ("0", 0), ("7", 1), ("", 0)):
        monkeypatch.setenv("PROBAV_GEMM_EXOTIC", value)
        h = make_engine(lib, 64, 2, 8, 51, 19)
        assert lib.probav_engine_gemm_exotic(h) == want and lib.probav_engine_gemm_route(h) == 0, value
        lib.probav_engine_destroy(h)
    monkeypatch.setenv("PROBAV_GEMM_EXOTIC", "1")
    monkeypatch.setenv("PROBAV_GEMM_ROUTE", "1")
    h = make_engine(lib, 64, 2, 8, 51, 19)
    assert lib.probav_engine_gemm_exotic(h) == 1 and _counts(lib, h)[0] == 0 and _counts(lib, h)[2] == 0
    lib.probav_engine_destroy(h)


class _Stub:
    def __init__(self):
        self.calls = []

    def set_gemm_route(self, on):
        self.calls.append(("route", on))

    def set_gemm_pair(self, on):
        self.calls.append(("pair", on))

    def set_gemm_x6(self, on):
        self.calls.append(("x6", on))

    def set_gemm_exotic(self, on):
        self.calls.append(("exotic", on))


def test_the_flag_parses_and_reaches_the_model(built_lib, monkeypatch):
    from probav_amd import inference
    cfg = os.path.join(ROOT, "cfg", "p16t9c85r12f64.cfg")
    train_py, test_py, evaluate_py = _load("train"), _load("test"), _load("evaluate")
    two, four = ["--gemm-route", "--gemm-exotic"], ["--gemm-route", "--gemm-pair", "--gemm-x6", "--gemm-exotic"]
    for parse, base in ((train_py.parser, ["--cfg", cfg]), (test_py.parser, ["--cfg", cfg]), (evaluate_py.parser, ["--cfg", cfg, "--model"])):
        assert parse(base).gemm_exotic is False and parse(base + ["--gemm-route", "--gemm-pair", "--gemm-x6"]).gemm_exotic is False
        opt = parse(base + two)
        assert opt.gemm_exotic is True and opt.gemm_pair is False and opt.gemm_x6 is False
        opt = parse(base + four)
        assert opt.gemm_exotic is True and opt.gemm_pair is True and opt.gemm_x6 is True and opt.gemm_route is True      # it combines freely
        with pytest.raises(SystemExit):
            parse(base + ["--gemm-exotic"])                                       # the switch is the route's: alone it is an error
    with pytest.raises(SystemExit):
        train_py.parser(["--cfg", cfg, "--modelType", "fusionNet", "--fusion-input", ROOT] + two)
    with pytest.raises(SystemExit):
        evaluate_py.parser(["--cfg", cfg, "--toCompare", ROOT] + two)
    for argv, want in ((["--cfg", cfg], []), (["--cfg", cfg] + two, [("route", True), ("exotic", True)]),
                       (["--cfg", cfg] + four, [("route", True), ("pair", True), ("x6", True), ("exotic", True)])):
        stub = _Stub()
        train_py.apply_engine_options(stub, train_py.parser(argv))
        assert stub.calls == want
    assert test_py.parser(["--cfg", cfg] + two).inference == inference.InferenceOptions()            # a switch of the engine, no option of the prediction
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
    assert inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_exotic=True) == (stub, "trainer")
    assert stub.calls == [("route", True), ("exotic", True)]
    stub.calls.clear()
    inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_pair=True, gemm_x6=True, gemm_exotic=True)
    assert stub.calls == [("route", True), ("pair", True), ("x6", True), ("exotic", True)]
    stub.calls.clear()
    inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_x6=True)
    assert stub.calls == [("route", True), ("x6", True)]


def test_model_methods_exist():
    from probav_amd.modelsTF import WDSRModel
    assert callable(WDSRModel.set_gemm_exotic) and isinstance(WDSRModel.gemm_exotic, property)
