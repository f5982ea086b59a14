"""The general matrix route (csrc/kernels_gemm.hip; include/probav_hip.h, 'the general matrix route') on the host: the built library, no device.

(a) switch off: probav_plan_conv and probav_workspace_bytes answer what they answered before the route existed -- tests/golden/gemm_route_parent_plans.json holds
    the reports of the commit before it (every row of test_gpu_parity.CONV_CASES and plan_cases.CONV_ROWS, impl 0..4, the three operators; the shipped engine's
    workspace sizes), generated there by parent_reports() below;
(b) switch on: probav_plan_conv_gemm hands to the route exactly the launches an engine of that family runs on the generic direct kernel on an ordinary geometry, and
    equals probav_plan_conv everywhere else;
(c) the integers of the route's plans tile the problem exactly once, and the backward-filter's slab count is a function of the geometry alone;
(d) probav_engine_route_counts: a 64-filter engine has no launch left on the VALU kernels with the switch on (19 frames: only the exotic reducers), the shipped engine
    launches what it launched;
(e) probav_engine_set_impl keeps the switch, PROBAV_GEMM_ROUTE sets it at creation; --gemm-route parses and reaches set_gemm_route; cfg/p16t9c85r12f64.cfg."""
import ctypes
import importlib.util
import json
import os

import pytest

from tests import plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_route_parent_plans.json")
OPS = ("fwd", "bwd", "wgrad")
IMPLS = (0, 1, 2, 3, 4)
NONE, DIRECT, GEMM, WGRAD_GEMM = 0, 6, 11, 12
SHIPPED = (32, 12, 8, 25, 9, 1)           # F, R, E, D, T, input channels
WS_CASES = [(impl, batch, training) for impl in IMPLS for batch in (1, 2, 128) for training in (0, 1)]


def rows():
    """(name, N, (Hi, Wi, Ti), Cin, Cout, pad, reflect, relu, gate, skip, k) of both tables."""
    from tests.test_gpu_parity import CONV_CASES
    out = [(c[0], c[1], c[2], c[3], c[4], c[6], c[7], c[8], c[9], c[10], c[5]) for c in CONV_CASES] + [r[:10] + (pc.K3,) for r in pc.CONV_ROWS]
    assert len({r[0] for r in out}) == len(out)
    return out


def _geom(row):
    return pc.geom(row[1], row[2], row[3], row[4], row[5], row[6], row[7], row[10])


def report(lib, fn, row, op, impl):
    """probav_plan_conv / probav_plan_conv_gemm of a row as the operator `op` is launched: [8 ints]."""
    gated = row[7] if op == "wgrad" else row[8]
    rep = (ctypes.c_int32 * 8)()
    rc = getattr(lib, fn)(ctypes.byref(_geom(row)), impl, int(bool(gated)), int(bool(row[9])), pc.OPS[op], ctypes.byref(rep))
    assert rc == 0, (fn, row[0], op, impl, rc)
    return list(rep)


def make_engine(lib, F, R, E, D, T, C=1, P=16):
    from probav_amd import _lib as L
    cfg = L.NetCfg(3, F, R, E, D, T, P, 6, 0.0, 1.0, C)
    h = ctypes.c_void_p()
    assert lib.probav_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def parent_reports(lib):
    """What the fixture holds.  Run on the commit BEFORE the route (any library that exports probav_plan_conv, probav_engine_create, probav_engine_set_impl and
    probav_workspace_bytes with their argument types set)."""
    plans = {r[0]: [report(lib, "probav_plan_conv", r, op, impl) for op in OPS for impl in IMPLS] for r in rows()}
    h = make_engine(lib, *SHIPPED)
    ws = []
    for impl, batch, training in WS_CASES:
        assert lib.probav_engine_set_impl(h, impl) == 0
        ws.append(int(lib.probav_workspace_bytes(h, batch, training)))
    lib.probav_engine_destroy(h)
    return {"plan_conv": plans, "workspace_bytes": ws}


@pytest.fixture(scope="module")
def lib(built_lib):
    from probav_amd import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as fh:
        return json.load(fh)


def _parent(parent, row, op, impl):
    return parent["plan_conv"][row[0]][OPS.index(op) * len(IMPLS) + impl]


def test_switch_off_every_plan_is_the_parents(lib, parent):
    now = parent_reports(lib)
    assert set(now["plan_conv"]) == set(parent["plan_conv"])
    for name, reps in parent["plan_conv"].items():
        assert now["plan_conv"][name] == reps, name
    assert now["workspace_bytes"] == parent["workspace_bytes"]
    assert len(parent["plan_conv"]) >= 140 and min(parent["workspace_bytes"]) > 0


def _exotic(row, op):
    k, pad, reflect = row[10], row[5], row[6]
    if op == "wgrad":
        return max(pad) > 1 or k[0] not in (1, 3)                        # wgrad_route
    return max(pad) > 2 or (k != (1, 1, 1) and k[0] != 3) or (reflect and pad[0] > 1)     # conv_route


def flips(parent, row, op, impl):
    """Whether an engine of family `impl` with the switch on hands this launch to the route: family >= 1, an ordinary geometry, and no matrix, split-operand or
    dedicated kernel of families 1..impl takes it -- for those the parent's report names a kernel (DIRECT at impl >= 1: the dedicated upscale pair); the
    single-operator backward-filter of impl 2 IS the direct kernel, so its report says nothing about the engine."""
    if impl == 0 or _exotic(row, op):
        return False
    return all(_parent(parent, row, op, i)[0] == NONE or (op == "wgrad" and i == 2) for i in range(1, impl + 1))


def test_switch_on_who_takes_what(lib, parent):
    n_flip = 0
    for row in rows():
        for op in OPS:
            for impl in IMPLS:
                was, got = _parent(parent, row, op, impl), report(lib, "probav_plan_conv_gemm", row, op, impl)
                if flips(parent, row, op, impl):
                    assert got[0] == (WGRAD_GEMM if op == "wgrad" else GEMM), (row[0], op, impl, was, got)
                    n_flip += 1
                else:
                    assert got == was, (row[0], op, impl, was, got)
    assert n_flip > 300
    # the rows the route exists for: every 1x1x1 layer, and the channel counts no matrix kernel takes (Cout > 32; Cin not 1, 25 or a multiple of 16), as the operator
    # the row is named for and as its backward-filter
    for row in rows():
        name, Cin, Cout, k = row[0], row[3], row[4], row[10]
        odd = Cout > 32 or (Cin not in (1, 25) and Cin % 16 != 0)
        if k == (1, 1, 1) or (name.startswith("cfg:") and odd and k == (3, 3, 3)):
            op = "bwd" if "bwd-data" in name else "fwd"
            for impl in (1, 2, 3, 4):
                if not (op == "bwd" and Cin == 9 and Cout == 32):            # (the dedicated backward-data kernel of the upscale layer)
                    assert report(lib, "probav_plan_conv_gemm", row, op, impl)[0] == GEMM, (name, op, impl)
                if op == "fwd" and (Cout > 32 or Cin not in (1, 25, 32)):
                    assert report(lib, "probav_plan_conv_gemm", row, "wgrad", impl)[0] == WGRAD_GEMM, (name, impl)
    for name in ("cfg: normConv same 51->64 + skip", "cfg: normConv same 43->48 + skip", "cfg: mirrored-pad reducer 20->20", "cfg: expConv 1x1x1 64->512 relu",
                 "cfg: bwd-data of normConv: same 64->51", "cfg: bwd-data of expConv: 512->64 gated + skip", "expConv 1x1x1 32->256 relu"):
        assert any(r[0] == name for r in rows()), name


def test_family_0_and_bad_arguments(lib):
    from probav_amd import _lib as L
    row = next(r for r in rows() if r[0] == "cfg: normConv same 51->64 + skip")
    rep = (ctypes.c_int32 * 8)()
    for op in OPS:
        assert report(lib, "probav_plan_conv_gemm", row, op, 0) == report(lib, "probav_plan_conv", row, op, 0)
    assert lib.probav_plan_conv_gemm(ctypes.byref(_geom(row)), 5, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL        # as probav_plan_conv refuses impl 5
    assert lib.probav_plan_conv(ctypes.byref(_geom(row)), 5, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv_gemm(None, 1, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL


def test_plan_integers_cover_the_problem_once(lib, parent):
    seen_multi_slab = seen_n_tiles = False
    for row in rows():
        name, N, hwt, Cin, Cout, pad, k = row[0], row[1], row[2], row[3], row[4], row[5], row[10]
        ho = tuple(hwt[i] + 2 * pad[i] - k[i] + 1 for i in range(3))
        nvox, taps = N * ho[0] * ho[1] * ho[2], k[0] * k[1] * k[2]
        for impl in (1, 4):
            for op in ("fwd", "bwd"):
                if flips(parent, row, op, impl):
                    kern, ntn, ntm, tm, tn, grid, kc, chunks = report(lib, "probav_plan_conv_gemm", row, op, impl)
                    assert grid == ntn * ntm and tm > 0 and tn > 0
                    assert (ntm - 1) * tm < nvox <= ntm * tm, (name, ntm, tm, nvox)                # the voxel tiles cover M once, none is empty
                    assert (ntn - 1) * tn < Cout <= ntn * tn, (name, ntn, tn, Cout)                # ... and the channel tiles N
                    assert (chunks - 1) * kc < Cin <= chunks * kc                                  # the K chunks cover a tap's channels
                    seen_n_tiles |= ntn > 1
            if flips(parent, row, "wgrad", impl):
                rep = report(lib, "probav_plan_conv_gemm", row, "wgrad", impl)
                kern, slabs, vps, tci, tco, grid = rep[:6]
                nbytes = lib.probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(_geom(row)))
                assert nbytes == slabs * 4 * (taps * Cin * Cout + Cout), (name, rep, nbytes)
                assert (slabs - 1) * vps < nvox <= slabs * vps and 1 <= slabs <= 32, (name, rep)  # the slabs cover the voxels once, none is empty
                assert grid == slabs * taps * -(-Cin // tci) * -(-Cout // tco)
                assert rep == report(lib, "probav_plan_conv_gemm", row, "wgrad", impl)             # twice the same
                for other in (1, 2, 3, 4):                                                          # ... and nothing but the geometry decides it
                    if flips(parent, row, "wgrad", other):
                        assert rep == report(lib, "probav_plan_conv_gemm", row, "wgrad", other)
                seen_multi_slab |= slabs > 1
    assert seen_multi_slab and seen_n_tiles
    # what the route refuses: no scratch size, as probav_conv3d_wgrad_scratch_bytes answers 0 for a refused geometry
    g5 = pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 2), 0, 0, (5, 5, 5))
    assert lib.probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(g5)) == 0
    g2 = pc.geom(1, (9, 9, 9), 8, 8, (2, 2, 2), 0, 0)
    assert lib.probav_gemm_conv3d_wgrad_scratch_bytes(ctypes.byref(g2)) == 0                       # pads of 2: the backward-filter's exotic


def _counts(lib, h, batch=2):
    c = (ctypes.c_int32 * 4)()
    assert lib.probav_engine_route_counts(h, batch, ctypes.byref(c)) == 0
    return tuple(c)


@pytest.mark.parametrize("T", [9, 7, 13, 19])
def test_route_counts_of_the_64_filter_engine(lib, T):
    h = make_engine(lib, 64, 12, 8, 51, T)
    try:
        for impl in (1, 2, 3, 4):
            assert lib.probav_engine_set_impl(h, impl) == 0
            assert lib.probav_engine_set_gemm_route(h, 0) == 0
            off = _counts(lib, h)
            assert off[1] == 0 and off[3] == 0 and off[0] > 0 and off[2] > 0, off
            assert lib.probav_engine_set_gemm_route(h, 1) == 0
            on = _counts(lib, h)
            print("64 filters, T = %d, impl %d: off %s on %s" % (T, impl, off, on))
            assert on[0] + on[1] == off[0] and on[2] + on[3] == off[2]        # the same launches, other hands
            assert _counts(lib, h, 128) == on                                    # (the batch size moves nothing)
            if T != 19:
                assert on[0] == 0 and on[2] == 0, on
            else:
                # the 19-frame reducer (models/modelsTF.py:76-121): the 5x5x5 layer, the mirrored depth pad and the mirrored H/W pads of 2 stay on the direct
                # kernels -- forward and backward-filter of reducers 1-4, and the backward-data forms that are exotic themselves (5x5x5; the others are zero-pad
                # full correlations with pads of 2, which the route takes)
                assert on[2] == 4 and 4 <= on[0] <= 8 and on[1] > 0 and on[3] > 0, on
        # family 0: the direct kernels with or without the switch
        assert lib.probav_engine_set_impl(h, 0) == 0
        on0 = _counts(lib, h)
        assert lib.probav_engine_set_gemm_route(h, 0) == 0
        assert _counts(lib, h) == on0 and on0[1] == 0 and on0[3] == 0
    finally:
        lib.probav_engine_destroy(h)


def test_the_shipped_engine_launches_what_it_launched(lib, parent):
    h = make_engine(lib, *SHIPPED)
    try:
        for impl in IMPLS:
            assert lib.probav_engine_set_impl(h, impl) == 0
            assert lib.probav_engine_set_gemm_route(h, 0) == 0
            off = _counts(lib, h, 128)
            ws_off = [lib.probav_workspace_bytes(h, 128, t) for t in (0, 1)]
            assert lib.probav_engine_set_gemm_route(h, 1) == 0
            assert _counts(lib, h, 128) == off, impl
            assert off[1] == 0 and off[3] == 0 and (impl == 0 or (off[0] == 0 and off[2] == 0)), (impl, off)
            assert [lib.probav_workspace_bytes(h, 128, t) for t in (0, 1)] == ws_off
            assert ws_off == [parent["workspace_bytes"][WS_CASES.index((impl, 128, t))] for t in (0, 1)]
    finally:
        lib.probav_engine_destroy(h)


def test_set_impl_keeps_the_switch_and_the_environment_sets_it(lib, monkeypatch):
    h = make_engine(lib, 64, 2, 8, 51, 9)
    try:
        assert lib.probav_engine_gemm_route(h) == 0                            # off by default
        assert lib.probav_engine_set_impl(h, 1) == 0
        ws_off = lib.probav_workspace_bytes(h, 2, 1)
        assert lib.probav_engine_set_gemm_route(h, 1) == 0 and lib.probav_engine_gemm_route(h) == 1
        ws_on = lib.probav_workspace_bytes(h, 2, 1)
        for impl in (4, 0, 2, 1):
            assert lib.probav_engine_set_impl(h, impl) == 0
            assert lib.probav_engine_gemm_route(h) == 1
            assert (_counts(lib, h)[1] > 0) == (impl >= 1)
        assert lib.probav_workspace_bytes(h, 2, 1) == ws_on != ws_off        # the backward-filter's slab regions change size with the switch
        inf_on = lib.probav_workspace_bytes(h, 2, 0)
        assert lib.probav_engine_set_gemm_route(h, 0) == 0
        assert lib.probav_workspace_bytes(h, 2, 0) == inf_on                  # inference: no slab regions, nothing to size
        assert lib.probav_workspace_bytes(h, 2, 1) == ws_off
    finally:
        lib.probav_engine_destroy(h)
    assert lib.probav_engine_set_gemm_route(None, 1) == -1 and lib.probav_engine_gemm_route(None) == 0
    for value, want in (("1", 1), ("0", 0), ("7", 1), ("", 0)):
        monkeypatch.setenv("PROBAV_GEMM_ROUTE", value)
        h = make_engine(lib, 64, 2, 8, 51, 9)
        assert lib.probav_engine_gemm_route(h) == want, value
        lib.probav_engine_destroy(h)
    monkeypatch.delenv("PROBAV_GEMM_ROUTE")
    h = make_engine(lib, 64, 2, 8, 51, 9)
    assert lib.probav_engine_gemm_route(h) == 0
    lib.probav_engine_destroy(h)


def _load(name):
    spec = importlib.util.spec_from_file_location("probav_cli_gemm_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Stub:
    def __init__(self):
        self.calls = []

    def set_gemm_route(self, on):
        self.calls.append(on)


def test_the_flag_parses_and_reaches_the_model(built_lib, monkeypatch):
    from probav_amd import inference
    cfg = os.path.join(ROOT, "cfg", "p16t9c85r12f64.cfg")
    train_py, test_py, evaluate_py = _load("train"), _load("test"), _load("evaluate")
    with pytest.raises(SystemExit):                                              # a switch of the patchNet engine: FuseNet has none
        train_py.parser(["--cfg", cfg, "--modelType", "fusionNet", "--fusion-input", ROOT, "--gemm-route"])
    assert train_py.parser(["--cfg", cfg]).gemm_route is False and train_py.parser(["--cfg", cfg, "--gemm-route"]).gemm_route is True
    for opt, want in ((train_py.parser(["--cfg", cfg]), []), (train_py.parser(["--cfg", cfg, "--gemm-route"]), [True])):
        stub = _Stub()
        train_py.apply_engine_options(stub, opt)
        assert stub.calls == want
    assert test_py.parser(["--cfg", cfg]).gemm_route is False and evaluate_py.parser(["--cfg", cfg, "--model"]).gemm_route is False
    assert test_py.parser(["--cfg", cfg, "--gemm-route"]).gemm_route is True
    assert evaluate_py.parser(["--cfg", cfg, "--model", "--gemm-route"]).gemm_route is True
    assert test_py.parser(["--cfg", cfg, "--gemm-route"]).inference == inference.InferenceOptions()      # a switch of the engine, no option of the prediction
    with pytest.raises(SystemExit):
        evaluate_py.parser(["--cfg", cfg, "--toCompare", ROOT, "--gemm-route"])         # a folder of PNGs is scored as it is: no network, no route
    # load_model hands the option to the model it builds
    import probav_amd.modelsTF as modelsTF
    import probav_amd.trainClass as trainClass
    stub = _Stub()
    stub.to = lambda dev: stub

    class Builder:
        def __init__(self, **kw):
            pass

        def build(self, **kw):
            assert kw["numFilters"] == 64
            return stub

    monkeypatch.setattr(modelsTF, "WDSRConv3D", Builder)
    monkeypatch.setattr(trainClass, "ModelTrainer", lambda *a, **kw: "trainer")
    from probav_amd.parseConfig import parseConfig
    config = parseConfig(cfg)
    assert inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True) == (stub, "trainer") and stub.calls == [True]
    stub.calls.clear()
    inference.load_model(config, cfg, "NIR", "raw", "test.py")
    assert stub.calls == []


def test_the_64_filter_cfg_is_the_shipped_one_with_64_filters():
    from probav_amd.parseConfig import parseConfig
    shipped = parseConfig(os.path.join(ROOT, "cfg", "p16t9c85r12.cfg"))
    f64 = parseConfig(os.path.join(ROOT, "cfg", "p16t9c85r12f64.cfg"))
    assert f64["num_filters"] == 64 and shipped["num_filters"] == 32
    own = ("num_filters", "train_out", "test_out")                          # the outputs go to directories of their own
    assert {k: v for k, v in f64.items() if k not in own} == {k: v for k, v in shipped.items() if k not in own}
    assert all(f64[k] != shipped[k] for k in own)


def test_model_methods_exist():
    from probav_amd.modelsTF import WDSRModel
    assert callable(WDSRModel.set_gemm_route) and isinstance(WDSRModel.gemm_route, property)
