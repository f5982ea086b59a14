"""The general matrix route's fused pointwise pair (csrc/kernels_gemm_pw.hip; include/probav_hip.h, 'the route's fused pointwise pair') on the host: the built
library, no device.

(a) the wish is off by default, PROBAV_GEMM_PAIR sets it, probav_engine_set_impl / probav_engine_set_gemm_route keep it, a null engine answers -1 / 0;
(b) probav_engine_pair_kind: 0 at family 0, 1 for the shipped shape at every family >= 1 whatever the switches, 2 only with route AND pair on inside the range;
(c) wish off -- or on where the kind is not 2 -- every workspace size and census count is the parent's: tests/golden/gemm_pair_parent.json, generated on the commit
    before the pair by parent_reports() below;
(d) kind 2: the census loses 5 convolution and 2 backward-filter launches per block on the route, nothing moves on the direct kernels;
(e) kind 2: the workspace loses its three hidden-sized tensors for less than one of them in slabs;
(f) probav_plan_pw_gemm: tiles, chunks and slabs cover the problem exactly once; the slab count follows from the voxel count alone;
(g) --gemm-pair parses, needs --gemm-route and reaches set_gemm_pair."""
import ctypes
import json
import os

import pytest

from tests.test_gemm_route_host import _load, make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_pair_parent.json")
IMPLS = (0, 1, 2, 3, 4)
PAIR_SHAPES = [(64, 8, 51), (48, 6, 43), (32, 8, 28), (32, 4, 25), (20, 3, 10), (16, 8, 12)]       # F, expRate, D: what the general pair exists for
SHIPPED = (32, 8, 25)
R = 2
VOX = 22 * 22 * 9                                                                               # voxels of a 16-pixel patch at 9 frames


def _engine(lib, shape, blocks=R, T=9):
    F, E, D = shape
    return make_engine(lib, F, blocks, E, D, T)


def _counts(lib, h, batch=2):
    c = (ctypes.c_int32 * 4)()
    assert lib.probav_engine_route_counts(h, batch, ctypes.byref(c)) == 0
    return list(c)


def _state(lib, h):
    """What an engine answers about its sizes and launches: workspace bytes (batch 1, 2, 128; inference, training), the split (batch 2, 128), the census."""
    ws = [int(lib.probav_workspace_bytes(h, b, t)) for b in (1, 2, 128) for t in (0, 1)]
    split = []
    for b in (2, 128):
        saved, scr = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.probav_workspace_split(h, b, ctypes.byref(saved), ctypes.byref(scr)) == 0
        split += [int(saved.value), int(scr.value)]
    return {"workspace_bytes": ws, "workspace_split": split, "route_counts": _counts(lib, h)}


def _key(shape, impl, route):
    return "f%d-e%d-d%d impl %d route %d" % (shape + (impl, route))


def parent_reports(lib):
    """What the fixture holds.  Run on the commit BEFORE the pair (any library that exports probav_engine_create, probav_engine_set_impl,
    probav_engine_set_gemm_route, probav_workspace_bytes, probav_workspace_split and probav_engine_route_counts with their argument types set)."""
    out = {}
    for shape in PAIR_SHAPES + [SHIPPED]:
        h = _engine(lib, shape)
        for impl in IMPLS:
            for route in (0, 1):
                assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, route) == 0
                out[_key(shape, impl, route)] = _state(lib, h)
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


def test_off_by_default_and_who_keeps_the_wish(lib, monkeypatch):
    monkeypatch.delenv("PROBAV_GEMM_PAIR", raising=False)
    monkeypatch.delenv("PROBAV_GEMM_ROUTE", raising=False)
    h = _engine(lib, (64, 8, 51))
    try:
        assert lib.probav_engine_gemm_pair(h) == 0 and lib.probav_engine_pair_kind(h) == 0           # off by default
        assert lib.probav_engine_set_gemm_pair(h, 1) == 0 and lib.probav_engine_gemm_pair(h) == 1
        assert lib.probav_engine_pair_kind(h) == 0                                                    # the wish alone: no route, no pair
        for impl in (1, 4, 0, 2):
            assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_gemm_pair(h) == 1
        for route in (1, 0, 1):
            assert lib.probav_engine_set_gemm_route(h, route) == 0 and lib.probav_engine_gemm_pair(h) == 1
        assert lib.probav_engine_pair_kind(h) == 2                                                    # impl 2, route on, wish kept through all of it
        assert lib.probav_engine_set_gemm_pair(h, 0) == 0 and lib.probav_engine_gemm_pair(h) == 0 and lib.probav_engine_pair_kind(h) == 0
        assert lib.probav_engine_gemm_route(h) == 1                                                   # ... and the pair's setter keeps the route
    finally:
        lib.probav_engine_destroy(h)
    assert lib.probav_engine_set_gemm_pair(None, 1) == -1 and lib.probav_engine_gemm_pair(None) == 0 and lib.probav_engine_pair_kind(None) == 0
    for value, want in (("1", 1), ("0", 0), ("7", 1), ("", 0)):
        monkeypatch.setenv("PROBAV_GEMM_PAIR", value)
        h = _engine(lib, (64, 8, 51))
        assert lib.probav_engine_gemm_pair(h) == want and lib.probav_engine_gemm_route(h) == 0, value
        lib.probav_engine_destroy(h)
    monkeypatch.setenv("PROBAV_GEMM_ROUTE", "1")
    monkeypatch.setenv("PROBAV_GEMM_PAIR", "1")
    h = _engine(lib, (64, 8, 51))
    assert lib.probav_engine_pair_kind(h) == 2                                                        # the default family, both from the environment
    lib.probav_engine_destroy(h)


def _set(lib, h, impl, route, pair):
    assert lib.probav_engine_set_impl(h, impl) == 0 and lib.probav_engine_set_gemm_route(h, route) == 0 and lib.probav_engine_set_gemm_pair(h, pair) == 0


def test_pair_kind(lib):
    for shape in PAIR_SHAPES:
        h = _engine(lib, shape)
        try:
            for impl in IMPLS:
                for route in (0, 1):
                    for pair in (0, 1):
                        _set(lib, h, impl, route, pair)
                        want = 2 if (impl >= 1 and route and pair) else 0
                        assert lib.probav_engine_pair_kind(h) == want, (shape, impl, route, pair)
        finally:
            lib.probav_engine_destroy(h)
    h = _engine(lib, SHIPPED, blocks=12)
    try:
        for impl in IMPLS:
            for route in (0, 1):
                for pair in (0, 1):
                    _set(lib, h, impl, route, pair)
                    assert lib.probav_engine_pair_kind(h) == (1 if impl >= 1 else 0), (impl, route, pair)      # the tuned pair keeps every shape it has
    finally:
        lib.probav_engine_destroy(h)
    for shape in ((80, 8, 64), (64, 8, 70), (80, 1, 80)):                                             # beyond the range: un-fused on the route
        h = _engine(lib, shape)
        try:
            for impl in (1, 4):
                _set(lib, h, impl, 1, 1)
                assert lib.probav_engine_pair_kind(h) == 0, shape
        finally:
            lib.probav_engine_destroy(h)


def test_switch_off_is_the_parents(lib, parent):
    assert parent_reports(lib) == parent
    assert len(parent) == 7 * 5 * 2 and all(min(v["workspace_bytes"]) > 0 for v in parent.values())
    # the wish on: still the parent's wherever the general pair does not run
    n_same = n_pair = 0
    for shape in PAIR_SHAPES + [SHIPPED]:
        h = _engine(lib, shape)
        try:
            for impl in IMPLS:
                for route in (0, 1):
                    _set(lib, h, impl, route, 1)
                    if lib.probav_engine_pair_kind(h) != 2:
                        assert _state(lib, h) == parent[_key(shape, impl, route)], (shape, impl, route)
                        n_same += 1
                    else:
                        assert _state(lib, h) != parent[_key(shape, impl, route)]
                        n_pair += 1
        finally:
            lib.probav_engine_destroy(h)
    assert n_pair == 6 * 4 and n_same == 70 - n_pair


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=["f%d-e%d-d%d" % s for s in PAIR_SHAPES])
def test_census_with_the_pair_on(lib, shape):
    for blocks in (2, 12):
        h = _engine(lib, shape, blocks)
        try:
            for impl in (1, 2, 3, 4):
                _set(lib, h, impl, 1, 0)
                off = _counts(lib, h)
                _set(lib, h, impl, 1, 1)
                assert lib.probav_engine_pair_kind(h) == 2
                on = _counts(lib, h)
                # exp, dec, the recomputed hidden tensor, dec's and exp's backward-data; dec's and exp's backward-filter
                assert on == [off[0], off[1] - 5 * blocks, off[2], off[3] - 2 * blocks], (shape, impl, off, on)
                assert _counts(lib, h, 128) == on
        finally:
            lib.probav_engine_destroy(h)


def test_workspace_with_the_pair_on(lib):
    """A condition of the design, not a measurement: three hidden tensors go away, the pair's slab regions cost at most one of them."""
    h = _engine(lib, (64, 8, 51), blocks=12)
    try:
        for impl in (1, 4):
            hidden = 128 * VOX * 512 * 4
            _set(lib, h, impl, 1, 0)
            off = lib.probav_workspace_bytes(h, 128, 1)
            off16 = lib.probav_workspace_bytes(h, 16, 0)
            _set(lib, h, impl, 1, 1)
            on = lib.probav_workspace_bytes(h, 128, 1)
            on16 = lib.probav_workspace_bytes(h, 16, 0)
            print("64 filters, batch 128, training, impl %d: %.3f GB un-fused, %.3f GB fused (a hidden tensor: %.3f GB)" % (impl, off / 1e9, on / 1e9, hidden / 1e9))
            assert off - on >= 2 * hidden, (off, on)
            assert off16 - on16 >= (16 * VOX * 512 * 4) // 2, (off16, on16)
            saved, scr = ctypes.c_size_t(), ctypes.c_size_t()
            assert lib.probav_workspace_split(h, 128, ctypes.byref(saved), ctypes.byref(scr)) == 0 and saved.value + scr.value == on
    finally:
        lib.probav_engine_destroy(h)


def _plan(lib, F, H, D, nvox, backward):
    rep = (ctypes.c_int32 * 8)()
    assert lib.probav_plan_pw_gemm(F, H, D, nvox, backward, ctypes.byref(rep)) == 0
    return list(rep)


@pytest.mark.parametrize("nvox", [900, 1800, 13068, 557568])
def test_plan_covers_the_problem_once(lib, nvox):
    for H in (60, 128, 288, 512):
        for F, D in ((64, 51), (20, 10), (32, 28)):
            for backward in (0, 1):
                tile, tiles, cw, chunks, grid, slabs, vps, zero = rep = _plan(lib, F, H, D, nvox, backward)
                assert tile > 0 and (tiles - 1) * tile < nvox <= tiles * tile, rep                  # the tiles cover [0, nvox) once, none is empty
                assert cw == 32 and (chunks - 1) * cw < H <= chunks * cw and zero == 0, rep         # the chunks cover [0, H) once
                if backward:
                    assert slabs >= 1 and vps % 32 == 0 and (slabs - 1) * vps < nvox <= slabs * vps, rep   # no empty slab before the last (nor there)
                    assert grid == tiles + slabs * -(-chunks // 8)
                    assert _plan(lib, 16, 8, 3, nvox, 1)[5:7] == [slabs, vps]                        # the voxel count alone decides the slabs
                else:
                    assert slabs == 0 and vps == 0 and grid == tiles
                assert rep == _plan(lib, F, H, D, nvox, backward)
    assert _plan(lib, 80, 512, 51, nvox, 0) == [0] * 8 and _plan(lib, 64, 512, 70, nvox, 1) == [0] * 8 and _plan(lib, 64, 0, 51, nvox, 0) == [0] * 8
    assert lib.probav_plan_pw_gemm(64, 512, 51, nvox, 0, None) == -1


class _Stub:
    def __init__(self):
        self.calls = []

    def set_gemm_route(self, on):
        self.calls.append(("route", on))

    def set_gemm_pair(self, on):
        self.calls.append(("pair", on))


def test_the_flags_parse_and_reach_the_model(built_lib, monkeypatch):
    from probav_amd import inference
    cfg = os.path.join(ROOT, "cfg", "p16t9c85r12f64.cfg")
    train_py, test_py, evaluate_py = _load("train"), _load("test"), _load("evaluate")
    both = ["--gemm-route", "--gemm-pair"]
    for parse, base in ((train_py.parser, ["--cfg", cfg]), (test_py.parser, ["--cfg", cfg]), (evaluate_py.parser, ["--cfg", cfg, "--model"])):
        assert parse(base).gemm_pair is False and parse(base + ["--gemm-route"]).gemm_pair is False and parse(base + both).gemm_pair is True
        with pytest.raises(SystemExit):
            parse(base + ["--gemm-pair"])                                         # the pair is the route's: alone it is an error
    with pytest.raises(SystemExit):
        train_py.parser(["--cfg", cfg, "--modelType", "fusionNet", "--fusion-input", ROOT] + both)
    with pytest.raises(SystemExit):
        evaluate_py.parser(["--cfg", cfg, "--toCompare", ROOT] + both)
    for argv, want in ((["--cfg", cfg], []), (["--cfg", cfg, "--gemm-route"], [("route", True)]), (["--cfg", cfg] + both, [("route", True), ("pair", True)])):
        stub = _Stub()
        train_py.apply_engine_options(stub, train_py.parser(argv))
        assert stub.calls == want
    assert test_py.parser(["--cfg", cfg] + both).inference == inference.InferenceOptions()            # switches of the engine, no options of the prediction
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
    assert inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True, gemm_pair=True) == (stub, "trainer")
    assert stub.calls == [("route", True), ("pair", True)]
    stub.calls.clear()
    inference.load_model(config, cfg, "NIR", "raw", "test.py", gemm_route=True)
    assert stub.calls == [("route", True)]


def test_model_methods_exist():
    from probav_amd.modelsTF import WDSRModel
    assert callable(WDSRModel.set_gemm_pair) and isinstance(WDSRModel.gemm_pair, property)
