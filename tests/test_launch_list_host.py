"""The engine's launch list (csrc/engine.hip: step_launches) on the host: the built library, no device.

The census (probav_engine_route_counts), the slab regions and the amax slot count of make_plan are loops over one list of a training step's launches.
tests/golden/launch_list_parent.json holds what the commit BEFORE that list answered -- where the census walked the network by hand and make_plan restated the
backward pass -- for every engine of tests/cfg_grid.py at every frame count, every kernel family, the general matrix route off and on, and three batch sizes: the four
census counts, probav_workspace_bytes (inference, training) and both values of probav_workspace_split.  The built library must answer the same, entry by entry."""
import ctypes
import json
import os

import pytest

from tests import cfg_grid
from tests.test_gemm_route_host import make_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_list_parent.json")
SHIPPED = (32, 12, 8, 0.8, 25)
FRAMES = (7, 9, 13, 19)
IMPLS = (0, 1, 2, 3, 4)
BATCHES = (1, 2, 128)


def engines():
    """(F, R, E, D, T, input channels): every row of the grid and the shipped network at every frame count, gray; the rgb row of VARIANTS."""
    rows = [row for row, _ in cfg_grid.GRID] + [SHIPPED]
    out = [(F, R, E, D, T, 1) for (F, R, E, _, D) in rows for T in FRAMES]
    out += [(F, R, E, D, T, 3) for (F, R, E, _, D), T, gray, _ in cfg_grid.VARIANTS if not gray]
    assert len(set(out)) == len(out)
    return out


def key(eng, impl, gemm, batch):
    return "f%d-r%d-e%d-d%d-t%d-c%d/impl%d/gemm%d/b%d" % (eng + (impl, gemm, batch))


def parent_reports(lib):
    """What the fixture holds: key -> [4 census counts, workspace bytes (inference, training), saved bytes, scratch bytes].  Run on the commit BEFORE the launch list
    (any library that exports probav_engine_route_counts and probav_workspace_split): json.dump(parent_reports(lib), fh, separators=(",", ":"))."""
    out = {}
    for eng in engines():
        h = make_engine(lib, *eng)
        try:
            for impl in IMPLS:
                assert lib.probav_engine_set_impl(h, impl) == 0
                for gemm in (0, 1):
                    assert lib.probav_engine_set_gemm_route(h, gemm) == 0
                    for batch in BATCHES:
                        counts = (ctypes.c_int32 * 4)()
                        assert lib.probav_engine_route_counts(h, batch, ctypes.byref(counts)) == 0
                        saved, scratch = ctypes.c_size_t(), ctypes.c_size_t()
                        assert lib.probav_workspace_split(h, batch, ctypes.byref(saved), ctypes.byref(scratch)) == 0
                        out[key(eng, impl, gemm, batch)] = [list(counts), [int(lib.probav_workspace_bytes(h, batch, t)) for t in (0, 1)],
                                                            int(saved.value), int(scratch.value)]
        finally:
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


def test_the_fixture_is_not_thin(parent):
    assert len(parent) >= 1400
    assert set(parent) == {key(eng, impl, gemm, batch) for eng in engines() for impl in IMPLS for gemm in (0, 1) for batch in BATCHES}
    for impl in IMPLS:
        assert any("/impl%d/" % impl in k for k in parent)
    for gemm in (0, 1):
        assert any("/gemm%d/" % gemm in k for k in parent)
    for slot in range(4):
        assert any(v[0][slot] > 0 for v in parent.values()), slot
    assert all(0 < v[1][0] < v[1][1] and v[2] + v[3] == v[1][1] for v in parent.values())


def test_census_and_workspace_sizes_are_the_parents(lib, parent):
    now = parent_reports(lib)
    assert set(now) == set(parent)
    for k, was in parent.items():
        assert now[k] == was, (k, was, now[k])
