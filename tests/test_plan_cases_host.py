"""The case table of tests/plan_cases.py against the plan report of the built library (probav_plan_conv / probav_plan_pw: host only, no GPU).

(a) every plan class of the table is reached by at least one row, on the operator and impl the class names: removing a class's rows fails here;
(b) no row of tests/test_gpu_parity.py::CONV_CASES with N <= 5 reaches any of these classes, under any operator: the gap this table closes -- if someone closes
    it there, this fails and the row here can go;
(c) the class a row names is what the report says of it: a change of a plan moves the row off its branch loudly;
and the report itself: it agrees with what the launch paths document of themselves (the scratch size of the backward-filter, the refusals of the single-operator
entry points), and it needs no device."""
import ctypes

import pytest

from tests import plan_cases as pc

CONV_RUNS = [(row, run) for row in pc.CONV_ROWS for run in row[10]]
PW_RUNS = [(row, run) for row in pc.PW_ROWS for run in row[4]]


def _ids(runs):
    return ["%s | %s impl %d" % (row[0], run[0], run[1]) for row, run in runs]


@pytest.mark.parametrize("row,run", CONV_RUNS, ids=_ids(CONV_RUNS))
def test_conv_row_is_on_its_plan_class(built_lib, row, run):
    op, impl, cls = run
    assert pc.CLASSES[cls][:2] == (op, impl)
    rep = pc.conv_report(row, op, impl)
    print("%s | %s impl %d: %s" % (row[0], op, impl, rep))
    assert pc.CLASSES[cls][2](rep, row), (cls, rep)                                         # (c)


@pytest.mark.parametrize("row,run", PW_RUNS, ids=_ids(PW_RUNS))
def test_pointwise_row_is_on_its_plan_class(built_lib, row, run):
    op, impl, cls = run
    assert pc.CLASSES[cls][:2] == (op, impl) and cls in pc.PW_CLASSES
    rep = pc.pw_report(row, op, impl)
    print("%s | %s impl %d: %s" % (row[0], op, impl, rep))
    assert pc.CLASSES[cls][2](rep, row), (cls, rep)                                         # (c)


def test_every_plan_class_has_a_row(built_lib):
    reached = {run[2] for _, run in CONV_RUNS + PW_RUNS}
    assert reached == set(pc.CLASSES), sorted(set(pc.CLASSES) ^ reached)                    # (a)
    names = [r[0] for r in pc.CONV_ROWS + pc.PW_ROWS]
    assert len(set(names)) == len(names)
    for a, b in pc.HANDOVERS:
        ra, rb = pc.row_by_name(a), pc.row_by_name(b)
        assert rb[1] == ra[1] + 1 and ra[2:4] == rb[2:4]


def test_the_small_batch_cases_reach_none_of_these_classes(built_lib):
    from tests.test_gpu_parity import CONV_CASES
    small = [c for c in CONV_CASES if c[1] <= 5]
    assert len(small) == len(CONV_CASES) >= 100                                             # (every row there is such a row)
    conv_classes = {c: v for c, v in pc.CLASSES.items() if c not in pc.PW_CLASSES}
    for case in small:
        name, N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip = case
        row = (name, N, hwt, Cin, Cout, pad, reflect, relu, use_gate, use_skip)
        reports = {}
        for cls, (op, impl, pred) in conv_classes.items():
            if (op, impl) not in reports:
                reports[(op, impl)] = pc.conv_report(row, op, impl, k)
            assert not pred(reports[(op, impl)], row), (name, cls, reports[(op, impl)])     # (b)


def test_the_report_agrees_with_the_entry_points(built_lib):
    """Where the report says `none` the single-operator entry point refuses the call (for the backward-filter: its scratch size is 0), elsewhere not; the grid of a
    backward-filter plan is the number of slabs its scratch is sized for."""
    from probav_amd import _lib as L
    from tests.test_gpu_parity import CONV_CASES
    lib = L.lib()
    rows = [(c[0], c[1], c[2], c[3], c[4], c[6], c[7], c[8], c[9], c[10], c[5]) for c in CONV_CASES] + [r[:10] + (pc.K3,) for r in pc.CONV_ROWS]
    seen = set()
    for row in rows:
        k = row[10]
        g = pc.geom(row[1], row[2], row[3], row[4], row[5], row[6], row[7], k)
        for impl in range(5):
            rep = pc.conv_report(row, "wgrad", impl, k)
            nbytes = lib.probav_conv3d_wgrad_scratch_bytes(ctypes.byref(g), impl)
            assert (rep["kernel"] == "none") == (nbytes == 0), (row[0], impl, rep, nbytes)
            if rep["kernel"] in ("wg4", "x6", "mfma"):
                slab = 27 * row[3] * row[4] + row[4]
                assert nbytes >= rep["grid"] * slab * 4, (row[0], impl, rep, nbytes)
                if rep["kernel"] != "wg4":
                    assert nbytes == rep["grid"] * slab * 4 or impl >= 3, (row[0], impl, rep, nbytes)
            seen.add(rep["kernel"])
            for op in ("fwd", "bwd"):
                rep = pc.conv_report(row, op, impl, k)
                assert impl > 0 or rep["kernel"] == "direct"
                if rep["kernel"] in ("cw4", "pp", "pstrip", "strip"):
                    ho = pc.out_dims(row[2], row[5])[0]
                    assert rep["grid"] == row[1] * rep["nstrips"] * rep["nsplit"] and (rep["nstrips"] - 1) * rep["SR"] < ho <= rep["nstrips"] * rep["SR"], (row[0], rep)
                seen.add(rep["kernel"])
    assert {"cw4", "pp", "pstrip", "strip", "rowtile", "direct", "wg4", "x6", "mfma", "none"} <= seen, seen


def test_the_report_refuses_what_it_cannot_read(built_lib):
    from probav_amd import _lib as L
    lib = L.lib()
    rep = (ctypes.c_int32 * 8)()
    g = pc.geom(2, (22, 22, 9), 25, 32, pc.SAME, 0, 0)
    assert lib.probav_plan_conv(ctypes.byref(g), 5, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv(ctypes.byref(g), 4, 0, 0, 3, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_conv(None, 4, 0, 0, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_pw(0, 0, 25, 4, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_pw(64, 0, 25, 1, 0, ctypes.byref(rep)) == L.PROBAV_EINVAL
    assert lib.probav_plan_pw(64, 0, 27, 4, 1, ctypes.byref(rep)) == L.PROBAV_OK and pc.KERNELS[rep[0]] == "none"      # what probav_pw_backward refuses
    assert lib.probav_plan_pw(64, 0, 25, 4, 1, ctypes.byref(rep)) == L.PROBAV_OK and pc.KERNELS[rep[0]] == "pw4" and rep[7] == 1024
