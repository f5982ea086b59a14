"""The case table of the batch- and width-dependent launch plans: one list serves tests/test_plan_cases_host.py (the plan report alone, no GPU) and
tests/test_gpu_plans.py (every row on the device against the fp64 oracle).

Every hand-scheduled convolution kernel partitions its work from the batch size N and the output extents (cw4_plan, pp_plan, pstrip_plan, strip_plan, wg4_plan,
x6_wgrad_split / x6_wgrad_grid, conv_plan; the fused pointwise pair from the sample count).  tests/test_gpu_parity.py::CONV_CASES never moves N above 5, where
each kernel takes one plan -- not the one a batch of 128 runs.  A row here names a geometry and, per (operator, impl), the PLAN CLASS it is there for; the class is
a predicate on what probav_plan_conv / probav_plan_pw report (include/probav_hip.h: the report comes from the functions the launch paths call), so a change of a
plan moves a row off its class loudly, on a machine without a GPU.

A conv row is (name, N, (Hi, Wi, Ti), Cin, Cout, pad, reflect, relu, gate, skip, runs): one 3x3x3 layer as CONV_CASES writes it; runs = ((op, impl, class), ...),
op 'fwd' = probav_conv3d_forward with a bias, 'bwd' = the same without one (how the engine launches backward-data), 'wgrad' = probav_conv3d_wgrad, whose dY is
masked by the layer's own output when the layer has a ReLU.  A pointwise row is (name, samples, voxels per sample, D, runs), op 'fwd' / 'bwd'.

What the report says at the shipped shapes (22 x 22 x 9, one workgroup slot per compute unit: 256):
  conv3_w4_kernel (cw4) cuts a 22-wide row into TWO column ranges (a whole row is 594 staging items, over its 512), so nstrips = ceil(256 / (2 N)):
      N <= 5: 5 strips of 5 rows; N = 32: strips of 6, 6, 6, 4; N = 43: 8, 8, 6; N = 64: 11, 11; N = 128 (shipped): one strip of 22 rows, grid 256; N = 256: the same, grid 512.
      A 30-wide row (patch size 24) takes three ranges; a 23-wide one (patch size 17) fits no range count and conv3_pstrip_kernel takes the layer.
  conv3_strip_kernel (impl 2, 3) has no column ranges: N = 128 gives two strips of 11 rows.
  conv3_pp_kernel takes the reducers and every gated or depth-13 layer: 36- and 44-wide rows at depth 13 take 3 and 4 ranges.
  conv3_wgrad_w4_kernel (wg4): nstrips = 256 / (N nsplit): N <= 5 gives one row per workgroup; N = 24: strips of 3 rows and a last one of 1; N = 128: 11 rows; N = 256: 22;
      N nsplit > 256 hands the layer to conv3_wgrad_x6_kernel (N = 257; N = 129 at depth 13, where a workgroup takes half the columns).
  conv3_wgrad_x6_kernel / conv3_wgrad_mfma_kernel walk runs of (patch, row) tiles once there are more tiles than workgroups.
  pw_bwd_w4_kernel: wps = 1024 / samples waves per sample; above 1024 samples pw_bwd_x6_kernel<H3> serves the pair."""
import ctypes
import zlib

import numpy as np

KERNELS = {0: "none", 1: "cw4", 2: "pp", 3: "pstrip", 4: "strip", 5: "rowtile", 6: "direct", 7: "wg4", 8: "x6", 9: "x6-h3", 10: "mfma",
           20: "pw4", 21: "pw-x6-h3", 22: "pw-x6", 23: "pf4", 24: "pw-h3k", 25: "pw-mfma"}
FIELDS = ("kernel", "nsplit", "nstrips", "SR", "nslot", "grid", "rvp", "wps")
OPS = {"fwd": 0, "bwd": 1, "wgrad": 2}
K3 = (3, 3, 3)


def out_dims(hwt, pad):
    return tuple(hwt[i] + 2 * pad[i] - 2 for i in range(3))


def geom(N, hwt, Cin, Cout, pad, reflect, relu, k=K3):
    ho = tuple(hwt[i] + 2 * pad[i] - k[i] + 1 for i in range(3))
    return (ctypes.c_int32 * 17)(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k[0], k[1], k[2], pad[0], pad[1], pad[2], reflect, relu)


def conv_report(row, op, impl, k=K3):
    """probav_plan_conv of a conv row (or a CONV_CASES row: pass its kernel size) as a dict of FIELDS, the kernel by name."""
    from probav_amd import _lib as L
    name, N, hwt, Cin, Cout, pad, reflect, relu, gate, skip = row[:10]
    gated = relu if op == "wgrad" else gate
    rep = (ctypes.c_int32 * 8)()
    L.check(L.lib().probav_plan_conv(ctypes.byref(geom(N, hwt, Cin, Cout, pad, reflect, relu, k)), impl, int(bool(gated)), int(bool(skip)), OPS[op], ctypes.byref(rep)),
            "probav_plan_conv")
    d = dict(zip(FIELDS, rep))
    d["kernel"] = KERNELS[d["kernel"]]
    return d


def pw_report(row, op, impl):
    from probav_amd import _lib as L
    name, nsamp, vps, D = row[:4]
    rep = (ctypes.c_int32 * 8)()
    L.check(L.lib().probav_plan_pw(nsamp * vps, vps, D, impl, int(op == "bwd"), ctypes.byref(rep)), "probav_plan_pw")
    d = dict(zip(FIELDS, rep))
    d["kernel"] = KERNELS[d["kernel"]]
    return d


# ---- the plan classes: name -> (op, impl, predicate(report, row)) -------------------------------------------------------------------------------------
def _is(row, Cin, Cout, pad, reflect=0):
    return row[3] == Cin and row[4] == Cout and tuple(row[5]) == pad and row[6] == reflect


def _Ho(row):
    return out_dims(row[2], row[5])[0]


def _Wo(row):
    return out_dims(row[2], row[5])[1]


SAME, MIRROR, VALID = (1, 1, 1), (1, 1, 0), (0, 0, 0)
_short = lambda r, w: _Ho(w) % r["SR"] != 0 and r["nstrips"] >= 3          # several strips, the last one shorter


def _cw4(Cin, Cout):
    """normConv forward (25 -> 32 + skip) / its backward-data (32 -> 25): the five plans of conv3_w4_kernel and the width at which it declines."""
    me = lambda w: _is(w, Cin, Cout, SAME) and not w[8]
    cw4 = lambda r, w: me(w) and r["kernel"] == "cw4"
    return {
        "shipped: N = 128, one strip of all 22 rows per column range, grid 256": lambda r, w: cw4(r, w) and r["nstrips"] == 1 and r["SR"] == 22 and r["grid"] == 256,
        "N = 256: one strip per column range, two workgroups per compute unit slot": lambda r, w: cw4(r, w) and r["nstrips"] == 1 and r["SR"] == 22 and r["grid"] >= 512,
        "SR = 11: two strips": lambda r, w: cw4(r, w) and r["nstrips"] == 2 and r["SR"] == 11,
        "SR of 6 or 8 with a short last strip": lambda r, w: cw4(r, w) and r["SR"] in (6, 8) and _short(r, w),
        "a 30-wide row at depth 9: three column ranges": lambda r, w: cw4(r, w) and r["nsplit"] == 3,
        # cw4's static conditions hold ('same', depth 9 or 7, no gate), yet no range count fits its staging: a piece-ring kernel takes the layer
        "declines on items (an odd width), a piece-ring kernel takes over": lambda r, w: me(w) and w[2][2] in (7, 9) and _Wo(w) % 2 == 1 and r["kernel"] in ("pp", "pstrip"),
    }


def _wg4(mode, Cin, pad, reflect):
    me = lambda w: _is(w, Cin, 32, pad, reflect)
    wg4 = lambda r, w: me(w) and r["kernel"] == "wg4"
    d = {
        "SR of 2 or 3 with a short last strip": lambda r, w: wg4(r, w) and r["SR"] in (2, 3) and _short(r, w),
        "N = 128: two strips of half the rows": lambda r, w: wg4(r, w) and r["nsplit"] == 1 and r["nstrips"] == 2 and r["SR"] >= 9,
        "N = 256: all rows in one strip, the last batch wg4 takes": lambda r, w: wg4(r, w) and r["nsplit"] == 1 and r["nstrips"] == 1 and w[1] == 256,
        "N = 257: handed to the general x6 kernel": lambda r, w: me(w) and w[1] == 257 and w[2][2] != 13 and r["kernel"] == "x6" and r["grid"] == 256,
    }
    if mode != "unpadded":
        d["depth 13, column halves, N = 128: all rows in one strip, the last batch wg4 takes"] = \
            lambda r, w: wg4(r, w) and r["nsplit"] == 2 and r["nstrips"] == 1 and r["SR"] == 22 and w[1] == 128
        d["depth 13, N = 129: handed to the general x6 kernel"] = lambda r, w: me(w) and w[1] == 129 and w[2][2] == 13 and r["kernel"] == "x6" and r["nsplit"] == 2
    return d


def _tiles(r, w):
    return w[1] * _Ho(w) * r["nsplit"]


def _pw(kernel):
    me = lambda r, w: r["kernel"] == kernel and w[3] == 25
    return {
        "shipped: 128 samples of 4 356 voxels (137 tiles, the last of 4 voxels), 8 waves per sample": lambda r, w: me(r, w) and w[1] == 128 and w[2] == 4356,
        "8 waves per sample over 8k + 1 tiles, the last of 4 voxels": lambda r, w: me(r, w) and w[1] == 128 and w[2] != 4356 and ((w[2] + 31) // 32) % 8 == 1 and w[2] % 32 == 4,
        "512 samples: 2 waves per sample": lambda r, w: me(r, w) and w[1] == 512,
        "1024 samples: 1 wave per sample, the last batch pw4 takes": lambda r, w: me(r, w) and w[1] == 1024,
    }


CLASSES = {}
for _k, _p in _cw4(25, 32).items():
    CLASSES["cw4 forward 25->32 + skip / " + _k] = ("fwd", 4, _p)
for _k, _p in _cw4(32, 25).items():
    CLASSES["cw4 backward-data 32->25 / " + _k] = ("bwd", 4, _p)
for _op in ("fwd", "bwd"):
    CLASSES.update({
        "pp %s / SR >= 8, two staging items per thread" % _op: (_op, 4, lambda r, w: r["kernel"] == "pp" and r["SR"] >= 8 and r["rvp"] == 2),
        "pp %s / SR >= 8, three staging items per thread" % _op: (_op, 4, lambda r, w: r["kernel"] == "pp" and r["SR"] >= 8 and r["rvp"] == 3),
    })
CLASSES.update({
    "pp / a 36-wide row at depth 13: three column ranges": ("bwd", 4, lambda r, w: r["kernel"] == "pp" and r["nsplit"] == 3),
    "pp / a 44-wide row at depth 13: four column ranges": ("bwd", 4, lambda r, w: r["kernel"] == "pp" and r["nsplit"] == 4),
    "pp forward / three and four column ranges": ("fwd", 4, lambda r, w: r["kernel"] == "pp" and r["nsplit"] >= 3),
    "pstrip / SR >= 8": ("fwd", 4, lambda r, w: r["kernel"] == "pstrip" and r["SR"] >= 8),
    "strip (impl 2) / SR >= 8": ("fwd", 2, lambda r, w: r["kernel"] == "strip" and r["SR"] >= 8),
})
for _mode, _a in (("normConv", (25, SAME, 0)), ("mirrored-pad reducer", (32, MIRROR, 1)), ("unpadded reducer", (32, VALID, 0))):
    for _k, _p in _wg4(_mode.split()[0], *_a).items():
        CLASSES["wg4 %s / %s" % (_mode, _k)] = ("wgrad", 4, _p)
CLASSES.update({
    # more (patch, row) tiles than the 256 workgroups, not a multiple of them: runs of several rows, uneven, crossing from a patch's last row to the next patch's first
    "x6 wgrad (impl 3) / runs of several rows across patches, uneven": ("wgrad", 3, lambda r, w: r["kernel"] == "x6" and r["grid"] == 256 and _tiles(r, w) > 512 and _tiles(r, w) % 256 != 0),
    "x6 wgrad (impl 3) / a ragged last column range": ("wgrad", 3, lambda r, w: r["kernel"] == "x6" and r["nsplit"] >= 2 and _Wo(w) % r["nsplit"] != 0 and _tiles(r, w) > 256),
    "mfma wgrad (impl 1) / more tiles than workgroups, uneven": ("wgrad", 1, lambda r, w: r["kernel"] == "mfma" and w[1] * r["nstrips"] > r["grid"] and (w[1] * r["nstrips"]) % r["grid"] != 0),
})
for _k, _p in _pw("pw4").items():
    CLASSES["pw4 backward / " + _k] = ("bwd", 4, _p)
CLASSES["pw4 backward / 8 waves per sample"] = ("bwd", 4, lambda r, w: r["kernel"] == "pw4" and r["wps"] == 8)
CLASSES["pw4 backward / 1025 samples: handed to the general H3 form"] = ("bwd", 4, lambda r, w: r["kernel"] == "pw-x6-h3" and w[1] == 1025 and w[3] == 25)
for _k, _p in _pw("pf4").items():
    CLASSES["pf4 forward / " + _k] = ("fwd", 4, _p)
CLASSES["pf4 forward / 1025 samples"] = ("fwd", 4, lambda r, w: r["kernel"] == "pf4" and w[1] == 1025 and w[3] == 25)
PW_CLASSES = {c for c in CLASSES if c.startswith(("pw4", "pf4"))}


def _runs(*pairs):
    """(class, ...) -> ((op, impl, class), ...) with op and impl read off the class."""
    return tuple((CLASSES[c][0], CLASSES[c][1], c) for c in pairs)


_F, _B = "cw4 forward 25->32 + skip / ", "cw4 backward-data 32->25 / "
_WN, _WM, _WU = "wg4 normConv / ", "wg4 mirrored-pad reducer / ", "wg4 unpadded reducer / "
# name, N, (Hi, Wi, Ti), Cin, Cout, pad, reflect, relu, gate, skip, runs.  Rows of one geometry stand together: they share their inputs and their oracle (inputs(), GROUPS)
CONV_ROWS = [
    # normConv 25 -> 32 + skip at the shipped extents: cw4 forward, strip (impl 2), wg4 / x6 / mfma backward-filter
    ("normConv 22x22x9, N = 24", 24, (22, 22, 9), 25, 32, SAME, 0, 0, 0, 1,
     _runs(_WN + "SR of 2 or 3 with a short last strip", "x6 wgrad (impl 3) / runs of several rows across patches, uneven", "mfma wgrad (impl 1) / more tiles than workgroups, uneven")),
    ("normConv 22x22x9, N = 32", 32, (22, 22, 9), 25, 32, SAME, 0, 0, 0, 1, _runs(_F + "SR of 6 or 8 with a short last strip")),
    ("normConv 22x22x9, N = 64", 64, (22, 22, 9), 25, 32, SAME, 0, 0, 0, 1, _runs(_F + "SR = 11: two strips")),
    ("normConv 22x22x9, N = 128 (shipped)", 128, (22, 22, 9), 25, 32, SAME, 0, 0, 0, 1,
     _runs(_F + "shipped: N = 128, one strip of all 22 rows per column range, grid 256", "strip (impl 2) / SR >= 8", _WN + "N = 128: two strips of half the rows")),
    ("normConv 22x22x9, N = 256", 256, (22, 22, 9), 25, 32, SAME, 0, 0, 0, 1,
     _runs(_F + "N = 256: one strip per column range, two workgroups per compute unit slot", _WN + "N = 256: all rows in one strip, the last batch wg4 takes")),
    ("normConv 22x22x9, N = 257", 257, (22, 22, 9), 25, 32, SAME, 0, 0, 0, 1,
     _runs(_F + "N = 256: one strip per column range, two workgroups per compute unit slot", _WN + "N = 257: handed to the general x6 kernel")),
    # its backward-data 32 -> 25
    ("bwd-data of normConv 22x22x9, N = 43", 43, (22, 22, 9), 32, 25, SAME, 0, 0, 0, 0, _runs(_B + "SR of 6 or 8 with a short last strip")),
    ("bwd-data of normConv 22x22x9, N = 64", 64, (22, 22, 9), 32, 25, SAME, 0, 0, 0, 0, _runs(_B + "SR = 11: two strips")),
    ("bwd-data of normConv 22x22x9, N = 128 (shipped)", 128, (22, 22, 9), 32, 25, SAME, 0, 0, 0, 0, _runs(_B + "shipped: N = 128, one strip of all 22 rows per column range, grid 256")),
    ("bwd-data of normConv 22x22x9, N = 256", 256, (22, 22, 9), 32, 25, SAME, 0, 0, 0, 0, _runs(_B + "N = 256: one strip per column range, two workgroups per compute unit slot")),
    # other widths (patch sizes 24 and 17)
    ("normConv 9x30x9", 2, (9, 30, 9), 25, 32, SAME, 0, 0, 0, 1, _runs(_F + "a 30-wide row at depth 9: three column ranges")),
    ("bwd-data of normConv 9x30x9", 2, (9, 30, 9), 32, 25, SAME, 0, 0, 0, 0, _runs(_B + "a 30-wide row at depth 9: three column ranges")),
    ("normConv 9x23x9", 2, (9, 23, 9), 25, 32, SAME, 0, 0, 0, 1, _runs(_F + "declines on items (an odd width), a piece-ring kernel takes over")),
    ("bwd-data of normConv 9x23x9", 2, (9, 23, 9), 32, 25, SAME, 0, 0, 0, 0, _runs(_B + "declines on items (an odd width), a piece-ring kernel takes over")),
    ("normConv 16x23x9, N = 128", 128, (16, 23, 9), 25, 32, SAME, 0, 0, 0, 1, _runs("pstrip / SR >= 8")),
    # the reducers: mirrored pads 9 -> 7 (shipped), and 5 -> 3 for the large batches
    ("mirrored-pad reducer 22x22x9 -> 7, N = 128 (shipped)", 128, (22, 22, 9), 32, 32, MIRROR, 1, 1, 0, 0,
     _runs("pp fwd / SR >= 8, two staging items per thread", _WM + "N = 128: two strips of half the rows")),
    ("mirrored-pad reducer 22x22x5 -> 3, N = 24", 24, (22, 22, 5), 32, 32, MIRROR, 1, 1, 0, 0, _runs(_WM + "SR of 2 or 3 with a short last strip")),
    ("mirrored-pad reducer 22x22x5 -> 3, N = 256", 256, (22, 22, 5), 32, 32, MIRROR, 1, 1, 0, 0,
     _runs("pp fwd / SR >= 8, two staging items per thread", _WM + "N = 256: all rows in one strip, the last batch wg4 takes")),
    ("mirrored-pad reducer 22x22x5 -> 3, N = 257", 257, (22, 22, 5), 32, 32, MIRROR, 1, 1, 0, 0,
     _runs("pp fwd / SR >= 8, two staging items per thread", _WM + "N = 257: handed to the general x6 kernel")),
    # the unpadded reducers: 7 -> 5 (shipped), 5 -> 3 for the large batches, an odd row count for the short last strip
    ("unpadded reducer 22x22x7 -> 20x20x5, N = 128 (shipped)", 128, (22, 22, 7), 32, 32, VALID, 0, 1, 0, 0,
     _runs("pp fwd / SR >= 8, three staging items per thread", _WU + "N = 128: two strips of half the rows")),
    ("unpadded reducer 19x20x5 -> 17x18x3, N = 24", 24, (19, 20, 5), 32, 32, VALID, 0, 1, 0, 0, _runs(_WU + "SR of 2 or 3 with a short last strip")),
    ("unpadded reducer 20x20x5 -> 18x18x3, N = 256", 256, (20, 20, 5), 32, 32, VALID, 0, 1, 0, 0,
     _runs("pp fwd / SR >= 8, two staging items per thread", _WU + "N = 256: all rows in one strip, the last batch wg4 takes")),
    ("unpadded reducer 20x20x5 -> 18x18x3, N = 257", 257, (20, 20, 5), 32, 32, VALID, 0, 1, 0, 0,
     _runs("pp fwd / SR >= 8, two staging items per thread", _WU + "N = 257: handed to the general x6 kernel")),
    # gated backward-data of the reducers (full correlation) at the shipped batch
    ("bwd-data of the unpadded reducer 7 -> 5: full 32->32 gated, N = 128", 128, (20, 20, 5), 32, 32, (2, 2, 2), 0, 0, 1, 0, _runs("pp bwd / SR >= 8, two staging items per thread")),
    # depth 13: column halves in wg4, three and four column ranges in pp
    ("T=13 normConv 22x22x13, N = 128", 128, (22, 22, 13), 25, 32, SAME, 0, 0, 0, 1,
     _runs(_WN + "depth 13, column halves, N = 128: all rows in one strip, the last batch wg4 takes")),
    ("T=13 normConv 22x22x13, N = 129", 129, (22, 22, 13), 25, 32, SAME, 0, 0, 0, 1, _runs(_WN + "depth 13, N = 129: handed to the general x6 kernel")),
    ("mirrored-pad reducer 22x22x13 -> 11, N = 128", 128, (22, 22, 13), 32, 32, MIRROR, 1, 1, 0, 0,
     _runs(_WM + "depth 13, column halves, N = 128: all rows in one strip, the last batch wg4 takes")),
    ("mirrored-pad reducer 22x22x13 -> 11, N = 129", 129, (22, 22, 13), 32, 32, MIRROR, 1, 1, 0, 0, _runs(_WM + "depth 13, N = 129: handed to the general x6 kernel")),
    ("bwd-data of the T=13 normConv, gated, 22x22x13, N = 64", 64, (22, 22, 13), 32, 25, SAME, 0, 0, 1, 0, _runs("pp bwd / SR >= 8, three staging items per thread")),
    ("bwd-data of a T=13 normConv, gated, 9x36x13", 2, (9, 36, 13), 32, 25, SAME, 0, 0, 1, 0, _runs("pp / a 36-wide row at depth 13: three column ranges")),
    ("bwd-data of a T=13 normConv, gated, 9x44x13", 2, (9, 44, 13), 32, 25, SAME, 0, 0, 1, 0, _runs("pp / a 44-wide row at depth 13: four column ranges")),
    ("mirrored-pad reducer 9x36x13 -> 11", 2, (9, 36, 13), 32, 32, MIRROR, 1, 1, 0, 0, _runs("pp forward / three and four column ranges")),
    # the general backward-filter kernel on a ragged last column range: 23 columns in two ranges of 12 and 11, 270 (patch, row, range) tiles
    ("T=13 normConv 9x23x13, N = 15", 15, (9, 23, 13), 25, 32, SAME, 0, 0, 0, 1, _runs("x6 wgrad (impl 3) / a ragged last column range")),
]

_P, _Q = "pw4 backward / ", "pf4 forward / "
# name, samples, voxels per sample, D, runs
PW_ROWS = [
    ("pair, 128 x 4356 (shipped)", 128, 4356, 25,
     _runs(_Q + "shipped: 128 samples of 4 356 voxels (137 tiles, the last of 4 voxels), 8 waves per sample",
           _P + "shipped: 128 samples of 4 356 voxels (137 tiles, the last of 4 voxels), 8 waves per sample", _P + "8 waves per sample")),
    ("pair, 128 x 260", 128, 260, 25, _runs(_Q + "8 waves per sample over 8k + 1 tiles, the last of 4 voxels", _P + "8 waves per sample over 8k + 1 tiles, the last of 4 voxels")),
    ("pair, 512 x 100", 512, 100, 25, _runs(_Q + "512 samples: 2 waves per sample", _P + "512 samples: 2 waves per sample")),
    ("pair, 1024 x 40", 1024, 40, 25, _runs(_Q + "1024 samples: 1 wave per sample, the last batch pw4 takes", _P + "1024 samples: 1 wave per sample, the last batch pw4 takes")),
    ("pair, 1025 x 40", 1025, 40, 25, _runs(_Q + "1025 samples", _P + "1025 samples: handed to the general H3 form")),
]

# the hand-overs: (row at N, row at N + 1).  Both sides meet their bars (each is a row); on the samples they share, forward results of one kernel are equal bit for bit
HANDOVERS = [("normConv 22x22x9, N = 256", "normConv 22x22x9, N = 257"),
             ("mirrored-pad reducer 22x22x5 -> 3, N = 256", "mirrored-pad reducer 22x22x5 -> 3, N = 257"),
             ("unpadded reducer 20x20x5 -> 18x18x3, N = 256", "unpadded reducer 20x20x5 -> 18x18x3, N = 257"),
             ("T=13 normConv 22x22x13, N = 128", "T=13 normConv 22x22x13, N = 129"),
             ("mirrored-pad reducer 22x22x13 -> 11, N = 128", "mirrored-pad reducer 22x22x13 -> 11, N = 129"),
             ("pair, 1024 x 40", "pair, 1025 x 40")]


def row_by_name(name):
    return next(r for r in CONV_ROWS + PW_ROWS if r[0] == name)


def group_key(row):
    """Rows of one geometry (everything but N) draw the same numbers: the row at N is the first N samples of the largest one."""
    return repr(row[2:10])


def group_max_n(row):
    return max(r[1] for r in CONV_ROWS if group_key(r) == group_key(row))


_drawn = {}


def inputs(row):
    """{x, w, bias, gate, skip, dy, ygate} of a conv row, fp32, from default_rng(crc32(geometry), k) alone; gate / skip None where the row has none, ygate (the
    layer's own output, whose sign masks dY in the backward-filter) None without a ReLU.  One group is kept."""
    key = group_key(row)
    if key not in _drawn:
        _drawn.clear()
        name, _, hwt, Cin, Cout, pad, reflect, relu, gate, skip = row[:10]
        n, ho, seed = group_max_n(row), out_dims(hwt, pad), zlib.crc32(key.encode())
        draw = lambda k, shape: np.random.default_rng([seed, k]).standard_normal(size=shape, dtype=np.float32)
        _drawn[key] = dict(x=draw(0, (n,) + tuple(hwt) + (Cin,)), w=draw(1, K3 + (Cin, Cout)) / np.float32(np.sqrt(27 * Cin)), bias=draw(2, (Cout,)),
                           gate=draw(3, (n,) + tuple(hwt) + (Cin,)) if gate else None, skip=draw(4, (n,) + ho + (Cout,)) if skip else None,
                           dy=draw(5, (n,) + ho + (Cout,)), ygate=draw(6, (n,) + ho + (Cout,)) if relu else None)
    N = row[1]
    return {k: (v[:N] if v is not None and k not in ("w", "bias") else v) for k, v in _drawn[key].items()}


_pw_drawn = {}


def pw_inputs(row):
    """(x, w1, b1, w2, b2, d_dec, d_skip) of a pointwise row; rows of one (voxels per sample, D) share their numbers, the row of fewer samples being the first samples
    of the larger one.  The comparison is un-gated and d relu is a step: a voxel with a pre-activation below 1e-4 -- ten times the rounding error of its own fp32
    evaluation on these inputs -- is drawn again (tests/test_gpu_parity.py::_fused_pointwise_case, decided_gates)."""
    name, nsamp, vps, D = row[:4]
    key = (vps, D)
    if key not in _pw_drawn:
        _pw_drawn.clear()
        nvox = max(r[1] for r in PW_ROWS if (r[2], r[3]) == key) * vps
        rng = np.random.default_rng([vps, D])
        x = rng.standard_normal(size=(nvox, 32), dtype=np.float32)
        w1 = (rng.normal(size=(32, 256)) / np.sqrt(32)).astype(np.float32)
        b1 = rng.normal(scale=0.3, size=256).astype(np.float32)
        w1d = w1.astype(np.float64)
        todo = np.arange(nvox)
        while todo.size:
            amb = (np.abs(x[todo].astype(np.float64) @ w1d + b1) < 1e-4).any(axis=1)
            todo = todo[amb]
            x[todo] = rng.standard_normal(size=(todo.size, 32), dtype=np.float32)
        w2 = (rng.normal(size=(256, D)) / 16).astype(np.float32)
        b2 = rng.normal(scale=0.3, size=D).astype(np.float32)
        ddec = rng.standard_normal(size=(nvox, D), dtype=np.float32)
        dskip = rng.standard_normal(size=(nvox, 32), dtype=np.float32)
        _pw_drawn[key] = (x, w1, b1, w2, b2, ddec, dskip)
    x, w1, b1, w2, b2, ddec, dskip = _pw_drawn[key]
    n = nsamp * vps
    return x[:n], w1, b1, w2, b2, ddec[:n], dskip[:n]
