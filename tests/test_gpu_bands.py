"""Every writing entry point of include/probav_hip.h inside the arena of tests/bands.py: each buffer at exactly its declared byte length between
guard bands, run under the fills 0xFF and 0x00 and on plain tensors.  Bands untouched, inputs unchanged, outputs bitwise equal under every
fill, skipped rows holding their fill, and every byte-size argument passed once exactly (the size query's answer) and once at size - 1 with
the header's refusal and nothing touched.  Every comparison is bitwise.

What this cannot see: a read past the end of an input whose value never reaches the result (a halo load that is selected away AFTER the
load).  Nobody should read this module as a proof of in-bounds reads; it proves in-bounds WRITES at these shapes and results that are
functions of the arguments alone.

Every run is followed by one on a late stream (tests/bands.py, `_late_run`; tests/late_stream.py): the same launch on a stream that is still busy
with a delay, its inputs delivered behind the delay.  The result must be the first run's bit for bit -- every launch, memset, fork and join of an
entry point is on, or from, the stream it was given -- and the call must come back while the delay is still running: it only enqueues.
HOST_WAIT_EXEMPT lists the calls the header allows to wait; they are held to the first half alone.

Entry points of include/probav_hip.h that take a stream -> the test that holds them: STREAMED below (tests/test_bands_host.py holds the table to
the header).  Left out: nothing that writes device memory.  The host-only entries (engine create / destroy, set_impl, side_stream, the size, layout,
view, plan and profile queries, probav_debug_hidden_from_forward_kernel) write none.

Rows of tests/plan_cases.py: the classes with a short last strip or more than one column range run at their own N.  Skipped, because a
tensor of the row exceeds 64 MiB (SKIPPED_PLAN_ROWS, asserted against the table):
    normConv 22x22x9, N = 128 (shipped) / N = 256 / N = 257;  bwd-data of normConv 22x22x9, N = 128 (shipped) / N = 256;
    T=13 normConv 22x22x13, N = 128;  mirrored-pad reducer 22x22x13 -> 11, N = 128
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from probav_amd import synth
from tests import bands, plan_cases
from tests.test_gpu_parity import CONV_CASES, WGRAD_CASES, _geom, _out_dims

pytestmark = pytest.mark.gpu

F32, I32, I64, U8, U16, F64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.uint16, torch.float64


# entry point that takes a stream -> the test of this module that holds it (the two probav_gemm_* operators: tests/test_gpu_gemm_route.py)
STREAMED = {
    "probav_forward": "test_engine_one_piece",                            # training 0 / 1
    "probav_backward": "test_engine_one_piece",
    "probav_backward_split": "test_engine_split",                         # (+ probav_workspace_split)
    "probav_backward_input": "test_engine_split",
    "probav_weight_cache_build": "test_engine_weight_cache",
    "probav_forward_wc": "test_engine_weight_cache",
    "probav_backward_wc": "test_engine_weight_cache",
    "probav_optimizer_step_fused": "test_engine_fused_optimizer",
    "probav_optimizer_step_fused_guarded": "test_engine_fused_optimizer",
    "probav_wn_forward": "test_engine_weight_norm",
    "probav_wn_backward": "test_engine_weight_norm",
    "probav_debug_hidden": "test_engine_debug_hidden",
    "probav_conv3d_forward": "test_conv3d_forward",                       # and test_conv3d_plan_rows
    "probav_conv3d_wgrad": "test_conv3d_wgrad",                           # (+ probav_conv3d_wgrad_scratch_bytes) and test_conv3d_plan_rows
    "probav_pw_forward": "test_pointwise_pair",
    "probav_pw_backward": "test_pointwise_pair",                          # (+ its scratch query)
    "probav_shift_loss_forward": "test_losses",
    "probav_shift_loss_backward": "test_losses",
    "probav_shift_l1edge_forward": "test_losses",
    "probav_shift_l1edge_backward": "test_losses",
    "probav_revssim_forward": "test_losses",
    "probav_revssim_backward": "test_losses",
    "probav_nadam_step": "test_optimizer",
    "probav_grad_guard": "test_optimizer",
    "probav_nadam_step_guarded": "test_optimizer",
    "probav_clip_round": "test_clip_round",                               # and the harness's self-tests
    "probav_input_grad": "test_input_grad",
    "probav_score_moments": "test_scoring",
    "probav_score_select": "test_scoring",
    "probav_ssim_table": "test_scoring",
    "probav_ssim_select": "test_scoring",
    "probav_prep_count_nonzero": "test_prep_count_nonzero",
    "probav_prep_register": "test_prep_register",
    "probav_prep_xcorr_surface": "test_prep_xcorr_surface",
    "probav_prep_patches": "test_prep_patches",
    "probav_prep_register_masked": "test_prep_register_masked",
    "probav_prep_refine_masks": "test_prep_refine_masks",
    "probav_augment_batch": "test_augment_and_ensemble",
    "probav_ensemble_expand": "test_augment_and_ensemble",
    "probav_ensemble_reduce": "test_augment_and_ensemble",
    "probav_tile_blend": "test_tile_blend",
    "probav_baseline_upscale_mean": "test_baseline",                      # both modes
    "probav_frame_windows_gather": "test_frame_windows",
    "probav_frame_windows_reduce": "test_frame_windows",
    "probav_window_counts": "test_crops",
    "probav_crop_batch": "test_crops",
    "probav_fusenet_forward": "test_fusenet",                             # (+ probav_fusenet_workspace_bytes)
    "probav_fusenet_backward": "test_fusenet",
    "probav_mfma_probe": "test_mfma_probe",                               # the measurement aid's `sink`
    "probav_mfma_probe_shape": "test_mfma_probe",
}

# The calls that may wait on the host, allocate or free: skipped for the late run's host-wait check, never for its comparison.  Each row quotes the sentence of
# include/probav_hip.h (Conventions) that grants it.  entry point -> (the header's sentence, which of its calls: args of the call, calls of the session before it -> bool)
_FIRST = "an engine's first call that launches with its layer table (a pass, a weight-norm or optimizer call) uploads that table, a few KB, once"
_SINGLE_OP = ("the single-operator entries probav_conv3d_forward (impl 1-4), probav_pw_forward and probav_pw_backward pack their filter into a scratch the library owns: "
              "every such call waits for `stream` to drain and uploads its packing jobs with a blocking copy")
_AMAX = "their H3 form (impl 4, probav_conv3d_wgrad included) frees and allocates the library's amax table when a call needs more slots than any call before it"
_CAND = "probav_shift_loss_forward frees and allocates the library's candidate table when its batch times (2 border + 1)^2 exceeds that of every call before it"


def _first_of_its_engine(args, before):
    handle = lambda a: getattr(a[0], "value", a[0])
    return not any(handle(a) == handle(args) for n, a in before if n in _ENGINE_ENTRIES)


def _larger_than_before(entry, need):
    return lambda args, before: need(args) > max([need(a) for n, a in before if n == entry], default=0)


_ENGINE_ENTRIES = ("probav_forward", "probav_backward", "probav_backward_split", "probav_backward_input", "probav_weight_cache_build", "probav_forward_wc", "probav_backward_wc",
                   "probav_optimizer_step_fused", "probav_optimizer_step_fused_guarded", "probav_wn_forward", "probav_wn_backward")
HOST_WAIT_EXEMPT = dict(
    [(n, (_FIRST, _first_of_its_engine)) for n in _ENGINE_ENTRIES] +
    [("probav_conv3d_forward", (_SINGLE_OP, lambda args, before: args[7] >= 1)),
     ("probav_pw_forward", (_SINGLE_OP, lambda args, before: True)),
     ("probav_pw_backward", (_SINGLE_OP, lambda args, before: True)),
     ("probav_conv3d_wgrad", (_AMAX, lambda args, before: args[8] == 4 and _larger_than_before("probav_conv3d_wgrad", lambda a: a[0]._obj[0] if a[8] == 4 else 0)(args, before))),
     ("probav_shift_loss_forward", (_CAND, _larger_than_before("probav_shift_loss_forward", lambda a: a[3] * (2 * a[5] + 1) ** 2)))])


def _host_wait_exempt(calls, before):
    """bands.host_wait_exempt: the header's sentence if one of the late launch's calls may wait on the host.  before: every recorded call of the session ahead of them."""
    for i, (name, args) in enumerate(calls):
        row = HOST_WAIT_EXEMPT.get(name)
        if row and row[1](args, before + calls[:i]):
            return "%s: %s" % (name, row[0])
    return None


class _Recorded:
    """probav_amd._lib with every entry-point call noted (tests/late_stream.py, `recording`): how the late run knows which entry points a launch went through."""

    def __getattr__(self, name):
        from probav_amd import _lib
        return getattr(_lib, name)

    def lib(self):
        from probav_amd import _lib
        from tests import late_stream
        return late_stream.recording(_lib.lib())


def _L():
    return _Recorded()


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def S():
    return _L().current_stream()


def _f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(size=shape) * scale).astype(np.float32)


def _opt(name, a):
    return [] if a is None else [bands.inp(name, a)]


# ---- the harness proves itself on the device ---------------------------------------------------------------------------------------------
def test_harness_reports_a_planted_overrun(dev):
    """probav_clip_round with n = 1025 on an output carved 16 bytes (four floats) short: the last four floats land in the band behind it,
    inside the arena.  The harness must name exactly that buffer, side and byte range."""
    n = 1025
    x = _f32(np.random.default_rng(1), n, scale=300.0)
    bufs = [bands.inp("in", x), bands.out("out", F32, n - 4)]
    rep = bands.run(bufs, lambda t: _L().lib().probav_clip_round(P(t["in"]), P(t["out"]), n, ctypes.c_float(1.0), ctypes.c_float(65535.0), S()), dev,
                    plain=False)
    print(rep)
    assert sorted((v.buffer, v.side, v.fill) for v in rep.violations) == [("out", "after", "0x00"), ("out", "after", "0xFF"), ("out", "after", "late")]
    found = {v.fill: (v.first, v.last) for v in rep.violations}
    assert found["0xFF"] == (0, 15) and found["late"] == (0, 15)            # four floats in [1, 65535]: no byte of theirs is 0xFF (the late run fills with 0xFF)
    assert found["0x00"][1] == 15 and found["0x00"][0] <= 3            # their low mantissa bytes may be zero, their exponent bytes are not


def test_harness_reports_a_planted_unwritten_element(dev):
    """An `out` of n + 1 floats handed to probav_clip_round with n: the last element is never written and holds the fill; the A / B
    comparison must report those four bytes."""
    n = 255
    x = _f32(np.random.default_rng(2), n, scale=300.0)
    bufs = [bands.inp("in", x), bands.out("out", F32, n + 1)]
    rep = bands.run(bufs, lambda t: _L().lib().probav_clip_round(P(t["in"]), P(t["out"]), n, ctypes.c_float(0.0), ctypes.c_float(65535.0), S()), dev,
                    plain=False)
    print(rep)
    assert [(v.buffer, v.side, v.first, v.last) for v in rep.violations] == [("out", "differs", 4 * n, 4 * n + 3)]


def test_harness_reports_a_planted_launch_on_the_null_stream(dev):
    """probav_clip_round handed a NULL stream.  In the ordinary runs the null stream is the current one and nothing shows.  In the late run the kernel does not wait for the
    delay: it writes `out` (inside the arena, from the valid input the run before left there) before the fill and the inputs arrive on the late stream, and the fill erases it.
    The harness must report exactly that: `out` differs on the late run, nothing else."""
    n = 1025
    x = _f32(np.random.default_rng(3), n, scale=300.0)
    bufs = [bands.inp("in", x), bands.out("out", F32, n)]
    rep = bands.run(bufs, lambda t: _L().lib().probav_clip_round(P(t["in"]), P(t["out"]), n, ctypes.c_float(1.0), ctypes.c_float(65535.0), None), dev)
    print(rep)
    assert [(v.buffer, v.side, v.fill, v.first, v.last) for v in rep.violations] == [("out", "differs", "0xFF vs late", 0, 4 * n - 1)]      # (values in [1, 65535]: no byte is 0xFF)


def test_harness_reports_a_planted_host_wait(dev):
    """A launch that synchronises its stream before it returns: correct bits, but the call comes back only after the delay -- also after ten times the delay."""
    n = 255
    x = _f32(np.random.default_rng(4), n, scale=300.0)
    bufs = [bands.inp("in", x), bands.out("out", F32, n)]

    def call(t):
        rc = _L().lib().probav_clip_round(P(t["in"]), P(t["out"]), n, ctypes.c_float(0.0), ctypes.c_float(65535.0), S())
        torch.cuda.current_stream().synchronize()
        return rc
    rep = bands.run(bufs, call, dev)
    print(rep)
    assert [(v.buffer, v.side, v.fill) for v in rep.violations] == [("(call)", "sync", "late")]


# ---- single convolutions ---------------------------------------------------------------------------------------------------------------
def _conv_bufs(N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip, seed, bias=True):
    rng = np.random.default_rng(seed)
    ho = _out_dims(hwt, k, pad, reflect)
    x = _f32(rng, N, *hwt, Cin)
    w = _f32(rng, *k, Cin, Cout, scale=1.0 / np.sqrt(np.prod(k) * Cin))
    b = _f32(rng, Cout) if bias else None
    gate = _f32(rng, *x.shape) if use_gate else None
    skip = _f32(rng, N, *ho, Cout) if use_skip else None
    g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    per = int(np.prod(ho)) * Cout
    bufs = [bands.inp("x", x)] + _opt("gate", gate) + [bands.inp("w", w)] + _opt("bias", b) + _opt("skip", skip) + [bands.out("y", F32, N * per, lead_count=per)]
    return g, bufs


def _conv_forward(dev, g, bufs, impl):
    call = lambda t: _L().lib().probav_conv3d_forward(ctypes.byref(g), P(t["x"]), P(t.get("gate")), P(t["w"]), P(t.get("bias")), P(t.get("skip")), P(t["y"]), impl, S())
    rep = bands.run(bufs, call, dev)
    if impl >= 1 and all(rc == _L().PROBAV_EINVAL for rc in rep.rcs.values()):
        assert all(v.side == "rc" for v in rep.violations), str(rep)            # a refused call writes nothing, bands included
        pytest.skip("geometry not covered by this MFMA kernel (the engine falls back)")
    assert rep.ok(), str(rep)


@pytest.mark.parametrize("impl", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv3d_forward(dev, case, impl):
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip = case
    g, bufs = _conv_bufs(N, hwt, Cin, Cout, k, pad, reflect, relu, use_gate, use_skip, zlib.crc32(name.encode()))
    _conv_forward(dev, g, bufs, impl)


def _wgrad_bufs(N, hwt, Cin, Cout, k, pad, reflect, relu, seed, impl):
    rng = np.random.default_rng(seed)
    ho = _out_dims(hwt, k, pad, reflect)
    x, dy = _f32(rng, N, *hwt, Cin), _f32(rng, N, *ho, Cout)
    gate = _f32(rng, *dy.shape) if relu else None
    g = _geom(N, hwt[0], hwt[1], hwt[2], Cin, ho[0], ho[1], ho[2], Cout, k, pad, reflect, relu)
    nbytes = _L().lib().probav_conv3d_wgrad_scratch_bytes(ctypes.byref(g), impl)
    bufs = [bands.inp("x", x), bands.inp("dy", dy)] + _opt("gate", gate) + [bands.out("dw", F32, int(np.prod(k)) * Cin * Cout), bands.out("db", F32, Cout),
                                                                            bands.scratch("scratch", nbytes)]
    return g, bufs, nbytes


def _conv_wgrad(dev, g, bufs, nbytes, impl):
    if impl in (1, 3, 4) and nbytes == 0:
        pytest.skip("geometry not covered by this MFMA backward-filter kernel (the engine falls back)")
    call = lambda nb: (lambda t: _L().lib().probav_conv3d_wgrad(ctypes.byref(g), P(t["x"]), P(t["dy"]), P(t.get("gate")), P(t["dw"]), P(t["db"]), P(t["scratch"]), nb,
                                                                  impl, S()))
    bands.check(bufs, call(nbytes), dev)
    bands.check_refusal(bufs, call(nbytes - 1), dev, _L().PROBAV_ENOSPACE)


@pytest.mark.parametrize("impl", [0, 1, 3, 4])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv3d_wgrad(dev, case, impl):
    name, N, hwt, Cin, Cout, k, pad, reflect, relu, _, _ = case
    g, bufs, nbytes = _wgrad_bufs(N, hwt, Cin, Cout, k, pad, reflect, relu, zlib.crc32(name.encode()) + 1, impl)
    _conv_wgrad(dev, g, bufs, nbytes, impl)


PLAN_KEYS = ("short last strip", "column range", "column halves")
LIMIT = 64 << 20


def _row_bytes(row):
    name, N, hwt, Cin, Cout, pad = row[:6]
    ho = plan_cases.out_dims(hwt, pad)
    return 4 * N * max(int(np.prod(hwt)) * Cin, int(np.prod(ho)) * Cout)


PLAN_RUNS = [(row, op, impl, cls) for row in plan_cases.CONV_ROWS for op, impl, cls in row[10] if any(k in cls for k in PLAN_KEYS)]
SKIPPED_PLAN_ROWS = ["normConv 22x22x9, N = 128 (shipped)", "normConv 22x22x9, N = 256", "normConv 22x22x9, N = 257", "bwd-data of normConv 22x22x9, N = 128 (shipped)",
                     "bwd-data of normConv 22x22x9, N = 256", "T=13 normConv 22x22x13, N = 128", "mirrored-pad reducer 22x22x13 -> 11, N = 128"]
PLAN_RUNS_SMALL = [r for r in PLAN_RUNS if _row_bytes(r[0]) <= LIMIT]


def test_the_skipped_plan_rows_are_the_listed_ones():
    assert sorted({r[0][0] for r in PLAN_RUNS if _row_bytes(r[0]) > LIMIT}) == sorted(SKIPPED_PLAN_ROWS)
    assert len(PLAN_RUNS_SMALL) >= 10


@pytest.mark.parametrize("run", PLAN_RUNS_SMALL, ids=["%s / %s" % (r[0][0], r[3]) for r in PLAN_RUNS_SMALL])
def test_conv3d_plan_rows(dev, run):
    row, op, impl, cls = run
    name, N, hwt, Cin, Cout, pad, reflect, relu, gate, skip = row[:10]
    seed = zlib.crc32(name.encode()) + 2
    if op == "wgrad":
        g, bufs, nbytes = _wgrad_bufs(N, tuple(hwt), Cin, Cout, plan_cases.K3, tuple(pad), reflect, relu, seed, impl)
        _conv_wgrad(dev, g, bufs, nbytes, impl)
    else:
        g, bufs = _conv_bufs(N, tuple(hwt), Cin, Cout, plan_cases.K3, tuple(pad), reflect, relu, gate, skip, seed, bias=(op == "fwd"))
        _conv_forward(dev, g, bufs, impl)


# ---- fused pointwise pair ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [2, 3, 4])
@pytest.mark.parametrize("D", [1, 24, 25, 26])
@pytest.mark.parametrize("nvox,vps", [(32, 0), (1000, 0), (7 * 33, 33), (5 * 1640, 1640), (1030 * 40, 40)])
def test_pointwise_pair(dev, nvox, vps, D, impl):
    L = _L()
    rng = np.random.default_rng([nvox, D])
    x, w1, b1 = _f32(rng, nvox, 32), _f32(rng, 32, 256, scale=1 / np.sqrt(32)), _f32(rng, 256, scale=0.3)
    w2, b2 = _f32(rng, 256, D, scale=1 / 16), _f32(rng, D, scale=0.3)
    ddec, dskip = _f32(rng, nvox, D), _f32(rng, nvox, 32)
    lead = (vps or nvox)
    ins = [bands.inp("x", x), bands.inp("w1", w1), bands.inp("b1", b1), bands.inp("w2", w2)]
    for b in ins[:1]:
        b.lead = lead * 32 * 4
    fwd = ins + [bands.inp("b2", b2), bands.out("dec", F32, nvox * D, lead_count=lead * D)]
    bands.check(fwd, lambda t: L.lib().probav_pw_forward(P(t["x"]), P(t["w1"]), P(t["b1"]), P(t["w2"]), P(t["b2"]), P(t["dec"]), nvox, vps, D, impl, S()), dev)
    nbytes = L.lib().probav_pw_backward_scratch_bytes(D)
    bwd = ins + [bands.inp("d_dec", ddec), bands.inp("d_skip", dskip), bands.out("dx", F32, nvox * 32, lead_count=lead * 32), bands.out("dw1", F32, 32 * 256),
                 bands.out("db1", F32, 256), bands.out("dw2", F32, 256 * D), bands.out("db2", F32, D), bands.scratch("scratch", nbytes)]
    call = lambda nb: (lambda t: L.lib().probav_pw_backward(P(t["x"]), P(t["d_dec"]), P(t["d_skip"]), P(t["w1"]), P(t["b1"]), P(t["w2"]), P(t["dx"]), P(t["dw1"]),
                                                            P(t["db1"]), P(t["dw2"]), P(t["db2"]), P(t["scratch"]), nb, nvox, vps, D, impl, S()))
    bands.check(bwd, call(nbytes), dev)
    bands.check_refusal(bwd, call(nbytes - 1), dev, L.PROBAV_ENOSPACE)


# ---- engine ------------------------------------------------------------------------------------------------------------------------------
ENGINE_CFGS = [(7, 1), (9, 1), (13, 1), (9, 3)]            # (T, in_channels) at P = 16
ENGINE_IMPLS = [0, 3, 4]
_models, _stale = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _give_the_device_back():
    """The engines and the stale state live as long as the module's tests need them, no longer: the modules that run afterwards get the memory back."""
    from tests import late_stream
    bands.host_wait_exempt = _host_wait_exempt
    yield
    bands.host_wait_exempt = None
    print("\n" + late_stream.summary())
    _models.clear()
    _stale.clear()
    if torch.cuda.is_available():
        bands.release("cuda:0")


def _engine(dev, T, C, impl):
    """(handle, params as a numpy array, layers) of the shipped architecture at T frames, C input channels; parameters moved off their initial values."""
    from probav_amd.modelsTF import WDSRConv3D
    if (T, C) not in _models:
        m = WDSRConv3D("bands", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, T, 16, C == 1, seed=5).to(dev)
        flat = m.flat.detach().cpu().numpy().copy()
        flat += (0.05 * np.random.default_rng(T * 10 + C).standard_normal(flat.shape)).astype(np.float32)
        _models[(T, C)] = (m, flat)
    m, flat = _models[(T, C)]
    h = m._handle()
    _L().check(_L().lib().probav_engine_set_impl(h, impl), "probav_engine_set_impl")
    return h, flat, m.layers


def _batch(T, C, B, seed=3):
    x, _, _ = synth.synth_batch(B, seed=seed, numImgLR=T, inChannels=C)
    dy = _f32(np.random.default_rng(seed + 1), B, 48, 48, 1)
    return np.ascontiguousarray(x, dtype=np.float32), dy


def _sizes(h, B):
    lib = _L().lib()
    saved, scr = ctypes.c_size_t(), ctypes.c_size_t()
    _L().check(lib.probav_workspace_split(h, B, ctypes.byref(saved), ctypes.byref(scr)), "probav_workspace_split")
    n0, n1, nwc = lib.probav_workspace_bytes(h, B, 0), lib.probav_workspace_bytes(h, B, 1), lib.probav_weight_cache_bytes(h)
    assert n1 == saved.value + scr.value and n0 > 0 and nwc > 0
    return n0, n1, saved.value, scr.value, nwc


def _stale_state(dev, T, C, impl):
    """Workspace and weight cache as a complete training pass at batch 3 leaves them, inputs and parameters scaled by 2^10: what a batch-1 call finds in a reused buffer
    (amax slots of a larger magnitude, slabs of a larger batch)."""
    key = (T, C, impl)
    if key not in _stale:
        _stale.clear()
        lib = _L().lib()
        h, flat, _ = _engine(dev, T, C, impl)
        _, n1, _, _, nwc = _sizes(h, 3)
        x, dy = _batch(T, C, 3, seed=11)
        p, xd, dyd = (torch.as_tensor(a * np.float32(1024.0)).to(dev) for a in (flat, x, dy))
        ws, wc = torch.zeros(n1, dtype=U8, device=dev), torch.zeros(nwc, dtype=U8, device=dev)
        y, grads = torch.empty(3 * 48 * 48, device=dev), torch.empty(flat.size, device=dev)
        _L().check(lib.probav_weight_cache_build(h, P(p), P(wc), nwc, S()), "probav_weight_cache_build")
        _L().check(lib.probav_forward_wc(h, P(p), P(xd), P(y), P(ws), n1, 3, 1, P(wc), nwc, S()), "probav_forward_wc")
        _L().check(lib.probav_backward_wc(h, P(p), P(dyd), P(grads), P(ws), n1, 3, P(wc), nwc, S()), "probav_backward_wc")
        torch.cuda.synchronize()
        _stale[key] = (ws, wc)
    return _stale[key]


def _fills(dev, T, C, impl, B, sizes):
    """0xFF, 0x00, and at batch 1 the stale state: {buffer name: bytes} for the buffers named in `sizes` = {name: (offset into the stale workspace | 'wc', nbytes)}."""
    if B != 1:
        return bands.FILLS
    ws, wc = _stale_state(dev, T, C, impl)
    preset = {n: (wc[:nb] if off == "wc" else ws[off:off + nb]) for n, (off, nb) in sizes.items()}
    return bands.FILLS + (bands.Fill(0xFF, preset=preset, label="stale"),)


ENGINE_PARAMS = [(T, C, B, impl) for T, C in ENGINE_CFGS for B in (1, 3) for impl in ENGINE_IMPLS]
engine_cases = pytest.mark.parametrize("T,C,B,impl", ENGINE_PARAMS)


def _io(flat, x, dy, B):
    ins = [bands.inp("params", flat), bands.inp("x", x)] + ([] if dy is None else [bands.inp("dy", dy)])
    return ins, bands.out("y", F32, B * 48 * 48, lead_count=48 * 48)


@engine_cases
def test_engine_one_piece(dev, T, C, B, impl):
    L, lib = _L(), _L().lib()
    h, flat, _ = _engine(dev, T, C, impl)
    n0, n1, saved, _, _ = _sizes(h, B)
    x, dy = _batch(T, C, B)
    for training, nws in ((0, n0), (1, saved)):
        ins, y = _io(flat, x, None, B)
        bufs = ins + [y, bands.scratch("ws", nws)]
        fwd = lambda nb: (lambda t: lib.probav_forward(h, P(t["params"]), P(t["x"]), P(t["y"]), P(t["ws"]), nb, B, training, S()))
        bands.check(bufs, fwd(nws), dev, fills=_fills(dev, T, C, impl, B, {"ws": (0, nws)}))
        bands.check_refusal(bufs, fwd(nws - 1), dev, L.PROBAV_ENOSPACE)
    ins, y = _io(flat, x, dy, B)
    bufs = ins + [y, bands.out("grads", F32, flat.size), bands.scratch("ws", n1)]

    def step(t):
        rc = lib.probav_forward(h, P(t["params"]), P(t["x"]), P(t["y"]), P(t["ws"]), n1, B, 1, S())
        return rc or lib.probav_backward(h, P(t["params"]), P(t["dy"]), P(t["grads"]), P(t["ws"]), n1, B, S())
    bands.check(bufs, step, dev, fills=_fills(dev, T, C, impl, B, {"ws": (0, n1)}))
    bands.check_refusal(bufs, lambda t: lib.probav_backward(h, P(t["params"]), P(t["dy"]), P(t["grads"]), P(t["ws"]), n1 - 1, B, S()), dev, L.PROBAV_ENOSPACE)


@engine_cases
def test_engine_split(dev, T, C, B, impl):
    L, lib = _L(), _L().lib()
    h, flat, _ = _engine(dev, T, C, impl)
    _, _, saved, scr, _ = _sizes(h, B)
    x, dy = _batch(T, C, B)
    ins, y = _io(flat, x, dy, B)
    bufs = ins + [y, bands.out("grads", F32, flat.size), bands.out("grads_in", F32, flat.size), bands.out("dx", F32, x.size, lead_count=x[0].size),
                  bands.scratch("saved", saved), bands.scratch("scratch", scr)]
    split = lambda t, a, b: lib.probav_backward_split(h, P(t["params"]), P(t["dy"]), P(t["grads"]), P(t["saved"]), a, P(t["scratch"]), b, B, None, 0, S())
    inpt = lambda t, a, b: lib.probav_backward_input(h, P(t["params"]), P(t["dy"]), P(t["grads_in"]), P(t["saved"]), a, P(t["scratch"]), b, B, None, 0, P(t["dx"]), S())

    def step(t):
        rc = lib.probav_forward(h, P(t["params"]), P(t["x"]), P(t["y"]), P(t["saved"]), saved, B, 1, S())
        return rc or split(t, saved, scr) or inpt(t, saved, scr)
    rep = bands.check(bufs, step, dev, fills=_fills(dev, T, C, impl, B, {"saved": (0, saved), "scratch": (saved, scr)}))
    assert torch.equal(rep.outputs["grads"], rep.outputs["grads_in"])          # the header: the same launches in the same order, the same bits
    for fn in (split, inpt):
        bands.check_refusal(bufs, lambda t: fn(t, saved - 1, scr), dev, L.PROBAV_ENOSPACE)
        bands.check_refusal(bufs, lambda t: fn(t, saved, scr - 1), dev, L.PROBAV_ENOSPACE)


@engine_cases
def test_engine_weight_cache(dev, T, C, B, impl):
    L, lib = _L(), _L().lib()
    h, flat, _ = _engine(dev, T, C, impl)
    n0, n1, saved, scr, nwc = _sizes(h, B)
    x, dy = _batch(T, C, B)
    ins, y = _io(flat, x, dy, B)
    bufs = ins + [y, bands.out("y_infer", F32, B * 48 * 48, lead_count=48 * 48), bands.out("grads", F32, flat.size), bands.out("grads_split", F32, flat.size),
                  bands.scratch("ws", n1), bands.scratch("ws_infer", n0), bands.scratch("scratch", scr), bands.scratch("wcache", nwc)]
    build = lambda t, nb: lib.probav_weight_cache_build(h, P(t["params"]), P(t["wcache"]), nb, S())
    fwd = lambda t, nw, nb, tr=1: lib.probav_forward_wc(h, P(t["params"]), P(t["x"]), P(t["y"]), P(t["ws"]), nw, B, tr, P(t["wcache"]), nb, S())
    bwd = lambda t, nw, nb: lib.probav_backward_wc(h, P(t["params"]), P(t["dy"]), P(t["grads"]), P(t["ws"]), nw, B, P(t["wcache"]), nb, S())
    split = lambda t, nb: lib.probav_backward_split(h, P(t["params"]), P(t["dy"]), P(t["grads_split"]), P(t["ws"]), saved, P(t["scratch"]), scr, B, P(t["wcache"]), nb, S())

    def step(t):
        return (build(t, nwc) or lib.probav_forward_wc(h, P(t["params"]), P(t["x"]), P(t["y_infer"]), P(t["ws_infer"]), n0, B, 0, P(t["wcache"]), nwc, S())
                or fwd(t, n1, nwc) or split(t, nwc) or bwd(t, n1, nwc))
    rep = bands.check(bufs, step, dev, fills=_fills(dev, T, C, impl, B, {"ws": (0, n1), "ws_infer": (0, n0), "scratch": (saved, scr), "wcache": ("wc", nwc)}))
    assert torch.equal(rep.outputs["grads"], rep.outputs["grads_split"]) and torch.equal(rep.outputs["y"], rep.outputs["y_infer"])
    for call in (lambda t: build(t, nwc - 1), lambda t: fwd(t, n1, nwc - 1), lambda t: bwd(t, n1, nwc - 1), lambda t: split(t, nwc - 1),
                 lambda t: fwd(t, saved - 1, nwc), lambda t: bwd(t, n1 - 1, nwc)):
        bands.check_refusal(bufs, call, dev, L.PROBAV_ENOSPACE)


def _ctl(scale, skip):
    return np.frombuffer(np.array([(scale, skip, 7, 2.5)], dtype=[("scale", "f4"), ("skip", "u4"), ("total", "u4"), ("norm", "f4")]).tobytes(), dtype=np.uint8).copy()


HYPER = [ctypes.c_float(v) for v in (1e-3, 0.9, 0.999, 1e-7, 0.5, 0.6, 1.2)]          # lr, beta1, beta2, eps, c_g, c_m, c_v


@pytest.mark.parametrize("T,C,impl", [(T, C, impl) for T, C in ENGINE_CFGS for impl in ENGINE_IMPLS])
def test_engine_fused_optimizer(dev, T, C, impl):
    """The fused steps update params / m / v (/ ema) in place and write the weight cache; the cache's contents are held through the forward pass that runs from it."""
    L, lib = _L(), _L().lib()
    h, flat, _ = _engine(dev, T, C, impl)
    n0, _, _, _, nwc = _sizes(h, 1)
    x, _ = _batch(T, C, 1)
    rng = np.random.default_rng(17)
    g, m, v = _f32(rng, flat.size, scale=1e-2), _f32(rng, flat.size, scale=1e-2), np.abs(_f32(rng, flat.size, scale=1e-4))
    fills = _fills(dev, T, C, impl, 1, {"wcache": ("wc", nwc), "ws": (0, n0)})

    def bufs(keep=None, guarded=False, ctl=None):
        io = lambda n, a: bands.Buf(n, F32, "inout", init=a, keep=keep)
        b = [io("params", flat), bands.inp("grads", g), io("m", m), io("v", v), bands.inp("x", x), bands.out("y", F32, 48 * 48), bands.scratch("ws", n0),
             bands.scratch("wcache", nwc)]
        return b + ([io("ema", flat * np.float32(0.5)), bands.inp("ctl", ctl)] if guarded else [])
    infer = lambda t: lib.probav_forward_wc(h, P(t["params"]), P(t["x"]), P(t["y"]), P(t["ws"]), n0, 1, 0, P(t["wcache"]), nwc, S())
    plain = lambda nb: (lambda t: lib.probav_optimizer_step_fused(h, P(t["params"]), P(t["grads"]), P(t["m"]), P(t["v"]), *HYPER, P(t["wcache"]), nb, S())
                        or (infer(t) if nb == nwc else 0))
    bands.check(bufs(), plain(nwc), dev, fills=fills)
    bands.check_refusal(bufs(), plain(nwc - 1), dev, L.PROBAV_ENOSPACE)
    guarded = lambda nb: (lambda t: lib.probav_optimizer_step_fused_guarded(h, P(t["params"]), P(t["grads"]), P(t["m"]), P(t["v"]), *HYPER, P(t["wcache"]), nb, P(t["ema"]),
                                                                            ctypes.c_float(0.99), P(t["ctl"]), S()) or (infer(t) if nb == nwc else 0))
    bands.check(bufs(guarded=True, ctl=_ctl(0.5, 0)), guarded(nwc), dev, fills=fills)
    bands.check(bufs(keep=np.ones(flat.size, bool), guarded=True, ctl=_ctl(0.5, 1)), guarded(nwc), dev, fills=fills)      # a skipped step leaves params, m, v, ema as they were
    bands.check_refusal(bufs(guarded=True, ctl=_ctl(0.5, 0)), guarded(nwc - 1), dev, L.PROBAV_ENOSPACE)


@pytest.mark.parametrize("T,C,impl", [(T, C, impl) for T, C in ENGINE_CFGS for impl in ENGINE_IMPLS])
def test_engine_weight_norm(dev, T, C, impl):
    lib = _L().lib()
    h, flat, layers = _engine(dev, T, C, impl)
    nw, nc = lib.probav_weff_count(h), lib.probav_cout_total(h)
    bias = np.zeros(flat.size, bool)                     # probav_wn_backward writes d loss / d g and d loss / d v; the bias entries of grads are left as they were
    for Lh in layers:
        bias[Lh.b_off:Lh.b_off + Lh.cout] = True
    bufs = [bands.inp("params", flat), bands.inp("dweff", _f32(np.random.default_rng(23), nw)), bands.out("weff", F32, nw), bands.out("weffT", F32, nw),
            bands.out("inv_norm", F32, nc), bands.out("grads", F32, flat.size, keep=bias)]
    bands.check(bufs, lambda t: lib.probav_wn_forward(h, P(t["params"]), P(t["weff"]), P(t["weffT"]), P(t["inv_norm"]), S())
                or lib.probav_wn_backward(h, P(t["params"]), P(t["dweff"]), P(t["inv_norm"]), P(t["grads"]), S()), dev)


@pytest.mark.parametrize("T,C,B,impl", [p for p in ENGINE_PARAMS if p[3] in (3, 4)])
def test_engine_debug_hidden(dev, T, C, B, impl):
    L, lib = _L(), _L().lib()
    h, flat, _ = _engine(dev, T, C, impl)
    _, _, saved, _, _ = _sizes(h, B)
    x, _ = _batch(T, C, B)
    vox = B * 22 * 22 * T
    ins, y = _io(flat, x, None, B)
    bufs = ins + [y, bands.scratch("ws", saved), bands.out("hidden", F32, vox * 256, lead_count=22 * 22 * T * 256), bands.out("dec", F32, vox * 25, lead_count=22 * 22 * T * 25)]
    hidden = lambda t, nb, block: lib.probav_debug_hidden(h, P(t["params"]), P(t["ws"]), nb, B, block, P(t["hidden"]), P(t["dec"]), None, S())
    block = 11 if B == 1 else 0
    bands.check(bufs, lambda t: lib.probav_forward(h, P(t["params"]), P(t["x"]), P(t["y"]), P(t["ws"]), saved, B, 1, S()) or hidden(t, saved, block), dev,
                fills=_fills(dev, T, C, impl, B, {"ws": (0, saved)}))
    bands.check_refusal(bufs, lambda t: hidden(t, saved - 1, block), dev, L.PROBAV_ENOSPACE)


# ---- losses, optimizer, epilogue ---------------------------------------------------------------------------------------------------------
def _cf(v):
    return ctypes.c_float(v)


@pytest.mark.parametrize("B,size,border", [(1, 48, 3), (5, 48, 3), (3, 30, 2)])
def test_losses(dev, B, size, border):
    from tests import loss_cases
    L, lib = _L(), _L().lib()
    hr, mask, pred = loss_cases.inputs(loss_cases._case("shift", size, border, B, seed=100 + B))
    ins = [bands.inp("hr", hr), bands.inp("mask", mask.astype(np.uint8)), bands.inp("pred", pred), bands.inp("upstream", np.float32([0.75]))]
    dpred = lambda n: bands.out(n, F32, B * size * size, lead_count=size * size)
    # L1 / L2 / cPSNR and both gradients, each from the arg-min the forward wrote
    bufs = ins + [bands.out(n, F32, B) for n in ("l1", "l2", "cpsnr")] + [bands.out(n, I32, B) for n in ("arg_l1", "arg_l2")] + \
        [bands.out("mean_l1", F32, 1), bands.out("mean_l2", F32, 1), dpred("dpred_l1"), dpred("dpred_l2")]

    def shift(t):
        rc = lib.probav_shift_loss_forward(P(t["hr"]), P(t["mask"]), P(t["pred"]), B, size, border, 16, P(t["l1"]), P(t["l2"]), P(t["cpsnr"]), P(t["arg_l1"]), P(t["arg_l2"]),
                                           P(t["mean_l1"]), P(t["mean_l2"]), S())
        for which in (1, 2):
            rc = rc or lib.probav_shift_loss_backward(P(t["hr"]), P(t["mask"]), P(t["pred"]), P(t["arg_l%d" % which]), B, size, border, which, P(t["upstream"]),
                                                      P(t["dpred_l%d" % which]), S())
        return rc
    bands.check(bufs, shift, dev)
    # sobel_l1_mix: mean is TWO floats (the loss and a scratch word -- the second is the library's own: scratch)
    bufs = ins + [bands.out("loss", F32, B), bands.out("arg", I32, B), bands.out("mean", F32, 2), dpred("dpred")]
    bands.check(bufs, lambda t: lib.probav_shift_l1edge_forward(P(t["hr"]), P(t["mask"]), P(t["pred"]), B, size, border, _cf(0.7), P(t["loss"]), P(t["arg"]), P(t["mean"]), S())
                or lib.probav_shift_l1edge_backward(P(t["hr"]), P(t["mask"]), P(t["pred"]), P(t["arg"]), B, size, border, _cf(0.7), P(t["upstream"]), P(t["dpred"]), S()), dev)
    # l1msssim with its scratch
    nbytes = lib.probav_revssim_scratch_bytes(B, border)
    bufs = ins + [bands.out("loss", F32, 1), bands.out("arg", I32, 1), dpred("dpred"), bands.scratch("scratch", nbytes)]
    fwd = lambda t, nb: lib.probav_revssim_forward(P(t["hr"]), P(t["mask"]), P(t["pred"]), B, size, border, 16, _cf(0.25), P(t["scratch"]), nb, P(t["loss"]), P(t["arg"]), S())
    bands.check(bufs, lambda t: fwd(t, nbytes) or lib.probav_revssim_backward(P(t["hr"]), P(t["mask"]), P(t["pred"]), P(t["arg"]), P(t["scratch"]), B, size, border, 16, _cf(0.25),
                                                                               P(t["upstream"]), P(t["dpred"]), S()), dev)
    bands.check_refusal(bufs, lambda t: fwd(t, nbytes - 1), dev, L.PROBAV_ENOSPACE)


@pytest.mark.parametrize("n", [1, 255, 257, 535267])
def test_optimizer(dev, n):
    L, lib = _L(), _L().lib()
    rng = np.random.default_rng(n)
    p, g, m, v = _f32(rng, n), _f32(rng, n, scale=1e-2), _f32(rng, n, scale=1e-2), np.abs(_f32(rng, n, scale=1e-4))
    io = lambda name, a, keep=None: bands.Buf(name, F32, "inout", init=a, keep=keep)
    bands.check([io("params", p), bands.inp("grads", g), io("m", m), io("v", v)],
                lambda t: lib.probav_nadam_step(P(t["params"]), P(t["grads"]), P(t["m"]), P(t["v"]), n, *HYPER, S()), dev)
    # the guard: scratch exactly its query; ctl is read (skipped_total) and written
    nbytes = lib.probav_grad_guard_scratch_bytes(n)
    for grads, skip in ((g, 0), (np.where(np.arange(n) == n // 2, np.float32("inf"), g), 1)):
        keep = np.ones(n, bool) if skip else None
        bufs = [io("params", p, keep), bands.inp("grads", grads), io("m", m, keep), io("v", v, keep), io("ema", p * np.float32(0.5), keep),
                bands.Buf("ctl", U8, "inout", init=_ctl(0.0, 0)), bands.scratch("scratch", nbytes)]
        guard = lambda t, nb: lib.probav_grad_guard(P(t["grads"]), n, _cf(0.01), 1, P(t["scratch"]), nb, P(t["ctl"]), S())
        rep = bands.check(bufs, lambda t: guard(t, nbytes) or lib.probav_nadam_step_guarded(P(t["params"]), P(t["grads"]), P(t["m"]), P(t["v"]), P(t["ema"]), n, *HYPER, _cf(0.99),
                                                                                             P(t["ctl"]), S()), dev)
        assert int(rep.outputs["ctl"].view(torch.int32)[1]) == skip and int(rep.outputs["ctl"].view(torch.int32)[2]) == 7 + skip
        bands.check_refusal(bufs, lambda t: guard(t, nbytes - 1), dev, L.PROBAV_ENOSPACE)


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_clip_round(dev, n):
    x = _f32(np.random.default_rng(n), n, scale=300.0)
    bands.check([bands.inp("in", x), bands.out("out", F32, n)], lambda t: _L().lib().probav_clip_round(P(t["in"]), P(t["out"]), n, _cf(0.0), _cf(65535.0), S()), dev)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("T", [7, 9])
def test_input_grad(dev, T, C):
    B, H = 2, 22
    rng = np.random.default_rng(T * 10 + C)
    g, act0 = _f32(rng, B, H, H, T, 32), _f32(rng, B, H, H, T, 32)
    d1, gate1 = _f32(rng, B, H - 2, H - 2, 9), _f32(rng, B, H - 2, H - 2, 9)
    wmain, w1 = _f32(rng, 3, 3, 3, C, 32, scale=0.1), _f32(rng, 3, 3, 1, C, 9, scale=0.1)
    for gated in (True, False):
        bufs = [bands.inp("g", g), bands.inp("act0", act0), bands.inp("wmain", wmain), bands.inp("d1", d1), bands.inp("w1", w1)] + (_opt("gate1", gate1) if gated else []) + \
            [bands.out("dx", F32, B * H * H * T * C, lead_count=H * H * T * C)]
        bands.check(bufs, lambda t: _L().lib().probav_input_grad(B, H, T, C, P(t["g"]), P(t["act0"]), P(t["wmain"]), P(t["d1"]), P(t.get("gate1")), P(t["w1"]),
                                                                 _cf(synth.NIR_STD), P(t["dx"]), S()), dev)


# ---- scoring ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [0, 3])
@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("size", [17, 48])
def test_scoring(dev, size, n_images, b):
    from probav_amd.scoring import gauss11
    from tests.ssim_helpers import noise_case
    L, lib = _L(), _L().lib()
    sr, hr, mask = noise_case(n_images, size, 14, seed=size + n_images + b)
    mask = mask.astype(np.uint8)
    if n_images == 3:
        mask[1] = 0                                      # an image with no clear pixel: NaN / (-1, -1) rows, still written
    ns = (2 * b + 1) ** 2
    nbytes = lib.probav_ssim_scratch_bytes(n_images, size, b)
    assert nbytes > 0
    bufs = [bands.inp("sr", sr), bands.inp("hr", hr), bands.inp("mask", mask), bands.inp("gauss11", np.asarray(gauss11(), np.float64)),
            bands.out("moments", I64, n_images * ns * 3, lead_count=ns * 3), bands.out("cpsnr", F64, n_images), bands.out("shift", I32, n_images * 2),
            bands.out("bias", F64, n_images), bands.out("n_clear", I64, n_images), bands.out("table", F64, n_images * ns, lead_count=ns),
            bands.out("cssim", F64, n_images), bands.out("sshift", I32, n_images * 2), bands.scratch("scratch", nbytes)]
    table = lambda t, nb: lib.probav_ssim_table(P(t["sr"]), P(t["hr"]), P(t["mask"]), P(t["moments"]), P(t["gauss11"]), n_images, size, b, P(t["scratch"]), nb, P(t["table"]), S())

    def score(t):
        return (lib.probav_score_moments(P(t["sr"]), P(t["hr"]), P(t["mask"]), n_images, size, b, P(t["moments"]), S())
                or lib.probav_score_select(P(t["moments"]), n_images, b, P(t["cpsnr"]), P(t["shift"]), P(t["bias"]), P(t["n_clear"]), S())
                or table(t, nbytes) or lib.probav_ssim_select(P(t["table"]), n_images, b, P(t["cssim"]), P(t["sshift"]), S()))
    bands.check(bufs, score, dev)
    bands.check_refusal(bufs, lambda t: table(t, nbytes - 1), dev, L.PROBAV_ENOSPACE)


# ---- data path ---------------------------------------------------------------------------------------------------------------------------------
def _frames16(rng, n, H, W):
    base = rng.integers(2000, 12000, (H, W))
    return np.stack([np.roll(base, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(0, 1)) + rng.integers(0, 200, (H, W)) for _ in range(n)]).astype(np.uint16)


def _rows(a, rows):
    """A keep mask over an array shaped like `a`: its leading-index slices `rows`."""
    k = np.zeros(a, bool) if isinstance(a, tuple) else np.zeros(a.shape, bool)
    k[list(rows)] = True
    return k


def test_prep_count_nonzero(dev):
    n, chunk = 5, 1001
    data = (np.random.default_rng(1).random(n * chunk) < 0.3).astype(np.uint8)
    bands.check([bands.inp("data", data), bands.out("counts", I32, n)],
                lambda t: _L().lib().probav_prep_count_nonzero(P(t["data"]), n, chunk, P(t["counts"]), S()), dev)


# three sets of 2, 1 and 2 frames; the reference of set 1 lies outside it: the header says its frame is neither read nor written and its shift is the BAD marker
_OFFSETS, _REFS, _BAD_FRAMES = np.int64([0, 2, 3, 5]), np.int32([0, 0, 4]), [2]


def test_prep_register(dev):
    rng = np.random.default_rng(2)
    F, n = 5, 128 * 128
    frames = _frames16(rng, F, 128, 128)
    masks = (rng.random((F, 128, 128)) < 0.9).astype(np.uint8)
    bufs = [bands.inp("frames", frames), bands.inp("masks", masks), bands.inp("set_offsets", _OFFSETS), bands.inp("ref_frame", _REFS),
            bands.scratch("spec_scratch", 3 * n * 2 * 4), bands.out("shifts", I32, F * 2),
            bands.out("reg_frames", U16, F * n, lead_count=n, keep=_rows((F, n), _BAD_FRAMES)), bands.out("reg_masks", U8, F * n, lead_count=n, keep=_rows((F, n), _BAD_FRAMES)),
            bands.out("reg_counts", I32, F, keep=_rows((F,), _BAD_FRAMES))]
    rep = bands.check(bufs, lambda t: _L().lib().probav_prep_register(P(t["frames"]), P(t["masks"]), P(t["set_offsets"]), 3, F, P(t["ref_frame"]), P(t["spec_scratch"]),
                                                                       P(t["shifts"]), P(t["reg_frames"]), P(t["reg_masks"]), P(t["reg_counts"]), S()), dev)
    assert rep.outputs["shifts"].view(torch.int32).view(F, 2)[2].tolist() == [-2 ** 31, -2 ** 31]


def test_prep_xcorr_surface(dev):
    pair = _frames16(np.random.default_rng(3), 2, 128, 128)
    bufs = [bands.inp("pair", pair), bands.scratch("spec_scratch", 128 * 128 * 2 * 4), bands.out("surface", F32, 128 * 128), bands.out("info", F64, 4)]
    bands.check(bufs, lambda t: _L().lib().probav_prep_xcorr_surface(P(t["pair"]), P(t["spec_scratch"]), P(t["surface"]), P(t["info"]), S()), dev)


@pytest.mark.parametrize("pad,win,stride", [(3, 22, 16), (0, 48, 48)])
def test_prep_patches(dev, pad, win, stride):
    rng = np.random.default_rng(4)
    Sn, T, H, W = 2, 3, (38, 50) if pad else (96, 144), None
    H, W = H
    nh, nw = (H + 2 * pad - win) // stride + 1, (W + 2 * pad - win) // stride + 1
    n = Sn * nh * nw * T
    frames, masks = _f32(rng, Sn, T, H, W), (rng.random((Sn, T, H, W)) < 0.2).astype(np.uint8) * 255
    bufs = [bands.inp("frames", frames), bands.inp("masks", masks), bands.out("patches", F32, n * win * win, lead_count=nh * nw * T * win * win),
            bands.out("patch_masks", U8, n * win * win, lead_count=nh * nw * T * win * win), bands.out("counts", I32, n)]
    bands.check(bufs, lambda t: _L().lib().probav_prep_patches(P(t["frames"]), P(t["masks"]), Sn, T, H, W, pad, win, stride, P(t["patches"]), P(t["patch_masks"]),
                                                               P(t["counts"]), S()), dev)


def test_prep_register_masked(dev):
    rng = np.random.default_rng(5)
    F, n = 5, 128 * 128
    frames = _frames16(rng, F, 128, 128)
    masks = (rng.random((F, 128, 128)) < 0.9).astype(np.uint8)
    bufs = [bands.inp("frames", frames), bands.inp("masks", masks), bands.inp("set_offsets", _OFFSETS), bands.inp("ref_frame", _REFS), bands.out("shifts", I32, F * 2),
            bands.out("registered", U8, F, keep=_rows((F,), _BAD_FRAMES)),
            bands.out("out_frames", U16, F * n, lead_count=n, keep=_rows((F, n), _BAD_FRAMES)), bands.out("out_masks", U8, F * n, lead_count=n, keep=_rows((F, n), _BAD_FRAMES)),
            bands.out("out_counts", I32, F, keep=_rows((F,), _BAD_FRAMES))]
    rep = bands.check(bufs, lambda t: _L().lib().probav_prep_register_masked(P(t["frames"]), P(t["masks"]), P(t["set_offsets"]), 3, F, P(t["ref_frame"]), 3, P(t["shifts"]),
                                                                              P(t["registered"]), P(t["out_frames"]), P(t["out_masks"]), P(t["out_counts"]), S()), dev)
    assert rep.outputs["shifts"].view(torch.int32).view(F, 2)[2].tolist() == [-2 ** 31, -2 ** 31]


@pytest.mark.parametrize("H,W", [(13, 9), (1, 70)])
def test_prep_refine_masks(dev, H, W):
    """Sets of 3, 4 and 3 frames with max_set_len = 3: the middle set breaks the precondition and is neither read nor written (its counts are the BAD marker)."""
    rng = np.random.default_rng(6)
    F, offs, bad = 10, np.int64([0, 3, 7, 10]), [3, 4, 5, 6]
    frames = rng.integers(3000, 3400, (F, H, W)).astype(np.uint16)
    frames[1, H // 2, W // 2] = 15000                      # an outlier, and a saturated pixel
    frames[8, 0, 0] = 16383
    masks = (rng.random((F, H, W)) < 0.9).astype(np.uint8)
    bufs = [bands.inp("frames", frames), bands.inp("masks", masks), bands.inp("set_offsets", offs),
            bands.out("pixel_masks", I64, 3 * 3 * H * W, lead_count=3 * H * W, keep=_rows((3, 3 * H * W), [1])),
            bands.out("out_masks", U8, F * H * W, lead_count=H * W, keep=_rows((F, H * W), bad)), bands.out("out_counts", I32, F), bands.out("flagged", I32, F * 2)]
    rep = bands.check(bufs, lambda t: _L().lib().probav_prep_refine_masks(P(t["frames"]), P(t["masks"]), P(t["set_offsets"]), 3, F, H, W, 3, 48, 16, 3, 1, 16000,
                                                                           P(t["pixel_masks"]), P(t["out_masks"]), P(t["out_counts"]), P(t["flagged"]), S()), dev)
    assert rep.outputs["out_counts"].view(torch.int32)[3:7].tolist() == [-1] * 4


def _recipe(rng, rows, T, n_src, bad_row=None):
    r = np.zeros((rows, 3 + T), np.int32)
    for b in range(rows):
        r[b, 0], r[b, 1], r[b, 2] = rng.integers(0, n_src), b % 4, (b // 2) % 4
        r[b, 3:] = rng.permutation(T)
    if bad_row is not None:
        r[bad_row, 0] = n_src + 3                           # points outside the base array: the row is skipped
    return r


def test_augment_and_ensemble(dev):
    lib = _L().lib()
    rng = np.random.default_rng(7)
    n_base, H, T, C, Sz, batch = 2, 7, 3, 1, 21, 5
    lr, hr, mask = _f32(rng, n_base, H, H, T, C), _f32(rng, n_base, Sz, Sz), (rng.random((n_base, Sz, Sz)) < 0.5).astype(np.uint8)
    recipe = _recipe(rng, batch, T, n_base, bad_row=2)
    nl, nh = H * H * T * C, Sz * Sz
    bufs = [bands.inp("lr", lr), bands.inp("hr", hr), bands.inp("mask", mask), bands.inp("recipe", recipe),
            bands.out("lr_b", F32, batch * nl, lead_count=nl, keep=_rows((batch, nl), [2])), bands.out("hr_b", F32, batch * nh, lead_count=nh, keep=_rows((batch, nh), [2])),
            bands.out("mask_b", U8, batch * nh, lead_count=nh, keep=_rows((batch, nh), [2]))]
    bands.check(bufs, lambda t: lib.probav_augment_batch(P(t["lr"]), P(t["hr"]), P(t["mask"]), n_base, H, T, C, Sz, P(t["recipe"]), batch, P(t["lr_b"]), P(t["hr_b"]),
                                                         P(t["mask_b"]), S()), dev)
    bufs = [bands.inp("lr", lr), bands.inp("recipe", recipe), bands.out("out", F32, batch * nl, lead_count=nl, keep=_rows((batch, nl), [2]))]
    bands.check(bufs, lambda t: lib.probav_ensemble_expand(P(t["lr"]), n_base, H, T, C, P(t["recipe"]), batch, P(t["out"]), S()), dev)
    # reduce: three base patches of V = 2 members; one member of patch 1 carries k = 7: that patch is skipped
    V, nb = 2, 3
    sr = _f32(rng, nb * V, Sz, Sz, scale=3000.0)
    rec = _recipe(rng, nb * V, T, nb)
    rec[3, 2] = 7
    for final_round, grid in ((1, 0), (0, 0)):
        bufs = [bands.inp("sr", sr), bands.inp("recipe", rec), bands.out("out", F32, nb * nh, lead_count=nh, keep=_rows((nb, nh), [1]))]
        bands.check(bufs, lambda t: lib.probav_ensemble_reduce(P(t["sr"]), P(t["recipe"]), nb, V, T, Sz, _cf(0.0), _cf(65535.0), final_round, grid, P(t["out"]), S()), dev)
    # the stitched form: four patches of one image, none skipped
    sr4, rec4 = _f32(rng, 4 * V, Sz, Sz, scale=3000.0), _recipe(rng, 4 * V, T, 4)
    bufs = [bands.inp("sr", sr4), bands.inp("recipe", rec4), bands.out("out", F32, 4 * nh)]
    bands.check(bufs, lambda t: lib.probav_ensemble_reduce(P(t["sr"]), P(t["recipe"]), 4, V, T, Sz, _cf(0.0), _cf(65535.0), 1, 2, P(t["out"]), S()), dev)


@pytest.mark.parametrize("n,Sz,stride", [(2, 12, 8), (3, 15, 15), (1, 48, 48)])
def test_tile_blend(dev, n, Sz, stride):
    rng = np.random.default_rng(8)
    n_images, G = 2, (n - 1) * stride + Sz
    sr, w = _f32(rng, n_images * n * n, Sz, Sz, scale=3000.0), rng.integers(1, 1025, Sz).astype(np.int32)
    bufs = [bands.inp("sr", sr), bands.inp("w", w), bands.out("out", F32, n_images * G * G, lead_count=G * G)]
    bands.check(bufs, lambda t: _L().lib().probav_tile_blend(P(t["sr"]), P(t["w"]), n_images, n, Sz, stride, _cf(0.0), _cf(65535.0), P(t["out"]), S()), dev)


@pytest.mark.parametrize("mode", [0, 1], ids=["esa", "clear"])
def test_baseline(dev, mode):
    """Sets of 2, 0 and 3 frames: the empty one breaks the precondition, is neither read nor written and gets k_used = -1.  counts_scratch is the caller's: it receives
    every frame's clear count in esa mode and is not touched in clear mode."""
    rng = np.random.default_rng(9)
    H, W, F = 5, 7, 5
    frames, clear = rng.integers(0, 16384, (F, H, W)).astype(np.uint16), (rng.random((F, H, W)) < 0.7).astype(np.uint8)
    n = 9 * H * W
    bufs = [bands.inp("frames", frames), bands.inp("clear", clear), bands.inp("set_offsets", np.int64([0, 2, 2, 5])),
            bands.out("counts_scratch", I32, F, keep=np.ones(F, bool) if mode == 1 else None), bands.out("out", F32, 3 * n, lead_count=n, keep=_rows((3, n), [1])),
            bands.out("k_used", I32, 3)]
    rep = bands.check(bufs, lambda t: _L().lib().probav_baseline_upscale_mean(P(t["frames"]), P(t["clear"]), P(t["set_offsets"]), 3, F, H, W, 3, mode, P(t["counts_scratch"]),
                                                                               P(t["out"]), P(t["k_used"]), S()), dev)
    assert int(rep.outputs["k_used"].view(torch.int32)[1]) == -1


@pytest.mark.parametrize("mode", [0, 1], ids=["clear", "uniform"])
def test_frame_windows(dev, mode):
    lib = _L().lib()
    rng = np.random.default_rng(10)
    N, T_pre, win, k, Wn, step, Sz = 3, 5, 6, 3, 2, 1, 18
    patches, counts = _f32(rng, N, T_pre, win, win), rng.integers(0, 30, (N, T_pre)).astype(np.int32)
    counts[1] = 36                                         # a tile without an eligible frame: all of them are
    bufs = [bands.inp("patches", patches), bands.inp("counts", counts), bands.out("x", F32, N * Wn * win * win * k, lead_count=Wn * win * win * k),
            bands.out("weight", I32, N * Wn, lead_count=Wn), bands.out("sel", I32, N * Wn * k, lead_count=Wn * k)]
    rep = bands.check(bufs, lambda t: lib.probav_frame_windows_gather(P(t["patches"]), P(t["counts"]), N, T_pre, win, k, 20, Wn, step, mode, P(t["x"]), P(t["weight"]),
                                                                       P(t["sel"]), S()), dev)
    weight = rep.outputs["weight"].view(torch.int32).cpu().numpy().reshape(N, Wn)
    sr = _f32(rng, N * Wn, Sz, Sz, scale=3000.0)
    bufs = [bands.inp("sr", sr), bands.inp("weight", weight), bands.out("out", F32, N * Sz * Sz, lead_count=Sz * Sz)]
    bands.check(bufs, lambda t: lib.probav_frame_windows_reduce(P(t["sr"]), P(t["weight"]), N, Wn, Sz, _cf(0.0), _cf(65535.0), P(t["out"]), S()), dev)


def test_crops(dev):
    lib = _L().lib()
    rng = np.random.default_rng(11)
    M, H, W, pad, win, stride = 2, 9, 11, 2, 4, 3
    ny, nx = (H + 2 * pad - win) // stride + 1, (W + 2 * pad - win) // stride + 1
    masks = (rng.random((M, H, W)) < 0.3).astype(np.uint8)
    bands.check([bands.inp("masks", masks), bands.out("counts", I32, M * ny * nx, lead_count=ny * nx)],
                lambda t: lib.probav_window_counts(P(t["masks"]), M, H, W, pad, win, stride, P(t["counts"]), S()), dev)
    n_scenes, T_pre, Hs, Pp, pad, win, scale, k, batch = 2, 4, 12, 5, 1, 7, 3, 3, 4
    Sz = scale * Pp
    lr, lr_mask = _f32(rng, n_scenes, T_pre, Hs, Hs), (rng.random((n_scenes, T_pre, Hs, Hs)) < 0.2).astype(np.uint8)
    hr, hr_clear = _f32(rng, n_scenes, scale * Hs, scale * Hs), (rng.random((n_scenes, scale * Hs, scale * Hs)) < 0.8).astype(np.uint8)
    positions = np.int32([[0, 0, 0], [1, 7, 7], [0, 3, 5]])
    recipe = _recipe(rng, batch, k, len(positions), bad_row=1)
    nl, nh = win * win * k, Sz * Sz
    bufs = [bands.inp("lr", lr), bands.inp("lr_mask", lr_mask), bands.inp("hr", hr), bands.inp("hr_clear", hr_clear), bands.inp("positions", positions),
            bands.inp("recipe", recipe), bands.out("lr_b", F32, batch * nl, lead_count=nl, keep=_rows((batch, nl), [1])),
            bands.out("hr_b", F32, batch * nh, lead_count=nh, keep=_rows((batch, nh), [1])), bands.out("mask_b", U8, batch * nh, lead_count=nh, keep=_rows((batch, nh), [1])),
            bands.out("sel", I32, batch * k, lead_count=k, keep=_rows((batch, k), [1]))]
    bands.check(bufs, lambda t: lib.probav_crop_batch(P(t["lr"]), P(t["lr_mask"]), P(t["hr"]), P(t["hr_clear"]), n_scenes, T_pre, Hs, Pp, pad, win, scale, k, win * win + 1,
                                                      P(t["positions"]), len(positions), P(t["recipe"]), batch, P(t["lr_b"]), P(t["hr_b"]), P(t["mask_b"]), P(t["sel"]), S()), dev)


@pytest.mark.parametrize("shape", [(1, 17, 17), (2, 48, 48), (1, 49, 83)], ids=str)
def test_fusenet(dev, shape):
    from tests import fusenet_helpers as fh
    L, lib = _L(), _L().lib()
    B, H, W = shape
    x, g, flat = fh.image(shape), fh.upstream(shape), fh.flat_of(*fh.params())
    nf, nb = lib.probav_fusenet_workspace_bytes(B, H, W, 0), lib.probav_fusenet_workspace_bytes(B, H, W, 1)
    assert nf > 0 and nb > 0 and flat.size == 147648
    bufs = [bands.inp("x", x), bands.inp("g", g), bands.inp("flat", flat), bands.out("out", F32, B * H * W, lead_count=H * W),
            bands.out("y", F32, B * H * W * 64, lead_count=H * W * 64), bands.out("stats", F32, B * 64 * 2, lead_count=128), bands.out("dflat", F32, flat.size),
            bands.scratch("ws_fwd", nf), bands.scratch("ws_bwd", nb)]
    fwd = lambda t, n: lib.probav_fusenet_forward(P(t["x"]), P(t["flat"]), flat.size, B, H, W, 1, P(t["out"]), P(t["y"]), P(t["stats"]), P(t["ws_fwd"]), n, S())
    bwd = lambda t, n: lib.probav_fusenet_backward(P(t["g"]), P(t["x"]), P(t["y"]), P(t["stats"]), P(t["flat"]), flat.size, B, H, W, P(t["dflat"]), P(t["ws_bwd"]), n, S())
    bands.check(bufs, lambda t: fwd(t, nf) or bwd(t, nb), dev)
    bands.check_refusal(bufs, lambda t: fwd(t, nf - 1), dev, L.PROBAV_EINVAL)
    bands.check_refusal(bufs, lambda t: bwd(t, nb - 1), dev, L.PROBAV_EINVAL)


# ---- measurement aid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [None, 0, 1], ids=["probe", "shape0", "shape1"])
def test_mfma_probe(dev, shape):
    lib = _L().lib()
    seed = (np.random.default_rng(12).standard_normal(128 * 8) * 0.25).astype(np.float16)            # 128 x 16 bytes
    bufs = [bands.inp("seed", seed), bands.out("sink", F32, 256 * 256)]
    if shape is None:
        bands.check(bufs, lambda t: lib.probav_mfma_probe(P(t["seed"]), P(t["sink"]), 2, 2, S()), dev)
    else:
        bands.check(bufs, lambda t: lib.probav_mfma_probe_shape(P(t["seed"]), P(t["sink"]), 2, 2, shape, S()), dev)
