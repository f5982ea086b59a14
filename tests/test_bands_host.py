"""tests/bands.py on CPU tensors: the carving arithmetic, and that the harness reports what it is there to report -- a write one byte
before or after a buffer at the right offset, an input that changed, an output that depends on the fill, a kept element that was written,
a refusal that touched something."""
import numpy as np
import pytest
import torch

from tests import bands

CPU = torch.device("cpu")


def _bufs():
    x = np.arange(3 * 7 * 5, dtype=np.float32).reshape(3, 7, 5)
    return [bands.inp("x", x),
            bands.out("y", torch.float32, 3 * 35 + 1, lead_count=35),            # 424 bytes: no multiple of 16
            bands.scratch("s", 13),
            bands.out("big", torch.uint16, 2 * 40000, lead_count=40000),         # one slice (80 000 bytes) is larger than BAND_MIN
            bands.out("d", torch.float64, 3)]


def test_carving_alignment_lengths_and_bands():
    bufs = _bufs()
    plan, total = bands.carve(bufs)
    assert total % bands.ALIGN == 0
    prev_end = 0
    for b, (before, start, after, end) in zip(bufs, plan):
        assert before == prev_end                                   # nothing between one buffer's bands and the next's
        assert start % bands.ALIGN == 0
        assert after == start + b.nbytes                            # the band after begins at the buffer's last byte + 1: no rounding up
        assert start - before >= max(bands.BAND_MIN, b.lead)
        assert end - after >= max(bands.BAND_MIN, b.lead)
        assert end % bands.ALIGN == 0 and end - after < max(bands.BAND_MIN, b.lead) + 2 * bands.ALIGN
        prev_end = end
    assert prev_end == total
    assert [b.nbytes for b in bufs] == [420, 424, 13, 160000, 24]
    assert bands.band_bytes(bufs[3]) == 80000 and bands.band_bytes(bufs[0]) == bands.BAND_MIN
    a = bands.Arena(bufs, CPU, bands.Fill(0xFF))
    for b in bufs:
        t = a.tensors[b.name]
        assert t.dtype == b.dtype and t.numel() * t.element_size() == b.nbytes and t.data_ptr() % 16 == 0
    # consecutive buffers are separated by both their bands
    assert a.tensors["y"].data_ptr() - (a.tensors["x"].data_ptr() + 420) >= 2 * bands.BAND_MIN
    assert torch.equal(a.tensors["x"].reshape(3, 7, 5), torch.arange(105, dtype=torch.float32).reshape(3, 7, 5))
    assert bool(torch.isnan(a.tensors["y"]).all()) and bool(torch.isnan(a.tensors["d"]).all()) and int(a.tensors["big"][0]) == 65535
    assert not a.violations()
    b0 = bands.Arena(bufs, CPU, bands.Fill(0x00))
    assert float(b0.tensors["y"].abs().sum()) == 0.0 and not b0.violations()


def _good(t):
    t["y"][:] = torch.arange(t["y"].numel(), dtype=torch.float32)
    t["big"][:] = 7
    t["d"][:] = t["x"].double().sum()
    t["s"][:] = 3
    return 0


def test_clean_launch_passes():
    rep = bands.check(_bufs(), _good, CPU)
    assert rep.ok() and rep.rcs == {"0xFF": 0, "0x00": 0, "plain": 0}


def _raw(t, name, off):
    """A one-byte view `off` bytes from the start of a carved tensor: the overrun of a kernel, staged by hand (inside the arena)."""
    base = t[name]
    return torch.as_strided(base.reshape(-1).view(torch.uint8), (1,), (1,), storage_offset=base.storage_offset() * base.element_size() + off)


@pytest.mark.parametrize("name,off,side,where", [("y", -1, "before", None), ("y", 424, "after", 0), ("s", 13, "after", 0), ("s", -1, "before", None),
                                                   ("big", 160000 + 79999, "after", 79999), ("x", -70, "before", None)])
def test_write_outside_a_buffer_is_reported_with_its_offset(name, off, side, where):
    bufs = _bufs()

    def call(t):
        _good(t)
        _raw(t, name, off)[0] = 0x5A
        return 0
    rep = bands.run(bufs, call, CPU, plain=False)
    band = bands.band_bytes([b for b in bufs if b.name == name][0])
    want = where if side == "after" else band + off              # offsets count from the band's first byte
    assert sorted(v.key() for v in rep.violations) == [(name, side, want, want)] * 2, str(rep)      # once per fill, nothing else
    with pytest.raises(AssertionError, match="%s: %s" % (name, side)):
        bands.check(bufs, call, CPU, plain=False)


def test_input_change_is_reported():
    def call(t):
        _good(t)
        t["x"].view(3, 7, 5)[1, 2, 3] = -1.0
        return 0
    rep = bands.run(_bufs(), call, CPU)
    first = (1 * 35 + 2 * 5 + 3) * 4
    assert {v.key()[:2] for v in rep.violations} == {("x", "in")}
    assert all(v.first >= first and v.last <= first + 3 for v in rep.violations)


def test_output_that_depends_on_the_fill_is_reported():
    def unwritten_plain(t):
        t["y"][:] = torch.arange(t["y"].numel(), dtype=torch.float32)
        t["big"][:] = 7
        t["d"][:2] = 1.5
        t["s"][:] = 3
        return 0
    rep = bands.run(_bufs(), unwritten_plain, CPU, plain=False)
    assert [(v.buffer, v.side, v.first, v.last) for v in rep.violations] == [("d", "differs", 16, 23)], str(rep)

    def stale(t):                                         # a result computed from what scratch held before the call
        _good(t)
        t["y"][3] = t["y"][3] + float(int(t["s"][0]) & 1)
        t["s"][0] = 1
        return 0

    def stale_read_first(t):
        s0 = float(int(t["s"][0]) & 1)
        _good(t)
        t["y"][3] = 100.0 + s0
        return 0
    assert bands.run(_bufs(), stale, CPU).ok()              # scratch written before it is read: independent of the fill
    rep = bands.run(_bufs(), stale_read_first, CPU, plain=False)
    assert [(v.buffer, v.side, v.first, v.last) for v in rep.violations] == [("y", "differs", 14, 14)], str(rep)      # fp32 100.0 against 101.0: one byte of element 3
    with pytest.raises(AssertionError, match="y: differs"):
        bands.check(_bufs(), stale_read_first, CPU, plain=False)


def test_kept_elements_must_hold_the_fill_and_are_not_compared():
    keep = np.zeros((4, 6), bool)
    keep[2] = True
    bufs = [bands.inp("x", np.ones(4, np.float32)), bands.out("rows", torch.int32, 24, lead_count=6, keep=keep)]

    def call(t, also=None):
        r = t["rows"].view(4, 6)
        for i in (0, 1, 3):
            r[i] = i
        if also is not None:
            r[2, also] = 9
        return 0
    assert bands.check(bufs, call, CPU).ok()
    rep = bands.run(bufs, lambda t: call(t, 5), CPU)
    assert sorted(v.key() for v in rep.violations) == [("rows", "kept", 68, 68), ("rows", "kept", 68, 71)], str(rep)   # int32 9 over 0x00: one byte, over 0xFF: four
    # an inout buffer's kept elements must hold their initial data
    p = np.arange(8, dtype=np.float32)
    bufs = [bands.inp("p", p, role="inout"), ]
    bufs[0].keep = torch.from_numpy(np.repeat(np.arange(8) >= 4, 4))

    def step(t, n=4):
        t["p"][:n] += 1
        return 0
    assert bands.check(bufs, step, CPU).ok()
    rep = bands.run(bufs, lambda t: step(t, 5), CPU)
    assert {v.key() for v in rep.violations} == {("p", "kept", 18, 18)}, str(rep)      # 4.0 -> 5.0: one byte of the fp32 pattern


def test_preset_fill_joins_the_comparison():
    bufs = [bands.inp("x", np.ones(4, np.float32)), bands.out("y", torch.float32, 4), bands.scratch("s", 8)]
    stale = bands.Fill(0xFF, preset={"s": torch.full((8,), 3, dtype=torch.uint8)}, label="stale")

    def call(t):
        t["y"][:] = t["x"] + float(t["s"][0] == 3)
        t["s"][:] = 1
        return 0
    rep = bands.run(bufs, call, CPU, fills=bands.FILLS + (stale,))
    assert [(v.buffer, v.side, v.fill) for v in rep.violations] == [("y", "differs", "0xFF vs stale")], str(rep)


def test_return_code_and_refusal():
    bufs = _bufs()
    rep = bands.run(bufs, lambda t: -2, CPU, expect_rc=0)
    assert [v.side for v in rep.violations] == ["rc"] * 3
    bands.check_refusal(bufs, lambda t: -2, CPU, -2)
    with pytest.raises(AssertionError, match="expected the refusal -2"):
        bands.check_refusal(bufs, lambda t: 0, CPU, -2)

    def touches(t):
        t["s"][12] = 0
        return -2
    with pytest.raises(AssertionError, match="s: kept"):
        bands.check_refusal(bufs, touches, CPU, -2)

    def touches_band(t):
        _raw(t, "d", 24)[0] = 0
        return -2
    with pytest.raises(AssertionError, match="d: after"):
        bands.check_refusal(bufs, touches_band, CPU, -2)


def test_arena_memory_is_kept_and_reused_then_released():
    bufs = _bufs()
    a = bands.Arena(bufs, CPU, bands.Fill(0xFF))
    base = a.mem.data_ptr()
    del a
    b = bands.Arena(bufs[:2], CPU, bands.Fill(0x00))                 # a smaller launch is carved from the same allocation
    assert b.mem.data_ptr() == base and float(b.tensors["y"].abs().sum()) == 0.0
    rep = bands.check(bufs, _good, CPU)                               # run() copies each fill's outputs out before the next arena takes the memory
    assert float(rep.outputs["y"].view(torch.float32)[5]) == 5.0
    bands.release(CPU)
    assert CPU not in bands._storage


# ---- the stream runs: every streamed entry point has a test, every exemption quotes the header ---------------------------------------------
def _header():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "probav_hip.h")) as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    streamed = {m.group(1) for m in re.finditer(r"\b(probav_\w+)\s*\(([^;{}()]*)\)\s*;", code) if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip())}
    return " ".join(text.split()), streamed


def test_every_streamed_entry_point_is_held_by_a_test_that_exists():
    from tests import test_gpu_bands as tb, test_gpu_gemm_route as tg
    _, streamed = _header()
    assert len(streamed) == 52 and not set(tb.STREAMED) & set(tg.STREAMED)
    assert set(tb.STREAMED) | set(tg.STREAMED) == streamed, sorted(streamed ^ (set(tb.STREAMED) | set(tg.STREAMED)))
    assert sorted(tg.STREAMED) == ["probav_gemm_conv3d_forward", "probav_gemm_conv3d_wgrad"]
    for mod, table in ((tb, tb.STREAMED), (tg, tg.STREAMED)):
        for entry, test in table.items():
            assert test.startswith("test_") and callable(getattr(mod, test, None)), (entry, test)
            src = __import__("inspect").getsource(getattr(mod, test))
            helpers = "".join(__import__("inspect").getsource(getattr(mod, h)) for h in ("_conv_forward", "_conv_wgrad") if hasattr(mod, h) and h + "(" in src)
            assert entry + "(" in src + helpers, "%s does not call %s" % (test, entry)


def test_every_host_wait_exemption_quotes_the_header():
    from tests import test_gpu_bands as tb
    text, streamed = _header()
    text = text.replace(" * ", " ")                        # (the comment's line prefix)
    assert set(tb.HOST_WAIT_EXEMPT) <= set(tb.STREAMED)
    for entry, (sentence, applies) in tb.HOST_WAIT_EXEMPT.items():
        assert " ".join(sentence.split()) in text, "%s: not a sentence of include/probav_hip.h: %s" % (entry, sentence)
        assert callable(applies)


def test_host_wait_exemptions_apply_to_the_calls_the_header_names_and_no_others():
    import ctypes
    from tests import test_gpu_bands as tb
    ex = tb._host_wait_exempt
    h1, h2 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    fwd = lambda h: ("probav_forward", (h, None, None, None, None, 0, 1, 0, None))
    assert ex([fwd(h1)], []) and ex([fwd(h2)], [fwd(h1)])              # an engine's first call
    assert ex([fwd(ctypes.c_void_p(0x1000))], [fwd(h1)]) is None        # the same engine again (another handle object of the same value)
    assert ex([fwd(h1), fwd(h1)], []) and ex([("probav_clip_round", (None,) * 6)], []) is None
    conv = lambda impl: ("probav_conv3d_forward", (None,) * 7 + (impl, None))
    assert ex([conv(0)], []) is None and all(ex([conv(i)], [conv(i)]) for i in (1, 2, 3, 4))
    assert ex([("probav_pw_forward", (None,) * 11)], []) and ex([("probav_pw_backward", (None,) * 18)], [])
    loss = lambda B, border: ("probav_shift_loss_forward", (None, None, None, B, 48, border) + (None,) * 9)
    assert ex([loss(2, 3)], []) and ex([loss(2, 3)], [loss(2, 3)]) is None and ex([loss(3, 3)], [loss(2, 3)]) and ex([loss(5, 2)], [loss(3, 3)]) is None
    g = lambda N: ctypes.byref((ctypes.c_int32 * 17)(N))
    wgrad = lambda N, impl: ("probav_conv3d_wgrad", (g(N),) + (None,) * 7 + (impl, None))
    assert ex([wgrad(2, 4)], []) and ex([wgrad(2, 4)], [wgrad(2, 4)]) is None and ex([wgrad(3, 4)], [wgrad(2, 4), wgrad(9, 3)]) and ex([wgrad(9, 3)], []) is None


def test_the_recording_library_notes_calls_in_order():
    from tests import late_stream

    class Lib:
        def probav_a(self, x):
            return x + 1
    rec = late_stream.recording(Lib())
    mark = len(late_stream.history)
    assert rec.probav_a(1) == 2 and rec.probav_a(5) == 6 and late_stream.history[mark:] == [("probav_a", (1,)), ("probav_a", (5,))]
    assert late_stream.recording(rec._cdll) is rec
