"""A late stream: a stream `s` as torch creates them (non-blocking with respect to the null stream) that is kept busy by a delay, a `gate`
event right behind the delay, and the launch under test enqueued behind both.

include/probav_hip.h: "every call only ENQUEUES work on `stream` and returns; it never synchronises, allocates or frees device memory".  On
the null stream of a fresh process -- where every other GPU test runs -- three mistakes cannot be seen, and here they can:

    work on the wrong stream      a kernel, a memset, a fork or a join that is not on (or from) `s` does not wait for the delay: it runs before
                                  the inputs are delivered, and what it wrote is erased by the delivery.  The result differs from the ordinary run.
    a wrapper that hands over     the same, one level up: the run is under torch.cuda.stream(s), so `_lib.current_stream()` is `s`
    the wrong stream
    a host wait inside the call   the call returns only after the delay has passed: `gate.query()` is true when it comes back

A run goes   stage (outside s, synchronised)  ->  begin(): delay, gate  ->  prepare + launch on s  ->  returned(): gate.query()  ->  results read
through s alone (`.cpu()` under torch.cuda.stream(s)).  No device-wide synchronisation stands between the launch and the comparison: it
would wait for work that another stream finishes late, such as a side stream that was never joined.

The delay is measured, not assumed: `torch.cuda._sleep(cycles)` (or, where that is missing or does nothing, a chain of device copies) is
timed with events once per process and scaled to TARGET_MS.  The module keeps the calibrated length and, per run, the host time between
the gate's record and the call's return -- the time the delay has to cover; summary() prints both.
"""
import time

import torch

TARGET_MS = 30.0
RETRY_FACTOR = 10                # a launch that fails the host-wait check is repeated once with this many times the delay

_state = {}                      # device index -> {"stream", "kind", "unit_ms", "units", "measured_ms", "buf"}
stats = {"runs": 0, "slowest_enqueue_ms": 0.0, "slowest_what": "", "retries": 0, "waited": {}}      # waited: exempted launch -> times it came back after the delay
history = []                     # (entry point, args) of every call made through recording(), in order


def _timed(s, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record(s)
        fn()
        b.record(s)
    b.synchronize()
    return a.elapsed_time(b)


def _calibrate(device):
    s = torch.cuda.Stream(device=device)
    st = {"stream": s}
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        with torch.cuda.stream(s):
            sleep(1000)                                            # (the kernel's first launch loads its code object)
        s.synchronize()
        cycles = 1 << 20
        ms = _timed(s, lambda: sleep(cycles))
        while ms < 2.0 and cycles < (1 << 34):                       # long enough for the events to resolve it
            cycles <<= 2
            ms = _timed(s, lambda: sleep(cycles))
        if ms >= 2.0:
            st.update(kind="sleep", unit_ms=ms / cycles, units=max(1, int(round(TARGET_MS * cycles / ms))))
    if "kind" not in st:                                            # a chain of device copies: 256 MiB each way per link
        buf = torch.empty(2, 1 << 28, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        _timed(s, lambda: buf[1].copy_(buf[0]))
        ms = _timed(s, lambda: [buf[1].copy_(buf[0]) for _ in range(8)]) / 8
        st.update(kind="copies", unit_ms=ms, units=max(1, int(round(TARGET_MS / ms))), buf=buf)
    _state[torch.device(device).index or 0] = st
    st["measured_ms"] = _timed(s, lambda: _delay(st, 1))
    print("late_stream: delay of %.1f ms (target %.0f) = %d %s" % (st["measured_ms"], TARGET_MS, st["units"],
                                                                    "cycles of torch.cuda._sleep" if st["kind"] == "sleep" else "device copies of 256 MiB"))
    return st


def _delay(st, factor):
    if st["kind"] == "sleep":
        torch.cuda._sleep(st["units"] * factor)
    else:
        for _ in range(st["units"] * factor):
            st["buf"][1].copy_(st["buf"][0])


def _st(device):
    device = torch.device(device)
    return _state.get(device.index or 0) or _calibrate(device)


def stream(device):
    """The late stream of `device` (one per process, calibrated on first use)."""
    return _st(device)["stream"]


def delay_ms(device):
    return _st(device)["measured_ms"]


class Gate:
    """One late run: created by begin() with the delay and the gate event already enqueued on the stream."""

    def __init__(self, st, factor, what):
        self.s, self.what, self.factor = st["stream"], what, factor
        self.event = torch.cuda.Event()
        with torch.cuda.stream(self.s):
            _delay(st, factor)
            self.event.record(self.s)
        self.t0 = time.perf_counter()

    def returned(self, what=None):
        """Call when the launch has returned to the host: True if the delay was still running (no host wait inside the call)."""
        self.what = what or self.what
        early = not self.event.query()
        ms = (time.perf_counter() - self.t0) * 1e3
        stats["runs"] += 1
        if early and ms > stats["slowest_enqueue_ms"]:
            stats["slowest_enqueue_ms"], stats["slowest_what"] = ms, self.what
        return early


def begin(device, factor=1, what=""):
    """Everything the launch reads must already be a device tensor and the device idle (torch.cuda.synchronize()): a pageable host-to-device copy
    behind the delay would hold the host until the delay had passed."""
    return Gate(_st(device), factor, what)


def note_wait(what):
    """An exempted launch that did wait on the host: kept for the summary (what the exemption table is in use for)."""
    stats["waited"][what] = stats["waited"].get(what, 0) + 1


def summary():
    if not _state:
        return "late_stream: not used"
    st = next(iter(_state.values()))
    return ("late_stream: delay %.1f ms (%s); %d runs, slowest enqueue it had to cover %.2f ms (%s); %d repeated with %d times the delay; exempted launches that waited: %s"
            % (st["measured_ms"], st["kind"], stats["runs"], stats["slowest_enqueue_ms"], stats["slowest_what"], stats["retries"], RETRY_FACTOR,
               ", ".join("%s x %d" % kv for kv in sorted(stats["waited"].items())) or "none"))


class _Recording:
    """The ctypes library with every entry-point call noted in `history` (name, args): how a harness learns which entry points a launch
    description went through without the description saying so."""

    def __init__(self, cdll):
        self._cdll, self._fns = cdll, {}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            inner = getattr(self._cdll, name)

            def fn(*args):
                history.append((name, args))
                return inner(*args)
            self._fns[name] = fn
        return fn


_recordings = {}


def recording(cdll):
    if id(cdll) not in _recordings:
        _recordings[id(cdll)] = _Recording(cdll)
    return _recordings[id(cdll)]
