"""The arena: every buffer of one launch carved out of ONE uint8 allocation, at exactly its declared byte length, between guard bands.

What the suite's parity tests cannot see is what a kernel does OUTSIDE the tensors it is handed, and what it takes from memory it was only
meant to write.  A launch is described once (a list of `Buf` and a callable that receives the carved tensors and returns the C return code)
and run three times:

    A   bands, `out` and `scratch` buffers filled with byte 0xFF  (a NaN as fp32 and fp64, 65535 as uint16, -1 as int32, a set mask byte,
        the largest unsigned for an atomicMax)
    B   the same with byte 0x00
    C   plain, separately allocated tensors, as the parity tests use

After A and B: every band still holds its fill byte for byte, every `in` buffer holds its initial bytes, and every `out` / `inout` buffer is
BITWISE equal across A, B and C -- except the elements a `keep` mask names (rows the header says an entry leaves as they were), which must
hold the fill.  Further fills (`Fill(byte, preset={name: bytes})`: a scratch buffer holding an earlier call's state) join the comparison.
Every check is evaluated where the arena lives; one boolean per check crosses to the host, and only a failed check is located (first and
last offending byte offset, relative to the buffer's or the band's first byte).

The arena's memory is one uint8 allocation per device, kept from launch to launch and grown on demand (one arena is alive at a time).
Layout, per buffer in the order given:   [band before][buffer: exactly nbytes][band after, then up to 15 bytes more to the next 16]
A buffer starts 16-byte aligned; a band is at least BAND_MIN bytes and at least one leading-index slice (`lead` bytes: one sample, image or
frame) of the buffer it guards, so a whole extra strip or sample still lands in a band.  The bytes that round a band up belong to the band
and are checked with it.  Works on CPU tensors too (tests/test_bands_host.py).

On a device a fourth run follows (`_late_run`): the same launch on a stream that is still busy with a delay (tests/late_stream.py), the arena
filled and its inputs delivered on that stream behind the delay.  The header's "every call only ENQUEUES work on `stream` and returns" is what
it holds: work that is not on (or forked from) the stream it was given runs before its inputs arrive and the result differs from run A's; a
call that waits on the host returns after the delay ('sync').  It is inert on CPU tensors, for refusals and for expect_rc != 0.

What this cannot see: a READ past the end of an input whose value never reaches the result.  Nothing here proves reads in bounds.
"""
import numpy as np
import torch

BAND_MIN = 64 * 1024
ALIGN = 16
ROLES = ("in", "out", "inout", "scratch")


def _bytes_of(data):
    """The bytes of a tensor / array as a flat uint8 CPU tensor."""
    if isinstance(data, torch.Tensor):
        return data.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()
    a = np.ascontiguousarray(data)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy())


class Buf:
    """One buffer of a launch.  nbytes: the declared length, exactly (default: that of `init`); role: in / out / inout / scratch; init: the
    initial data of an `in` / `inout` buffer (tensor or array, any shape); lead: bytes of one leading-index slice (default: the whole buffer);
    keep: boolean array over the buffer's ELEMENTS (any shape, dtype's item size) naming those the launch must leave as they were."""

    def __init__(self, name, dtype, role, nbytes=None, init=None, lead=None, keep=None):
        assert role in ROLES, role
        self.name, self.dtype, self.role = name, dtype, role
        self.item = torch.empty(0, dtype=dtype).element_size()
        self.init = None if init is None else _bytes_of(init)
        if role in ("in", "inout"):
            assert self.init is not None, "%s: an %s buffer needs initial data" % (name, role)
        else:
            assert self.init is None, "%s: an %s buffer takes no initial data" % (name, role)
        self.nbytes = int(self.init.numel() if nbytes is None else nbytes)
        assert self.nbytes >= 0 and self.nbytes % self.item == 0, "%s: %d bytes is no whole number of elements" % (name, self.nbytes)
        assert self.init is None or self.init.numel() == self.nbytes, "%s: initial data of %d bytes for %d" % (name, self.init.numel(), self.nbytes)
        self.lead = int(self.nbytes if lead is None else lead)
        self.keep = None
        if keep is not None:
            k = np.asarray(keep, bool).reshape(-1)
            assert k.size * self.item == self.nbytes, "%s: keep mask of %d elements" % (name, k.size)
            self.keep = torch.from_numpy(np.repeat(k, self.item))


def out(name, dtype, count, lead_count=None, keep=None, role="out"):
    """An output of `count` elements (lead_count: elements of one leading-index slice)."""
    item = torch.empty(0, dtype=dtype).element_size()
    return Buf(name, dtype, role, nbytes=int(count) * item, lead=None if lead_count is None else int(lead_count) * item, keep=keep)


def scratch(name, nbytes, dtype=torch.uint8):
    return Buf(name, dtype, "scratch", nbytes=nbytes)


def inp(name, data, role="in", dtype=None):
    """An input holding `data` (tensor or array); one leading-index slice is data[0]."""
    t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
    lead = t[0].numel() * t.element_size() if t.dim() > 1 else None
    return Buf(name, dtype or t.dtype, role, init=t, lead=lead)


class Fill:
    """A fill: the byte of the bands and of every out / scratch buffer, and optionally the bytes some of those buffers hold instead."""

    def __init__(self, byte, preset=None, label=None):
        self.byte, self.preset = int(byte), dict(preset or {})
        self.label = label or "0x%02X" % self.byte


def band_bytes(buf):
    n = max(BAND_MIN, buf.lead)
    return (n + ALIGN - 1) // ALIGN * ALIGN


def carve(bufs):
    """The layout: [(before_off, buf_off, after_off, end_off)] per buffer, and the arena's length.  Offsets are relative to a 16-byte
    aligned base; before = [before_off, buf_off), buffer = [buf_off, buf_off + nbytes), after = [after_off, end_off)."""
    plan, off = [], 0
    for b in bufs:
        band = band_bytes(b)
        before, start = off, off + band
        after = start + b.nbytes
        end = (after + band + ALIGN - 1) // ALIGN * ALIGN
        plan.append((before, start, after, end))
        off = end
    return plan, off


class Violation:
    """One failed check: buffer name, side ('before' / 'after': a band; 'in': an input changed; 'kept': an element that had to keep its fill;
    'differs': an output differs between two runs; 'rc': the return code; 'sync': the call waited on the host), the fill's label ('late': the run on the
    late stream), first and last offending byte offset."""

    def __init__(self, buffer, side, fill, first=None, last=None, note=""):
        self.buffer, self.side, self.fill, self.first, self.last, self.note = buffer, side, fill, first, last, note

    def key(self):
        return (self.buffer, self.side, self.first, self.last)

    def __repr__(self):
        return "%s: %s [fill %s] bytes %s..%s %s" % (self.buffer, self.side, self.fill, self.first, self.last, self.note)


def _span(bad):
    """First and last set index of a boolean tensor (only on a failed check)."""
    idx = torch.nonzero(bad.reshape(-1))
    return int(idx[0]), int(idx[-1])


class Arena:
    def __init__(self, bufs, device, fill, deliver=True):
        self.bufs, self.fill, self.device = list(bufs), fill, torch.device(device)
        names = [b.name for b in self.bufs]
        assert len(set(names)) == len(names), "buffer names must differ"
        self.plan, total = carve(self.bufs)
        self.mem = _arena_bytes(self.device, total)
        self.tensors, self.views = {}, {}
        for b, (before, start, after, end) in zip(self.bufs, self.plan):
            v = self.mem[start:start + b.nbytes]
            if b.init is None and b.name in fill.preset:
                p = fill.preset[b.name]
                assert p.numel() == b.nbytes, "%s: preset of %d bytes for %d" % (b.name, p.numel(), b.nbytes)
            self.views[b.name] = v
            self.tensors[b.name] = v.view(b.dtype)
            assert self.tensors[b.name].data_ptr() % ALIGN == 0
        if deliver:
            self.deliver(self.staged())

    def staged(self):
        """[(view, bytes on the arena's device)]: the initial data of the in / inout buffers and the fill's presets, ready to be delivered."""
        src = [(b.name, b.init if b.init is not None else self.fill.preset.get(b.name)) for b in self.bufs]
        return [(self.views[n], d.to(self.device)) for n, d in src if d is not None]

    def deliver(self, staged):
        """The fill of the whole arena, then the staged bytes (device to device): enqueued on the current stream."""
        self.mem.fill_(self.fill.byte)
        for v, d in staged:
            v.copy_(d)

    def checks(self, untouched=False):
        """[(buffer, side, bad-bytes tensor)]: the bands, the inputs, the kept elements; with untouched, every out / scratch buffer whole."""
        res = []
        for b, (before, start, after, end) in zip(self.bufs, self.plan):
            res.append((b.name, "before", self.mem[before:start] != self.fill.byte))
            res.append((b.name, "after", self.mem[after:end] != self.fill.byte))
            v = self.views[b.name]
            if b.role == "in" or (untouched and b.role == "inout"):
                res.append((b.name, "in", v != b.init.to(self.device)))
            elif untouched and b.name not in self.fill.preset:
                res.append((b.name, "kept", v != self.fill.byte))
            elif untouched:
                res.append((b.name, "kept", v != self.fill.preset[b.name].to(self.device)))
            elif b.keep is not None and b.role == "out":
                res.append((b.name, "kept", (v != self.fill.byte) & b.keep.to(self.device)))
            elif b.keep is not None:
                res.append((b.name, "kept", (v != b.init.to(self.device)) & b.keep.to(self.device)))
        return res

    def violations(self, untouched=False):
        res = self.checks(untouched)
        flags = torch.stack([bad.any() for _, _, bad in res]).cpu().tolist() if res else []      # one boolean per check crosses
        return [Violation(n, side, self.fill.label, *_span(bad)) for (n, side, bad), f in zip(res, flags) if f]


def _plain(bufs, device):
    """Run C's tensors: separately allocated, as the parity tests allocate them."""
    ts = {}
    for b in bufs:
        if b.init is not None:
            ts[b.name] = b.init.to(device).clone().view(b.dtype)
        else:
            ts[b.name] = torch.empty(b.nbytes, dtype=torch.uint8, device=device).view(b.dtype)
    return ts


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


_storage = {}                    # device -> the uint8 tensor every arena on that device is carved from


def _arena_bytes(device, nbytes):
    """The arena's memory: one allocation, kept from launch to launch and grown when a launch needs more.  No two arenas have one size, and some
    take gigabytes: allocated afresh each time they would either stay reserved in the caching allocator, block beside block, until the device is
    full for the tests that run afterwards, or cost a free and an allocation per launch.  ONE arena is alive at a time: run() copies the outputs
    of a fill out before the next fill's arena takes the memory."""
    device = torch.device(device)
    have = _storage.get(device)
    if have is None or have.numel() < nbytes + ALIGN:
        _storage.pop(device, None)
        del have
        release(device, storage=False)
        _storage[device] = torch.empty((nbytes + ALIGN + (1 << 26) - 1) >> 26 << 26, dtype=torch.uint8, device=device)
    raw = _storage[device]
    shift = (-raw.data_ptr()) % ALIGN
    return raw[shift:shift + nbytes]


def release(device, storage=True):
    """Hand the arena's memory (and what the caching allocator holds of the plain runs) back to the device: a module's teardown calls it."""
    device = torch.device(device)
    if storage:
        _storage.pop(device, None)
    if device.type == "cuda":
        torch.cuda.empty_cache()


FILLS = (Fill(0xFF), Fill(0x00))


class Report:
    def __init__(self):
        self.violations, self.rcs, self.outputs = [], {}, {}
        self.late_exempt = None          # why the late run's host-wait check was skipped (host_wait_exempt's answer), or None

    def ok(self):
        return not self.violations

    def __str__(self):
        return "\n".join(repr(v) for v in self.violations) or "clean"


host_wait_exempt = None          # set by a test module: callable([(entry point, args)] of the late launch, the same of every call before it) -> the reason it may wait on the host, or None


def _late_run(bufs, call, device, fill, first, rep):
    """The launch once more, on the late stream of tests/late_stream.py.  The arena still holds the complete, valid state the last fill's run left
    (a kernel that escapes to another stream runs at once and must read valid inputs).  Enqueued on the stream, behind its delay: the fill of the
    whole arena, the delivery of the staged inputs and presets, `call` (its `current_stream()` is the late stream).  Whatever did not wait for the
    delay wrote before the fill and is erased.  Checked through that stream alone: bands, inputs and kept elements as after every run, every
    output bitwise against the first run's ('differs', fill '<first> vs late'), and that the call came back while the delay was still running
    ('sync'; repeated once with RETRY_FACTOR times the delay before it is reported)."""
    from tests import late_stream
    dev = torch.device(device)
    a = Arena(bufs, dev, fill, deliver=False)
    staged = a.staged()
    s = late_stream.stream(dev)
    for factor in (1, late_stream.RETRY_FACTOR):
        found = []
        torch.cuda.synchronize(dev)
        mark = len(late_stream.history)
        gate = late_stream.begin(dev, factor)
        with torch.cuda.stream(s):
            a.deliver(staged)
            rc = call(a.tensors)
            early = gate.returned(", ".join(sorted({n for n, _ in late_stream.history[mark:]})))
            reason = host_wait_exempt(late_stream.history[mark:], late_stream.history[:mark]) if host_wait_exempt else None
            if rc != 0:
                found.append(Violation("(call)", "rc", "late", note="returned %r, expected 0" % (rc,)))
            found += a.violations()
            for v in found:
                v.fill = "late"
            res = []
            for b in bufs:
                if b.role in ("out", "inout"):
                    bad = first[b.name] != a.views[b.name]
                    res.append((b.name, bad if b.keep is None else bad & ~b.keep.to(dev)))
            flags = torch.stack([bad.any() for _, bad in res]).cpu().tolist() if res and rc == 0 else []
            found += [Violation(n, "differs", "%s vs late" % fill.label, *_span(bad)) for (n, bad), f in zip(res, flags) if f]
        s.synchronize()
        if not early and reason:
            late_stream.note_wait(reason.split(":")[0])
        if early or reason:
            break
        if factor == 1:
            late_stream.stats["retries"] += 1
        else:
            found.append(Violation("(call)", "sync", "late", note="the call returned only after a delay of %d x %.1f ms on its stream had passed: it waited on the host (%s)"
                                   % (factor, late_stream.delay_ms(dev), gate.what or "entry points not recorded")))
    rep.rcs["late"] = rc
    rep.late_exempt = reason
    rep.violations += found
    del a


def run(bufs, call, device, fills=FILLS, plain=True, expect_rc=0, compare=True, late=True):
    """Run the launch under every fill and once on plain tensors; returns a Report (see the module docstring for the checks).
    report.outputs: {name: uint8 tensor} the out / inout buffers of the first run (copies), for a caller that wants to hold the values to
    something else too.  late: one more run on a late stream (_late_run; device tensors and accepted launches only)."""
    rep, runs = Report(), []
    results = [b.name for b in bufs if b.role in ("out", "inout")]
    for f in fills:
        a = Arena(bufs, device, f)
        rc = call(a.tensors)
        _sync(device)
        rep.rcs[f.label] = rc
        if rc != expect_rc:
            rep.violations.append(Violation("(call)", "rc", f.label, note="returned %r, expected %r" % (rc, expect_rc)))
        rep.violations += a.violations()
        runs.append((f.label, {n: a.views[n].clone() for n in results}))
        del a
    if plain:
        ts = _plain(bufs, device)
        rc = call(ts)
        _sync(device)
        rep.rcs["plain"] = rc
        if rc != expect_rc:
            rep.violations.append(Violation("(call)", "rc", "plain", note="returned %r, expected %r" % (rc, expect_rc)))
        runs.append(("plain", {n: t.reshape(-1).view(torch.uint8) for n, t in ts.items()}))
    rep.outputs = runs[0][1]
    if compare and expect_rc == 0 and all(rc == 0 for rc in rep.rcs.values()):
        label0, first = runs[0]
        res = []
        for b in bufs:
            if b.role not in ("out", "inout"):
                continue
            live = None if b.keep is None else ~b.keep.to(device)
            for label, views in runs[1:]:
                bad = first[b.name] != views[b.name]
                res.append((b.name, "%s vs %s" % (label0, label), bad if live is None else bad & live))
        flags = torch.stack([bad.any() for _, _, bad in res]).cpu().tolist() if res else []
        rep.violations += [Violation(n, "differs", lab, *_span(bad)) for (n, lab, bad), f in zip(res, flags) if f]
    if late and torch.device(device).type == "cuda" and expect_rc == 0 and all(rc == 0 for rc in rep.rcs.values()):
        _late_run(bufs, call, device, fills[0], runs[0][1], rep)
    return rep


def check(bufs, call, device, **kw):
    """run(), and raise with the report when any check failed."""
    rep = run(bufs, call, device, **kw)
    assert rep.ok(), "band / fill-independence checks failed:\n%s" % rep
    return rep


def check_refusal(bufs, call, device, expect_rc, fill=FILLS[0]):
    """The `size - 1` call: `call` declares one byte less than a full-sized carved buffer holds.  The return code must be the refusal and
    nothing -- band, input, output, scratch -- may have been touched."""
    a = Arena(bufs, device, fill)
    rc = call(a.tensors)
    _sync(device)
    v = a.violations(untouched=True)
    del a
    if rc != expect_rc:
        v.insert(0, Violation("(call)", "rc", fill.label, note="returned %r, expected the refusal %r" % (rc, expect_rc)))
    assert not v, "a refused call touched memory or was not refused:\n%s" % "\n".join(map(repr, v))
