"""Stream order of the device entry points: does every step of an entry run on the stream its caller gave it?

include/kmap_hip.h promises that the device-pointer entries are asynchronous on `stream`.  A launch, memset or copy inside an entry
that forgot the stream runs on the null stream instead; as long as the caller passes NULL nobody can tell.  `Case` makes it visible
on a stream of kmap_stream_create (hipStreamNonBlocking: no implicit order with the null stream):

  1. every device input exists twice on the host, the TRUTH and a DECOY: a valid input of the same shape whose result differs;
  2. the device inputs hold the decoy, the outputs a sentinel byte; the streams are drained;
  3. on the stream S, with no host synchronisation in between: kmap_selftest_delay_dev(D, S); kmap_memcpy_d2d(input <- truth, S) for
     every input, from a second device copy uploaded beforehand; the entries under test with stream = S;
     kmap_memcpy_d2d(snapshot <- output, S) for every device output;
  4. kmap_stream_sync(S); the snapshots and the host outputs must equal the expected result of the truth;
  5. the expected result of the decoy must differ from it -- `expect` refuses a case that could detect nothing -- and the guard band
     around every buffer must be intact (tests/_footprint.Guarded).

A step that escaped to the null stream runs while S still sits in the delay: it reads the decoy (or writes what a later step on S
overwrites), and step 4 reports that the array "saw the decoy".  The control of tests/test_gpu_streams.py passes stream = NULL to
three entries on purpose and must see exactly that.

The device is a parameter (`Device`), so that tests/test_stream_order_host.py can run the choreography against a numpy stand-in
whose streams are lists of deferred calls.  It needs: buffer_cls (the surface tests/_footprint.Guarded uses), stream(i),
delay(ms, s), d2d(dst, src, nbytes, s), stream_sync(s)."""
import ctypes as C
import functools
import re

import numpy as np

from tests import _footprint as F

# Measured on one MI355X with the three control cases of tests/test_gpu_streams.py (20 repetitions per delay): the control saw the
# decoy in 20 of 20 repetitions at 5, 10, 20 and 50 ms alike.  The smallest is 5 ms, so the cases wait twice that.
DELAY_MEASURED_MS = 5
DELAY_MS = 10
assert DELAY_MS == 2 * DELAY_MEASURED_MS <= 100

SENTINEL = 0xA5            # fill of the outputs and of every guard band
SNAP_FILL = 0x5A           # fill of the snapshots: a snapshot copy that never ran shows neither the sentinel nor a result


class StreamOrderError(AssertionError):
    """`kind`: blind (the decoy's result equals the truth's), decoy (the array holds the decoy's result), wrong (neither result),
    sentinel (a guard band was written); `array` names the buffer"""

    def __init__(self, kind, array, msg):
        super().__init__(msg)
        self.kind, self.array = kind, array


class Device:
    """the library's streams, copies and delay kernel"""

    def __init__(self):
        from kmap_amd import _ffi
        self._ffi, self.L = _ffi, _ffi.lib()
        self.buffer_cls = F.device_buffer_cls()
        self._streams = []

    def stream(self, i=0):
        """the i-th stream of this device object, created on first use; `destroy_streams` ends them all"""
        while len(self._streams) <= i:
            p = C.c_void_p()
            self._ffi.check(self.L.kmap_stream_create(C.byref(p)))
            assert p.value, "kmap_stream_create returned the null stream"
            self._streams.append(C.c_void_p(p.value))
        return self._streams[i]

    def destroy_streams(self):
        n = len(self._streams)
        while self._streams:
            self._ffi.check(self.L.kmap_stream_destroy(self._streams.pop()))
        return n

    def delay(self, ms, s):
        self._ffi.check(self.L.kmap_selftest_delay_dev(ms, s))

    def d2d(self, dst, src, nbytes, s):
        self._ffi.check(self.L.kmap_memcpy_d2d(dst, src, nbytes, s))

    def stream_sync(self, s):
        self._ffi.check(self.L.kmap_stream_sync(s))


_device = None


def device():
    global _device
    if _device is None:
        _device = Device()
    return _device


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same(a, b):
    """bit for bit: shape, dtype and bytes"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bytes(a), _bytes(b))


class _Buf:
    def __init__(self, name, live, truth_dev, snap):
        self.name, self.live, self.truth_dev, self.snap = name, live, truth_dev, snap
        self.ptr, self.nbytes = live.ptr, live.nbytes


class Case:
    """one run of the choreography; see the module's docstring.  `escape=True` in run() is the control: the entry gets stream NULL
    while the truth still arrives on S."""

    def __init__(self, name, dev=None, delay_ms=DELAY_MS, stream=0):
        self.name, self.dev, self.delay_ms = name, dev or device(), int(delay_ms)
        self.S = self.dev.stream(stream)
        self.bufs, self._ran = {}, False

    # ---- buffers ----
    def _add(self, name, live, truth_dev, snap):
        assert name not in self.bufs and not self._ran
        self.bufs[name] = b = _Buf(name, live, truth_dev, snap)
        return b

    def _snapshot(self, nbytes):
        s = self.dev.buffer_cls(max(nbytes, 1))
        s.memset(SNAP_FILL, 0, nbytes)
        return s

    def input(self, name, truth, decoy, snapshot=False):
        """a device input: holds the decoy until the truth arrives on S.  truth == decoy is allowed for arrays the case has to
        keep (read borders); the result check decides whether the case as a whole can tell the two apart."""
        truth, decoy = np.ascontiguousarray(truth), np.ascontiguousarray(decoy)
        assert truth.shape == decoy.shape and truth.dtype == decoy.dtype, f"{self.name}: {name}: the decoy has another shape"
        live = F.Guarded.of(decoy, fill=SENTINEL, buffer_cls=self.dev.buffer_cls, name=f"{self.name}: {name}")
        src = self.dev.buffer_cls(max(truth.nbytes, 1))
        src.write(truth, 0)
        return self._add(name, live, src, self._snapshot(truth.nbytes) if snapshot else None)

    def inout(self, name, truth, decoy):
        """an input the entry changes in place: decoy/truth treatment and a snapshot"""
        return self.input(name, truth, decoy, snapshot=True)

    def output(self, name, nbytes):
        live = F.Guarded(nbytes, fill=SENTINEL, buffer_cls=self.dev.buffer_cls, name=f"{self.name}: {name}")
        return self._add(name, live, None, self._snapshot(nbytes))

    # ---- the run ----
    def begin(self):
        """drain the streams, then enqueue on S the delay and the copies that bring the truth (delay_ms 0: no delay)"""
        assert not self._ran
        self._ran = True
        d, S = self.dev, self.S
        d.stream_sync(None)
        d.stream_sync(S)
        if self.delay_ms:
            d.delay(self.delay_ms, S)
        for b in self.bufs.values():
            if b.truth_dev is not None and b.nbytes:
                d.d2d(b.ptr, b.truth_dev.ptr, b.nbytes, S)

    def end(self):
        """enqueue the snapshot copies on S and drain it"""
        d, S = self.dev, self.S
        for b in self.bufs.values():
            if b.snap is not None and b.nbytes:
                d.d2d(b.snap.ptr, b.ptr, b.nbytes, S)
        d.stream_sync(S)

    def run(self, enqueue, escape=False):
        """begin(), enqueue(stream) -- which issues the entries under test --, end(); whatever enqueue returns is returned"""
        self.begin()
        res = enqueue(None if escape else self.S)
        self.end()
        return res

    def snapshot(self, name, dtype, shape=None):
        b = self.bufs[name]
        assert self._ran and b.snap is not None
        dtype = np.dtype(dtype)
        shape = (b.nbytes // dtype.itemsize,) if shape is None else shape
        return b.snap.to_numpy(dtype, shape)

    # ---- the checks ----
    def observed(self, name, want_truth, want_decoy, got=None):
        """'truth' or 'decoy' or 'other': which expected result `got` (default: the snapshot of device buffer `name`) equals.
        Refuses a pair of expectations that cannot be told apart."""
        want_truth, want_decoy = np.asarray(want_truth), np.asarray(want_decoy)
        if same(want_truth, want_decoy):
            raise StreamOrderError("blind", name, f"{self.name}: array '{name}': the decoy's expected result equals the truth's: "
                                                  "this case can detect nothing")
        if got is None:
            got = self.snapshot(name, want_truth.dtype, want_truth.shape)
        got = np.asarray(got)
        return "truth" if same(got, want_truth) else "decoy" if same(got, want_decoy) else "other"

    def expect(self, name, want_truth, want_decoy, got=None):
        if got is None:
            got = self.snapshot(name, np.asarray(want_truth).dtype, np.asarray(want_truth).shape)
        seen = self.observed(name, want_truth, want_decoy, got)
        if seen == "decoy":
            raise StreamOrderError("decoy", name, f"{self.name}: array '{name}' saw the decoy: a step that produces it ran before the "
                                                  "truth arrived on the caller's stream, so it is not ordered on that stream")
        if seen != "truth":
            g, w = _bytes(np.asarray(got)), _bytes(np.asarray(want_truth))
            m = min(len(g), len(w))
            diff = np.flatnonzero(g[:m] != w[:m])
            at = int(diff[0]) if len(diff) else m
            raise StreamOrderError("wrong", name, f"{self.name}: array '{name}' holds neither the truth's nor the decoy's result "
                                                  f"(first differing byte {at} of {len(w)}; {len(g)} bytes found)")

    def finish(self):
        """every guard band intact; the buffers freed"""
        try:
            for b in self.bufs.values():
                try:
                    b.live.check_guards()
                except F.FootprintError as e:
                    raise StreamOrderError("sentinel", b.name, str(e)) from None
        finally:
            for b in self.bufs.values():
                for x in (b.live, b.truth_dev, b.snap):
                    if x is not None:
                        x.free()
            self.bufs = {}


# ---- which entries have a case --------------------------------------------------------------------------------------------------
REGISTERED = {}            # entry name -> names of the tests that declared it


def covers(*entries):
    """marks a test as the case of these stream-taking entries (registered when the module is imported, so that the list check
    does not depend on which tests were selected)"""
    def deco(fn):
        for e in entries:
            REGISTERED.setdefault(e, []).append(fn.__name__)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            return fn(*a, **kw)
        wrapper.covers = entries
        return wrapper
    return deco


def stream_entries(header_text):
    """names of the prototypes of a C header that have a `void *stream` parameter"""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"\b(kmap_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out
