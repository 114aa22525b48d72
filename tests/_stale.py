"""Stale state: does an entry's result depend on what the scratch arena, or a handle, held before the call?

Every verb borrows its temporary device memory from one cached arena (kmap_scratch in csrc/api_core.hip: one buffer per device,
stream and slot, grown on demand with 1/8 head-room, never cleared), and the handles keep buffers that only ever grow.  Counters,
cursors and bit masks in them are right only if every such word was cleared or fully overwritten earlier in the same call.  Two
things hide a missing clear from a suite that runs in one fixed order: fresh device memory is zero, and the head-room beyond the
bytes asked for is never written.  `states` takes both away:

  cold   kmap_scratch_release(0) first, as in a fresh process; then case()
  0x00   primer() -- a LARGER instance of the same family, so that every slot is larger than the case needs and its tail is
         stale --, kmap_scratch_fill(0x00), then case()
  0x5A   primer(), kmap_scratch_fill(0x5A), case()
  0xFF   primer(), kmap_scratch_fill(0xFF), case()         (mildest first)

The four results must be bit for bit the case's REFERENCE -- the oracle or host model the entry's own test uses, never another
run of the entry -- and kmap_scratch_acquired must have advanced during every run of the case: a case that took a path without
scratch proves nothing.  `reused` does the same for a handle: small() on a handle that has just run big() must equal small() on a
fresh handle and the reference.

A failure is a StaleError whose `kind` says what was seen:
  unused     the case took no scratch (states) -- it cannot discriminate
  unfilled   the fill found no cached buffer after the primer -- it cannot discriminate
  undersized the primer left no more bytes in the arena than the case alone -- no slot has a stale tail
  cold       the cold run differs from the reference: the case is wrong without any stale state
  warm       the run after a fill with zeros differs: the primer left something behind outside the arena's bytes (a handle, a
             size the library remembers)
  stale      only a run after a non-zero fill differs: the entry read arena bytes it had not written in this call -- a counter
             that is not cleared, a clear that is short, or a read beyond the carved size
  fresh      small() on a fresh handle differs from the reference (reused)
  handle     small() after big() on the same handle differs: a buffer that survived big() is read before it is written
`state` names the run and `array` the first result that differs.

The arena is a parameter, so that tests/test_stale_host.py can run the choreography against a numpy stand-in with planted
defects.  It needs release(), fill(byte) -> (buffers, bytes) and acquired() -> int."""
import ctypes as C
import re

import numpy as np

FILLS = (0x00, 0x5A, 0xFF)


class StaleError(AssertionError):
    def __init__(self, kind, state, array, msg):
        super().__init__(msg)
        self.kind, self.state, self.array = kind, state, array


class Arena:
    """the library's arena on the current device"""

    def __init__(self):
        from kmap_amd import _ffi
        self._ffi, self.L = _ffi, _ffi.lib()

    def release(self):
        self._ffi.check(self.L.kmap_scratch_release(0))

    def fill(self, byte):
        nb, nbytes = C.c_int64(-1), C.c_int64(-1)
        self._ffi.check(self.L.kmap_scratch_fill(int(byte), C.byref(nb), C.byref(nbytes)))
        return nb.value, nbytes.value

    def acquired(self):
        n = C.c_int64(-1)
        self._ffi.check(self.L.kmap_scratch_acquired(C.byref(n)))
        return n.value


_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = Arena()
    return _arena


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same(a, b):
    """bit for bit: shape, dtype and bytes"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bytes(a), _bytes(b))


def _as_dict(res):
    if isinstance(res, dict):
        return {k: np.asarray(v) for k, v in res.items()}
    if isinstance(res, (tuple, list)):
        return {str(i): np.asarray(v) for i, v in enumerate(res)}
    return {"0": np.asarray(res)}


def first_difference(got, want):
    """None, or (array name, text) of the first array of `got` that is not bit for bit `want`'s"""
    got, want = _as_dict(got), _as_dict(want)
    if sorted(got) != sorted(want):
        return "<names>", f"the result has the arrays {sorted(got)}, the reference {sorted(want)}"
    for k in sorted(want):
        g, w = got[k], want[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            return k, f"array '{k}' is {g.dtype}{g.shape}, the reference {w.dtype}{w.shape}"
        if not same(g, w):
            at = int(np.flatnonzero(g.reshape(-1) != w.reshape(-1))[0]) if g.dtype.kind != "f" else \
                int(np.flatnonzero(_bytes(g) != _bytes(w))[0]) // g.dtype.itemsize
            return k, f"array '{k}' differs from the reference at element {at} of {w.size}: {g.reshape(-1)[at]!r} for {w.reshape(-1)[at]!r}"
    return None


_WHY = {
    "cold": "the case is wrong even on a freshly released arena",
    "warm": "the arena held zeros, so the primer left state behind outside the arena's bytes",
    "stale": "the entry read arena bytes that it had not written in this call: a counter that is not cleared, a clear that is "
             "short, or a read beyond the carved size",
}


def states(name, case, primer, reference=None, arena_=None, check=None):
    """case() in the four arena states (cold, then behind primer() and a fill with 0x00, 0x5A, 0xFF: fixed, mildest first).
    Every result must be bit for bit `reference` (a dict of arrays, a tuple of arrays or one array, like case()'s result).  Where
    the entry's own test holds floating-point results to its model within a bound and not bit for bit, pass check(result) instead:
    it is applied to the cold result (and raises on a miss), and the three warm results must be bit for bit the cold one.
    The primer must be larger than the case: after it the arena must hold more bytes than after the cold run, unless every buffer
    is at the arena's 4096-byte minimum in both (then the case's tail inside the minimum is what is stale).  Returns the cold result."""
    A = arena_ or arena()
    assert (reference is None) != (check is None), "a reference, or the check of the entry's own test"

    def one(state):
        before = A.acquired()
        got = case()
        if A.acquired() <= before:
            raise StaleError("unused", state, None, f"{name}: [{state}] the case took no scratch from the arena: it cannot tell a "
                                                    "stale arena from a clean one")
        return got
    A.release()
    cold = one("cold")
    if check is not None:
        check(cold)
        reference = cold
    d = first_difference(cold, reference)
    if d:
        raise StaleError("cold", "cold", d[0], f"{name}: [cold] {d[1]}: {_WHY['cold']}")
    cold_buffers, cold_bytes = A.fill(0x00)                   # how much the case alone takes; its run is over
    for byte in FILLS:
        primer()
        n_buffers, n_bytes = A.fill(byte)
        state = f"0x{byte:02X}"
        if n_buffers < 1 or n_bytes < 1:
            raise StaleError("unfilled", state, None, f"{name}: [{state}] the arena holds no buffer after the primer: the fill set nothing")
        at_minimum = n_bytes == 4096 * n_buffers and cold_bytes == 4096 * cold_buffers
        if n_bytes < cold_bytes or (n_bytes == cold_bytes and not at_minimum):
            raise StaleError("undersized", state, None, f"{name}: [{state}] the arena holds {n_bytes} bytes after the primer and {cold_bytes} "
                                                        "after the case alone: the primer is no larger instance, no slot has a stale tail")
        d = first_difference(one(state), reference)
        if d:
            kind = "warm" if byte == 0 else "stale"
            raise StaleError(kind, state, d[0], f"{name}: [after the primer and a fill with {state}] {d[1]}: {_WHY[kind]}")
    return cold


def reused(name, handle_factory, big, small, reference, close=None):
    """small(h) on a handle that has just run big(h) must be bit for bit small(h) on a fresh handle and `reference`.
    handle_factory() -> h; close(h) ends one (default: h.close() where it exists)."""
    def end(h):
        if close is not None:
            close(h)
        elif hasattr(h, "close"):
            h.close()
    h = handle_factory()
    try:
        fresh = small(h)
    finally:
        end(h)
    d = first_difference(fresh, reference)
    if d:
        raise StaleError("fresh", "fresh", d[0], f"{name}: [fresh handle] {d[1]}")
    h = handle_factory()
    try:
        big(h)
        got = small(h)
    finally:
        end(h)
    d = first_difference(got, reference)
    if d:
        raise StaleError("handle", "reused", d[0], f"{name}: [after a larger run on the same handle] {d[1]}: a buffer of the handle that "
                                                   "survived the larger run is read before this run writes it")
    return got


# ---- which audit rows have a case -------------------------------------------------------------------------------------------------
REGISTERED = {}            # entry name -> names of the tests that declared it


def covers(*entries):
    """marks a test as the stale-state case of these entries (the decorator of tests/_stream_order.py with a registry of its own:
    the list check of tests/test_gpu_streams.py counts what is registered there).  tests/test_stale_host.py holds DESIGN.md's audit
    rows to this registry: a row's tests must be declared cases of the row's entries."""
    def deco(fn):
        for e in entries:
            REGISTERED.setdefault(e, []).append(fn.__name__)
        return fn
    return deco


AUDIT_HEADING = "Stale scratch and handle state"


def audit_rows(design_text):
    """the rows of the tables of DESIGN.md's section `AUDIT_HEADING`: [(first cell without back-ticks, last cell)].  The first
    cell names the entry (or handle), the last one its case: `test_...` names of tests/test_gpu_stale_state.py, or `none: reason`."""
    m = re.search(r"^#+[^\n]*" + re.escape(AUDIT_HEADING) + r"[^\n]*\n(.*?)(?=^#{1,2} |\Z)", design_text, flags=re.S | re.M)
    assert m, f"DESIGN.md has no section '{AUDIT_HEADING}'"
    rows = []
    for line in m.group(1).splitlines():
        line = line.strip()
        if not line.startswith("|") or re.fullmatch(r"\|[\s:|-]+\|", line):
            continue
        cells = [c.strip() for c in line.strip("|").split("|")]
        if cells[0].lower() in ("entry", "handle"):
            continue
        rows.append((cells[0].replace("`", ""), cells[-1]))
    return rows


def row_case(cell):
    """([test names], reason or None) of a row's last cell"""
    tests = re.findall(r"\btest_\w+\b(?!\.py)", cell)            # not the file names
    m = re.match(r"\s*none:\s*(.+)", cell)
    return tests, (m.group(1).strip() if m else None)
