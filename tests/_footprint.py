"""Guard bands around device arrays: what a kernel writes outside what it owes, and what it reads outside what it was given.

GPU address sanitizing is not available to this suite, so the only bounds check a kernel can get is a band of known bytes
inside the test's own allocation.  `Guarded` makes ONE buffer of

    front | lead | payload (nbytes) | back

bytes, all set to `fill`, and hands out `ptr` = base + front + lead with base a multiple of 4096: `lead` IS the pointer's
misalignment relative to a 4096-byte boundary (lead = 0: what hipMalloc gives; lead = 1: an odd pointer; lead = 16: 16- but not
4096-byte aligned).  After the launch `check_guards()` requires every byte of front, lead and back to still hold `fill`, and
names the first one that does not by its offset relative to the payload (negative: in front of it; >= nbytes: behind it).

The guards exist so that an overrun stays inside memory the test owns; no test aims at a fault.  `front` and `back` must be at
least as wide as the widest store one workgroup of the kernel under test can issue: 4 KiB (the tile kernel's chunk; 256 threads x
16 bytes elsewhere), plus one row of a pitched output behind it, covers every kernel of this library.  That is the default.

Pitched (2-D) outputs: `Guarded.pitched(nrows, row_bytes, ld)` owns rows [0, nrows) of `row_bytes` bytes at a pitch of `ld`
bytes.  Its payload runs from the first owed byte to the last one, the pad bytes [row_bytes, ld) of the rows in between are
checked by `check_guards()` as well, the last row's pad and the rows behind the range are the back gap (4 KiB + one row), the
rows in front of the range are the front gap: the three checks of tests/test_gpu_hamdist_tail.py.

Outputs are always pre-filled.  Where the fill is a legal output value (0xA5 as a distance byte, 0xA5A5A5A5 as a hash) a case
runs twice, with fill 0xA5 and 0x5A: `check_written(a, b)` reports the first owed byte that holds the fill in BOTH runs, i.e.
was never written.  Inputs go into `Guarded` buffers too, with guard fill 0x00 in one run and 0xFF in the other; the outputs of
the two runs must be identical, so the result may not depend on a byte outside the declared input.  `FILLS` pairs the two.

The buffer class is a parameter so that tests/test_footprint_host.py can plant defects in a numpy-backed stand-in.  It needs:
`cls(nbytes)`, `.ptr`, `.to_numpy(dtype, shape, offset=)`, `.memset(value, offset, nbytes)`, `.write(array, offset)`, `.free()`.
"""
import numpy as np

PAGE = 4096
FILLS = ((0xA5, 0x00), (0x5A, 0xFF))       # (output fill, input guard fill) of the two runs of a case


class FootprintError(AssertionError):
    """`region` is one of front / lead / back / pad / payload; `offset` is in bytes relative to the payload's first byte."""

    def __init__(self, region, offset, msg):
        super().__init__(msg)
        self.region, self.offset = region, int(offset)


_device_cls = None


def device_buffer_cls():
    """_ffi.DeviceBuffer with the memset / write surface `Guarded` uses"""
    global _device_cls
    if _device_cls is None:
        from kmap_amd import _ffi

        class DeviceBytes(_ffi.DeviceBuffer):
            def memset(self, value, offset, nbytes):
                if nbytes:
                    _ffi.check(_ffi.lib().kmap_memset(self.ptr + offset, value, nbytes, None))

            def write(self, a, offset):
                a = np.ascontiguousarray(a)
                if a.nbytes:
                    _ffi.check(_ffi.lib().kmap_memcpy_h2d(self.ptr + offset, _ffi.ptr(a), a.nbytes, None))

        _device_cls = DeviceBytes
    return _device_cls


def _first(mask):
    return int(np.flatnonzero(mask)[0])


class Guarded:
    def __init__(self, nbytes, lead=0, fill=0xA5, front=PAGE, back=PAGE, buffer_cls=None, name="buffer"):
        assert nbytes >= 0 and 0 <= lead < PAGE and 0 <= fill <= 0xFF and front >= 0 and back >= 0
        self.nbytes, self.lead, self.fill, self.front, self.back, self.name = int(nbytes), int(lead), int(fill), int(front), int(back), name
        self.row_bytes = self.ld = self.nrows = None
        cls = buffer_cls or device_buffer_cls()
        total = self.front + self.lead + self.nbytes + self.back
        self.buf = cls(total + PAGE)                       # room to round the base up where the allocator gave less than a page
        self._skip = (-self.buf.ptr) % PAGE
        base = self.buf.ptr + self._skip
        assert base % PAGE == 0
        self._total = total
        self._off = self._skip + self.front + self.lead    # payload's offset inside buf
        self.ptr = base + self.front + self.lead
        self.buf.memset(self.fill, self._skip, total)

    @classmethod
    def pitched(cls, nrows, row_bytes, ld, lead=0, fill=0xA5, front=PAGE, back=None, buffer_cls=None, name="buffer"):
        """rows [0, nrows) of row_bytes bytes, ld bytes apart; the back gap holds the last row's pad and one more row"""
        assert nrows >= 1 and 0 < row_bytes <= ld
        g = cls((nrows - 1) * ld + row_bytes, lead, fill, front, PAGE + ld if back is None else back, buffer_cls, name)
        g.nrows, g.row_bytes, g.ld = int(nrows), int(row_bytes), int(ld)
        return g

    @classmethod
    def of(cls, array, lead=0, fill=0x00, **kw):
        """an input: `array`'s bytes as the payload"""
        a = np.ascontiguousarray(array)
        g = cls(a.nbytes, lead, fill, **kw)
        g.upload(a)
        return g

    # ---- payload ----
    def upload(self, array, offset=0):
        a = np.ascontiguousarray(array)
        assert 0 <= offset and offset + a.nbytes <= self.nbytes, "upload past the payload"
        self.buf.write(a, self._off + offset)

    def upload_rows(self, array2d):
        """a C-contiguous (nrows, row_bytes / itemsize) array into the pitched rows; the pads keep the fill"""
        a = np.ascontiguousarray(array2d)
        assert self.ld is not None and a.shape[0] == self.nrows and a[0].nbytes == self.row_bytes
        for r in range(self.nrows):
            self.buf.write(a[r], self._off + r * self.ld)

    def payload(self, dtype=np.uint8, shape=None):
        dtype = np.dtype(dtype)
        if shape is None:
            assert self.nbytes % dtype.itemsize == 0
            shape = (self.nbytes // dtype.itemsize,)
        assert int(np.prod(shape)) * dtype.itemsize <= self.nbytes
        return self.buf.to_numpy(dtype, shape, offset=self._off)

    def rows(self, dtype=np.uint8):
        """the owed bytes of a pitched payload as (nrows, row_bytes / itemsize), pads dropped"""
        dtype = np.dtype(dtype)
        raw = np.concatenate([self.payload(np.uint8), np.full(self.ld - self.row_bytes, self.fill, np.uint8)])
        return np.ascontiguousarray(raw.reshape(self.nrows, self.ld)[:, :self.row_bytes]).view(dtype)

    # ---- checks ----
    def check_guards(self):
        raw = self.buf.to_numpy(np.uint8, (self._total,), offset=self._skip)
        p0 = self.front + self.lead
        bad = raw != self.fill

        def fail(region, at, what):
            off = at - p0
            raise FootprintError(region, off, f"{self.name}: {what}: byte at payload offset {off} is 0x{raw[at]:02X}, not the fill "
                                              f"0x{self.fill:02X} (payload = {self.nbytes} bytes, lead = {self.lead})")
        if bad[:self.front].any():
            fail("front", _first(bad[:self.front]), "written in front of the array")
        if bad[self.front:p0].any():
            fail("lead", self.front + _first(bad[self.front:p0]), "written in front of the array")
        if self.ld is not None and self.nrows > 1 and self.ld > self.row_bytes:
            body = bad[p0:p0 + (self.nrows - 1) * self.ld].reshape(self.nrows - 1, self.ld)
            pads = body[:, self.row_bytes:]
            if pads.any():
                r, c = np.argwhere(pads)[0]
                fail("pad", p0 + int(r) * self.ld + self.row_bytes + int(c), f"pad byte {self.row_bytes + int(c)} of row {int(r)} written")
        tail = bad[p0 + self.nbytes:]
        if tail.any():
            at = p0 + self.nbytes + _first(tail)
            what = "written behind the array"
            if self.ld is not None:
                off = at - p0
                what = (f"pad byte {off % self.ld} of the last row written" if off < self.nrows * self.ld
                        else f"row {off // self.ld} behind the range written")
            fail("back", at, what)

    def owed_mask(self):
        """True at the payload bytes the kernel owes (all of them; in a pitched payload not the pads)"""
        m = np.ones(self.nbytes, bool)
        if self.ld is not None:
            full = np.ones(self.nrows * self.ld, bool).reshape(self.nrows, self.ld)
            full[:, self.row_bytes:] = False
            m = full.reshape(-1)[:self.nbytes]
        return m

    def free(self):
        self.buf.free()


def check_written(a, b):
    """a, b: the Guarded outputs of two runs of one case with different fills.  A byte that holds the fill in both was never
    written (a written byte holds the same value in both runs, so it can equal at most one of the fills)."""
    assert a.nbytes == b.nbytes and a.fill != b.fill and a.ld == b.ld
    pa, pb = a.payload(np.uint8), b.payload(np.uint8)
    un = (pa == a.fill) & (pb == b.fill) & a.owed_mask()
    if un.any():
        off = _first(un)
        raise FootprintError("payload", off, f"{a.name}: byte at payload offset {off} was never written: it holds the fill in both runs "
                                             f"(0x{a.fill:02X} and 0x{b.fill:02X})")
    diff = (pa != pb) & a.owed_mask()
    if diff.any():
        off = _first(diff)
        raise FootprintError("payload", off, f"{a.name}: byte at payload offset {off} differs between the two runs (0x{pa[off]:02X} vs "
                                             f"0x{pb[off]:02X}): the result depends on the pre-fill or on bytes outside the declared inputs")


def ok(rc):
    """a library call's status checked, and the stream drained so that what follows reads finished results"""
    from kmap_amd import _ffi
    _ffi.check(rc)
    _ffi.sync()


def host(a):
    """void* of a host array argument"""
    import ctypes
    assert a.flags.c_contiguous                                        # a copy made here would be gone before the call reads it
    return a.ctypes.data_as(ctypes.c_void_p)


def guards(*bufs):
    for g in bufs:
        g.check_guards()


def free(*bufs):
    for g in bufs:
        g.free()


def run_twice(case):
    """`case(out_fill, in_fill)` runs the entry once and returns the list of its Guarded OUTPUT buffers (it checks the guards of
    inputs and outputs and the values itself).  Runs it with both pairs of FILLS and requires every owed output byte written and
    identical in both runs.  Frees the outputs."""
    outs = [case(*f) for f in FILLS]
    try:
        for a, b in zip(*outs):
            check_written(a, b)
    finally:
        for run in outs:
            for g in run:
                g.free()
