"""tests/_footprint.py on a numpy-backed stand-in of the device buffer (no GPU): the checker has to be able to fail.  A clean
"kernel" passes; one stray byte just in front of the payload, one just behind it, one in a pad column and one unwritten payload
cell are each reported with the region and the offset relative to the payload."""
import numpy as np
import pytest

from tests import _footprint as F


class HostBytes:
    """the surface Guarded needs, on host memory.  `skew` shifts the bytes inside an over-sized array so that `ptr` is NOT
    page aligned: Guarded has to round its base up itself."""

    def __init__(self, nbytes, skew=24):
        self.nbytes = int(nbytes)
        self._raw = np.zeros(self.nbytes + F.PAGE + skew, np.uint8)
        pad = (-self._raw.ctypes.data) % F.PAGE + skew
        self.mem = self._raw[pad:pad + self.nbytes]
        self.ptr = self.mem.ctypes.data

    def memset(self, value, offset, nbytes):
        assert 0 <= offset and offset + nbytes <= self.nbytes
        self.mem[offset:offset + nbytes] = value

    def write(self, a, offset):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert 0 <= offset and offset + b.size <= self.nbytes
        self.mem[offset:offset + b.size] = b

    def to_numpy(self, dtype, shape, stream=None, offset=0):
        dtype = np.dtype(dtype)
        nb = int(np.prod(shape)) * dtype.itemsize
        assert 0 <= offset and offset + nb <= self.nbytes
        return self.mem[offset:offset + nb].copy().view(dtype).reshape(shape)

    def free(self):
        self.mem = None


def _host_view(g):
    """the bytes a 'kernel' sees through g.ptr: index 0 is the payload's first byte, negative indices reach the front gap"""
    return g.buf.mem, g._off


def _poke(g, off, value):
    mem, p0 = _host_view(g)
    mem[p0 + off] = value


@pytest.mark.parametrize("lead", [0, 1, 15, 16])
def test_pointer_and_clean_run(lead):
    g = F.Guarded(100, lead=lead, buffer_cls=HostBytes)
    assert g.buf.ptr % F.PAGE != 0, "the stand-in is meant to be unaligned"
    assert (g.ptr - lead) % F.PAGE == 0 and g.ptr % F.PAGE == lead
    assert np.all(g.payload(np.uint8) == 0xA5)
    want = np.arange(25, dtype=np.uint32)
    g.upload(want)
    np.testing.assert_array_equal(g.payload(np.uint32), want)
    np.testing.assert_array_equal(g.payload(np.uint32, (5, 5)), want.reshape(5, 5))
    g.check_guards()
    with pytest.raises(AssertionError):
        g.upload(np.zeros(101, np.uint8))
    # the pointer addresses the payload: a write through it lands where payload() reads
    import ctypes
    ctypes.memset(g.ptr + 7, 0x11, 1)
    assert g.payload(np.uint8)[7] == 0x11
    g.check_guards()


@pytest.mark.parametrize("lead", [0, 3])
def test_stray_byte_in_front(lead):
    g = F.Guarded(64, lead=lead, buffer_cls=HostBytes)
    g.upload(np.zeros(64, np.uint8))
    _poke(g, -1, 0)
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert e.value.offset == -1 and e.value.region == ("lead" if lead else "front")
    assert "offset -1" in str(e.value)


def test_stray_byte_far_in_front_and_first_one_wins():
    g = F.Guarded(64, lead=2, buffer_cls=HostBytes)
    _poke(g, -2 - 4096, 1)         # first byte of the front gap
    _poke(g, -1, 1)
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert (e.value.region, e.value.offset) == ("front", -4098)


def test_stray_byte_behind():
    g = F.Guarded(64, lead=5, buffer_cls=HostBytes)
    g.upload(np.zeros(64, np.uint8))
    _poke(g, 64, 0)
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert (e.value.region, e.value.offset) == ("back", 64)
    g2 = F.Guarded(64, buffer_cls=HostBytes)
    _poke(g2, 64 + 4095, 0)         # the last guarded byte
    with pytest.raises(F.FootprintError) as e:
        g2.check_guards()
    assert (e.value.region, e.value.offset) == ("back", 64 + 4095)


def test_fill_valued_stray_byte_needs_the_second_fill():
    """a stray 0xA5 is invisible under fill 0xA5 and seen under 0x5A: why outputs run with both"""
    for fill, seen in ((0xA5, False), (0x5A, True)):
        g = F.Guarded(16, fill=fill, buffer_cls=HostBytes)
        _poke(g, 16, 0xA5)
        if seen:
            with pytest.raises(F.FootprintError):
                g.check_guards()
        else:
            g.check_guards()


def test_pad_column():
    nrows, n, ld = 5, 13, 32
    g = F.Guarded.pitched(nrows, n, ld, lead=1, buffer_cls=HostBytes)
    assert g.nbytes == 4 * 32 + 13 and g.back == F.PAGE + ld
    want = np.arange(nrows * n, dtype=np.uint8).reshape(nrows, n)
    g.upload_rows(want)
    g.check_guards()
    np.testing.assert_array_equal(g.rows(), want)
    _poke(g, 2 * ld + n, 7)          # first pad byte of row 2
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert (e.value.region, e.value.offset) == ("pad", 2 * ld + n)
    assert "pad byte 13 of row 2" in str(e.value)
    # the last row's pad and the row behind the range are the back gap
    g = F.Guarded.pitched(nrows, n, ld, buffer_cls=HostBytes)
    _poke(g, 4 * ld + ld - 1, 7)
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert (e.value.region, e.value.offset) == ("back", 5 * ld - 1) and "pad byte 31 of the last row" in str(e.value)
    g = F.Guarded.pitched(nrows, n, ld, buffer_cls=HostBytes)
    _poke(g, 5 * ld + 3, 7)
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert (e.value.region, e.value.offset) == ("back", 5 * ld + 3) and "row 5 behind the range" in str(e.value)
    # a row in front of the range
    g = F.Guarded.pitched(nrows, n, ld, buffer_cls=HostBytes)
    _poke(g, -ld + 3, 7)
    with pytest.raises(F.FootprintError) as e:
        g.check_guards()
    assert (e.value.region, e.value.offset) == ("front", -ld + 3)


def test_dense_rows_have_no_pad():
    g = F.Guarded.pitched(3, 7, 7, buffer_cls=HostBytes)
    g.upload_rows(np.zeros((3, 7), np.uint8))
    g.check_guards()
    assert g.owed_mask().all() and g.nbytes == 21


def _run(fill, skip=None, wrong=None):
    g = F.Guarded(40, lead=1, fill=fill, buffer_cls=HostBytes)
    out = np.arange(10, dtype=np.uint32) * 0x01010101      # cell 0xA5 would be 0xA5A5A5A5 at index 165: not in here
    out[3] = 0xA5A5A5A5                                    # a legal output value that equals the first fill
    g.upload(out)
    if skip is not None:
        g.buf.memset(fill, g._off + skip, 1)               # the "kernel" forgot this byte
    if wrong is not None:
        _poke(g, wrong, fill ^ 0x0F)                       # ... or derived it from the pre-fill
    return g


def test_unwritten_cell():
    a, b = _run(0xA5), _run(0x5A)
    F.check_written(a, b)            # cell 3 holds 0xA5 bytes in both runs but only equals ONE fill: written
    a, b = _run(0xA5, skip=21), _run(0x5A, skip=21)
    with pytest.raises(F.FootprintError) as e:
        F.check_written(a, b)
    assert (e.value.region, e.value.offset) == ("payload", 21) and "never written" in str(e.value)
    a.check_guards(), b.check_guards()      # an unwritten cell is not a guard violation
    a, b = _run(0xA5, wrong=8), _run(0x5A, wrong=8)
    with pytest.raises(F.FootprintError) as e:
        F.check_written(a, b)
    assert (e.value.region, e.value.offset) == ("payload", 8) and "differs between the two runs" in str(e.value)


def test_unwritten_pad_is_not_owed():
    a = F.Guarded.pitched(2, 3, 8, fill=0xA5, buffer_cls=HostBytes)
    b = F.Guarded.pitched(2, 3, 8, fill=0x5A, buffer_cls=HostBytes)
    for g in (a, b):
        g.upload_rows(np.array([[1, 2, 3], [4, 5, 6]], np.uint8))
    F.check_written(a, b)
    b.buf.memset(0x5A, b._off + 8 + 2, 1)
    a.buf.memset(0xA5, a._off + 8 + 2, 1)
    with pytest.raises(F.FootprintError) as e:
        F.check_written(a, b)
    assert e.value.offset == 10


def test_run_twice_reports_and_frees():
    seen = []

    def case(out_fill, in_fill):
        seen.append((out_fill, in_fill))
        return [_run(out_fill, skip=4)]
    with pytest.raises(F.FootprintError) as e:
        F.run_twice(case)
    assert e.value.offset == 4 and seen == list(F.FILLS)


# ---- tests/_packed_model.py: the numpy packer the GPU cases lean on, against words worked out by hand ----------------------------------
def test_ref_pack_known_words():
    from tests._packed_model import packed_groups, ref_pack
    assert [packed_groups(n) for n in (0, 1, 16, 17, 32, 33)] == [2, 4, 4, 4, 4, 6]
    codes, inval, valid = ref_pack(np.array([0, 1, 2, 3, 255, 7, 3], np.uint8))
    assert len(codes) == packed_groups(7) == 4
    assert codes[0] == 0b00_01_10_11_00_00_11 << 18 and inval[0] == 0b0000_1101_1111_1111
    assert valid[0] == 0b11_11_11_11_00_00_11 << 18
    assert np.all(inval[1:] == 0xFFFF) and np.all(codes[1:] == 0) and np.all(valid[1:] == 0)
    # noise in the code bits of invalid positions leaves the valid ones and the mask alone
    noisy, inval2, valid2 = ref_pack(np.array([0, 1, 2, 3, 255, 7, 3], np.uint8), np.random.default_rng(1))
    assert np.array_equal(noisy & valid, codes) and np.array_equal(inval2, inval) and np.array_equal(valid2, valid)
    # position 16 opens the second group; a full group has no invalid bit
    codes, inval, _ = ref_pack(np.array([3] * 16 + [2], np.uint8))
    assert codes[0] == 0xFFFFFFFF and inval[0] == 0 and codes[1] == 2 << 30 and inval[1] == 0x7FFF


def test_ref_planes_known_words():
    from tests._packed_model import ref_planes
    codes = np.array([0b11_10_01_00 << 24, 0b01 << 0, 0, 0xFFFFFFFF], np.uint32)   # A C G T reversed: T G C A first; C last of 32
    planes = ref_planes(codes)
    assert planes.dtype == np.uint32 and len(planes) == 4
    assert planes[0] == 0b1100 << 28 and planes[1] == (0b1010 << 28) | 1          # high bits; low bits
    assert planes[2] == 0x0000FFFF and planes[3] == 0x0000FFFF
