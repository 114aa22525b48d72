"""tests/_stream_order.py on a numpy stand-in of the device (no GPU): the choreography has to be able to fail.  The stand-in's
streams are lists of deferred calls that run at stream_sync; work given the null stream runs at once, which is what an escaped
launch does while the caller's stream still sits in the delay.  An entry that stays on its stream passes; one that escaped is
reported as having seen the decoy, with the array's name; a decoy that gives the truth's result is refused; a stray byte behind an
output is reported."""
import ctypes

import numpy as np
import pytest

from tests import _stream_order as S
from tests.test_footprint_host import HostBytes


class HostDevice:
    buffer_cls = HostBytes

    def __init__(self):
        self.queues = {}
        self.log = []

    def stream(self, i=0):
        self.queues.setdefault(f"s{i}", [])
        return f"s{i}"

    def launch(self, fn, s):
        """fn() on stream s: deferred until stream_sync(s), at once on the null stream"""
        if s is None:
            fn()
        else:
            self.queues[s].append(fn)

    def delay(self, ms, s):
        assert s is not None and 1 <= ms <= 100
        self.launch(lambda: self.log.append(("delay", ms)), s)

    def d2d(self, dst, src, nbytes, s):
        self.launch(lambda: ctypes.memmove(dst, src, nbytes), s)

    def stream_sync(self, s):
        if s is not None:
            q = self.queues[s]
            while q:
                q.pop(0)()


def _view(ptr, n, dtype):
    return np.frombuffer((ctypes.c_uint8 * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype)


def _double(dev, src, dst, n, s):
    """the 'entry': dst[i] = 2 src[i] as one launch on stream s"""
    def kernel():
        _view(dst, n, np.uint32)[:] = 2 * _view(src, n, np.uint32)
    dev.launch(kernel, s)


TRUTH = np.arange(100, dtype=np.uint32)
DECOY = TRUTH[::-1].copy()


def _case(dev, name="double"):
    c = S.Case(name, dev=dev, delay_ms=7)
    return c, c.input("in", TRUTH, DECOY), c.output("out", TRUTH.nbytes)


def test_an_entry_on_its_stream_passes():
    dev = HostDevice()
    c, i, o = _case(dev)
    c.run(lambda s: _double(dev, i.ptr, o.ptr, 100, s))
    assert dev.log == [("delay", 7)] and not dev.queues["s0"]
    c.expect("out", 2 * TRUTH, 2 * DECOY)
    assert c.observed("out", 2 * TRUTH, 2 * DECOY) == "truth"
    c.finish()


def test_an_escaped_launch_is_reported_with_the_arrays_name():
    dev = HostDevice()
    c, i, o = _case(dev)
    c.run(lambda s: _double(dev, i.ptr, o.ptr, 100, None))            # the entry forgot its stream
    assert c.observed("out", 2 * TRUTH, 2 * DECOY) == "decoy"
    with pytest.raises(S.StreamOrderError) as e:
        c.expect("out", 2 * TRUTH, 2 * DECOY)
    assert e.value.kind == "decoy" and e.value.array == "out"
    assert "double: array 'out' saw the decoy" in str(e.value)
    c.finish()


def test_the_control_switch_gives_the_entry_the_null_stream():
    dev = HostDevice()
    c, i, o = _case(dev)
    seen = []
    c.run(lambda s: (seen.append(s), _double(dev, i.ptr, o.ptr, 100, s)), escape=True)
    assert seen == [None]
    assert c.observed("out", 2 * TRUTH, 2 * DECOY) == "decoy"
    c.finish()


def test_a_planted_decoy_result_on_the_host_is_reported():
    """host outputs go through the same check: `got` is the array the entry filled"""
    dev = HostDevice()
    c, i, o = _case(dev, "count")
    c.run(lambda s: None)
    with pytest.raises(S.StreamOrderError) as e:
        c.expect("n_uniq", np.int64(5), np.int64(7), got=np.int64(7))
    assert e.value.kind == "decoy" and e.value.array == "n_uniq" and "count: array 'n_uniq' saw the decoy" in str(e.value)
    c.expect("n_uniq", np.int64(5), np.int64(7), got=np.int64(5))
    c.finish()


def test_a_decoy_equal_result_is_refused():
    dev = HostDevice()
    c, i, o = _case(dev)
    c.run(lambda s: _double(dev, i.ptr, o.ptr, 100, s))
    with pytest.raises(S.StreamOrderError) as e:
        c.expect("out", 2 * TRUTH, 2 * TRUTH)
    assert e.value.kind == "blind" and e.value.array == "out" and "can detect nothing" in str(e.value)
    c.finish()


def test_a_result_that_is_neither_is_reported_with_the_first_byte():
    dev = HostDevice()
    c, i, o = _case(dev)

    def entry(s):
        _double(dev, i.ptr, o.ptr, 100, s)
        dev.launch(lambda: _view(o.ptr, 100, np.uint32).__setitem__(3, 0xFFFFFFFF), s)
    c.run(entry)
    with pytest.raises(S.StreamOrderError) as e:
        c.expect("out", 2 * TRUTH, 2 * DECOY)
    assert e.value.kind == "wrong" and "first differing byte 12 of 400" in str(e.value)
    c.finish()


def test_an_unwritten_output_is_neither_result():
    """the snapshot of an output the entry never wrote holds the sentinel: not the truth, and not a pass"""
    dev = HostDevice()
    c, i, o = _case(dev)
    c.run(lambda s: None)
    assert np.all(c.snapshot("out", np.uint8) == S.SENTINEL)
    assert c.observed("out", 2 * TRUTH, 2 * DECOY) == "other"
    c.finish()


@pytest.mark.parametrize("off", [-1, 400])
def test_a_broken_sentinel_is_reported(off):
    dev = HostDevice()
    c, i, o = _case(dev)

    def entry(s):
        _double(dev, i.ptr, o.ptr, 100, s)
        dev.launch(lambda: ctypes.memset(o.ptr + off, 0x11, 1), s)
    c.run(entry)
    c.expect("out", 2 * TRUTH, 2 * DECOY)
    with pytest.raises(S.StreamOrderError) as e:
        c.finish()
    assert e.value.kind == "sentinel" and e.value.array == "out" and f"offset {off}" in str(e.value)


def test_in_place_inputs_get_a_snapshot():
    dev = HostDevice()
    c = S.Case("inc", dev=dev)
    b = c.inout("h", TRUTH, DECOY)
    c.run(lambda s: dev.launch(lambda: np.add(_view(b.ptr, 100, np.uint32), 1, out=_view(b.ptr, 100, np.uint32)), s))
    c.expect("h", TRUTH + 1, DECOY + 1)
    c.finish()


def test_a_decoy_of_another_shape_is_refused():
    c = S.Case("shape", dev=HostDevice())
    with pytest.raises(AssertionError):
        c.input("in", TRUTH, DECOY[:-1])


def test_the_header_parser_finds_the_stream_parameter():
    text = """
    /* int kmap_in_a_comment(void *stream); */
    int kmap_a_dev(const uint8_t *x, int64_t n,
                   void *stream);   // int kmap_commented(void *stream);
    int kmap_b(const uint8_t *x, int64_t n);
    int64_t kmap_groups(int64_t n);
    int kmap_c(kmap_counts *c, int64_t *n, void *stream /* optional */);
    int kmap_d(void *ev, void * stream);
    int kmap_e(void *streamer);
    """
    assert S.stream_entries(text) == ["kmap_a_dev", "kmap_c", "kmap_d"]


def test_the_chosen_delay_is_twice_the_measured_one():
    assert S.DELAY_MS == 2 * S.DELAY_MEASURED_MS and S.DELAY_MEASURED_MS in (5, 10, 20, 50) and S.DELAY_MS <= 100


def test_the_real_header_parses_and_the_library_binds_the_delay():
    from pathlib import Path
    from kmap_amd import _ffi
    names = S.stream_entries((Path(__file__).resolve().parents[1] / "include" / "kmap_hip.h").read_text())
    assert "kmap_selftest_delay_dev" in names and "kmap_revcom_u32_dev" in names and "kmap_counts_total" not in names
    assert len(names) == len(set(names)) > 80
    assert set(names) <= set(_ffi.exported_symbols())
