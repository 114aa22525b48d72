"""tests/_stale.py against a numpy stand-in of the arena and of a handle, with planted defects (host only).

The stand-in's arena follows csrc/api_core.hip: one buffer per slot, grown on demand with 1/8 head-room (4096 bytes at least),
fresh memory is zero, nothing is cleared on reuse.  Its verb counts bytes into a histogram with a cursor word behind it, all carved
from slot A, the way the counting kernels carve theirs; its handle keeps an offsets buffer that only grows.  Every planted defect
gives right answers on fresh memory and after a fill with zeros, as on the device; the helper has to name each of them.  No
defect is planted in the real kernels anywhere.

The last tests tie DESIGN.md's audit tables to tests/test_gpu_stale_state.py: every row names a case there or a reason."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _stale as ST

ROOT = Path(__file__).resolve().parents[1]


class FakeArena:
    def __init__(self):
        self.bufs, self.n_acquired = {}, 0

    def scratch(self, slot, nbytes):
        """the WHOLE allocation, as a kernel sees it: nothing stops a read or write beyond nbytes"""
        self.n_acquired += 1
        b = self.bufs.get(slot)
        if b is None or len(b) < nbytes:
            b = self.bufs[slot] = np.zeros(4096 if nbytes < 4096 else nbytes + nbytes // 8, np.uint8)
        return b

    def release(self):
        self.bufs = {}

    def fill(self, byte):
        for b in self.bufs.values():
            b[:] = byte
        return len(self.bufs), sum(len(b) for b in self.bufs.values())

    def acquired(self):
        return self.n_acquired


def histogram_verb(A, data, defect=None):
    """{hist: counts of the byte values 0 .. nb-1 of data, n: (how many were counted, the sum of the counters)}: one cursor word
    and nb uint32 counters behind it, from slot A.  defect: 'counter' (the cursor is not cleared), 'short' (the clear ends one
    word early: the last counter), 'headroom' (the counters are summed up to the next multiple of 64 instead of the nb carved)"""
    nb = int(data.max()) + 1
    words = A.scratch("A", (nb + 1) * 4).view(np.uint32)
    if defect == "counter":
        words[1:nb + 1] = 0
    elif defect == "short":
        words[:nb] = 0
    else:
        words[:nb + 1] = 0
    np.add.at(words, data + 1, 1)                            # read-modify-write, like atomicAdd
    words[0] += len(data)
    upto = -(-nb // 64) * 64 if defect == "headroom" else nb
    return {"hist": words[1:nb + 1].copy(), "n": np.array([words[0], words[1:upto + 1].sum()], np.int64)}


def reference(data):
    nb = int(data.max()) + 1
    return {"hist": np.bincount(data, minlength=nb).astype(np.uint32), "n": np.array([len(data), len(data)], np.int64)}


def data_pair():
    """(small, big): 37 counters, and 2000 counters so that slot A grows past its 4096-byte minimum and the small case's tail is stale"""
    rng = np.random.default_rng(0)
    small = rng.integers(0, 37, 500)
    small[0] = 36                                            # the last counter is used
    return small, np.concatenate([rng.integers(0, 200, 50_000), np.arange(2000)])


def run_states(defect):
    A = FakeArena()
    small, big = data_pair()
    return ST.states(f"histogram ({defect})", lambda: histogram_verb(A, small, defect), lambda: histogram_verb(A, big), reference(small),
                     arena_=A)


def test_clean_stand_in_passes():
    got = run_states(None)
    assert ST.first_difference(got, reference(data_pair()[0])) is None


@pytest.mark.parametrize("defect,array", [("counter", "n"), ("short", "hist"), ("headroom", "n")])
def test_planted_arena_defect_is_named(defect, array):
    """each defect is invisible cold and after zeros, and is reported for the first non-zero fill with the array it spoils"""
    with pytest.raises(ST.StaleError) as e:
        run_states(defect)
    assert (e.value.kind, e.value.state, e.value.array) == ("stale", "0x5A", array), str(e.value)
    assert "had not written" in str(e.value)


def test_a_case_without_scratch_is_refused():
    A = FakeArena()
    small, big = data_pair()
    with pytest.raises(ST.StaleError) as e:
        ST.states("no scratch", lambda: reference(small), lambda: histogram_verb(A, big), reference(small), arena_=A)
    assert e.value.kind == "unused" and e.value.state == "cold"


def test_a_primer_without_scratch_is_refused():
    A = FakeArena()
    small, _ = data_pair()

    def case():
        out = histogram_verb(A, small)
        A.release()                                          # nothing stays cached: the fill has nothing to set
        return out
    with pytest.raises(ST.StaleError) as e:
        ST.states("no buffer", case, lambda: None, reference(small), arena_=A)
    assert e.value.kind == "unfilled" and e.value.state == "0x00"


def test_a_wrong_case_is_reported_cold():
    A = FakeArena()
    small, big = data_pair()
    want = reference(small)
    want["hist"] = want["hist"] + np.uint32(1)
    with pytest.raises(ST.StaleError) as e:
        ST.states("wrong", lambda: histogram_verb(A, small), lambda: histogram_verb(A, big), want, arena_=A)
    assert (e.value.kind, e.value.array) == ("cold", "hist")


def test_state_outside_the_arena_is_reported_warm():
    A = FakeArena()
    small, big = data_pair()
    seen = []

    def case():
        out = histogram_verb(A, small)
        out["n"] = out["n"] + len(seen)                      # remembers that the primer ran
        return out
    with pytest.raises(ST.StaleError) as e:
        ST.states("remembers", case, lambda: (seen.append(1), histogram_verb(A, big)), reference(small), arena_=A)
    assert (e.value.kind, e.value.state) == ("warm", "0x00")


def test_results_are_compared_bit_for_bit():
    assert ST.first_difference(np.array([0.0]), np.array([-0.0]))[0] == "0"
    assert ST.first_difference(np.array([np.nan]), np.array([np.nan])) is None
    assert ST.first_difference(np.zeros(3, np.int32), np.zeros(3, np.int64))[0] == "0"
    assert ST.first_difference({"a": np.zeros(3)}, {"b": np.zeros(3)})[0] == "<names>"
    assert "element 2 of 3" in ST.first_difference((np.arange(3),), (np.array([0, 1, 5]),))[1]


# ---- the handle ---------------------------------------------------------------------------------------------------------------------
class FakeScan:
    """offsets of a run's hit counts in a buffer that only grows, like kmap_scan's s->offs.  defect 'shrink': the summary sums the
    offsets buffer up to the largest size it has had, not up to this run's"""

    def __init__(self, defect=None):
        self.offs, self.defect, self.n, self.closed = np.zeros(0, np.int64), defect, 0, False

    def run(self, hits):
        if len(self.offs) < len(hits) + 1:
            self.offs = np.zeros(len(hits) + 1, np.int64)    # fresh memory: zero
        self.n = len(hits)
        self.offs[1:self.n + 1] = np.cumsum(hits)
        upto = len(self.offs) if self.defect == "shrink" else self.n + 1
        return {"offs": self.offs[:self.n + 1].copy(), "max": np.array([self.offs[:upto].max()], np.int64)}

    def close(self):
        self.closed = True


def scan_reference(hits):
    offs = np.concatenate([[0], np.cumsum(hits)]).astype(np.int64)
    return {"offs": offs, "max": np.array([offs.max()], np.int64)}


def test_clean_handle_passes_and_is_closed():
    rng = np.random.default_rng(1)
    big, small = rng.integers(0, 9, 30_000), rng.integers(0, 9, 7)
    made = []

    def factory():
        made.append(FakeScan())
        return made[-1]
    ST.reused("scan", factory, lambda h: h.run(big), lambda h: h.run(small), scan_reference(small))
    assert len(made) == 2 and all(h.closed for h in made)


def test_planted_handle_defect_is_named():
    rng = np.random.default_rng(1)
    big, small = rng.integers(0, 9, 30_000), rng.integers(0, 9, 7)
    with pytest.raises(ST.StaleError) as e:
        ST.reused("scan", lambda: FakeScan("shrink"), lambda h: h.run(big), lambda h: h.run(small), scan_reference(small))
    assert (e.value.kind, e.value.state, e.value.array) == ("handle", "reused", "max"), str(e.value)
    assert "survived the larger run" in str(e.value)


def test_a_wrong_fresh_handle_is_reported_first():
    small = np.arange(7)
    want = scan_reference(small)
    want["max"] = want["max"] + 1
    with pytest.raises(ST.StaleError) as e:
        ST.reused("scan", FakeScan, lambda h: h.run(np.arange(100)), lambda h: h.run(small), want)
    assert e.value.kind == "fresh"


# ---- the audit tables -----------------------------------------------------------------------------------------------------------------
def gpu_file_tests():
    return set(re.findall(r"^def (test_\w+)\(", (ROOT / "tests" / "test_gpu_stale_state.py").read_text(), flags=re.M))


def test_audit_rows_parse():
    text = ("# x\n## 9. Stale scratch and handle state\nwords\n\n| entry | slots | case |\n|---|---|---|\n| `kmap_a_dev`, `kmap_b` | A | `test_a`, `test_b[x]` |\n"
            "| `kmap_c` | - | none: takes a second GPU |\n\n| handle | survives | case |\n|--|--|--|\n| `kmap_scan` | offs | `test_h` |\n## 10. next\n| entry | case |\n| `kmap_z` | `test_z` |\n")
    rows = ST.audit_rows(text)
    assert [r[0] for r in rows] == ["kmap_a_dev, kmap_b", "kmap_c", "kmap_scan"]
    assert ST.row_case(rows[0][1]) == (["test_a", "test_b"], None)
    assert ST.row_case(rows[1][1]) == ([], "takes a second GPU")


def test_every_audit_row_has_a_case_or_a_reason():
    """every row of DESIGN.md's audit tables names a test of tests/test_gpu_stale_state.py or says `none: <reason>`; a new verb that
    takes a slot gets a row, and the row fails here until it has either"""
    rows = ST.audit_rows((ROOT / "DESIGN.md").read_text())
    assert len(rows) >= 39, f"only {len(rows)} rows found: the tables had 35 entry rows and 4 handle rows when they were written"
    have = gpu_file_tests()
    bad = []
    for entry, cell in rows:
        tests, reason = ST.row_case(cell)
        if reason is not None:                               # it may point to the cases that run the shared code
            if len(reason) <= 10:
                bad.append(f"{entry}: `none:` needs a reason ({cell!r})")
            bad += [f"{entry}: the reason names {t}, which is not in tests/test_gpu_stale_state.py" for t in tests if t not in have]
        elif not tests:
            bad.append(f"{entry}: neither a case nor `none: reason`")
        else:
            bad += [f"{entry}: {t} is not in tests/test_gpu_stale_state.py" for t in tests if t not in have]
    assert not bad, "\n".join(bad)


HANDLES = ("kmap_scan", "kmap_counts", "kmap_enrich")


def test_every_audited_entry_is_declared():
    """the kmap_* names of the rows' first cells are prototypes of include/kmap_hip.h and no entry has two rows"""
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    declared = set(re.findall(r"\b(kmap_\w+)\s*\(", header))
    named = [n for entry, _ in ST.audit_rows((ROOT / "DESIGN.md").read_text()) for n in re.findall(r"\bkmap_\w+", entry)]
    unknown = sorted(n for n in named if n not in declared and n not in HANDLES)
    assert not unknown, f"rows name entries that include/kmap_hip.h does not declare: {unknown}"
    twice = sorted({n for n in named if named.count(n) > 1} - set(HANDLES))
    assert not twice, f"entries with more than one row: {twice}"


def test_rows_name_declared_cases_of_their_entries():
    """a row's tests are held to the @covers lists of tests/test_gpu_stale_state.py: every entry of the row is covered by one of
    the tests the row names, and every test the row names covers an entry of the row -- a row cannot point at a test that never
    calls its entry"""
    import tests.test_gpu_stale_state  # noqa: F401  (registers the cases)
    bad = []
    for entry, cell in ST.audit_rows((ROOT / "DESIGN.md").read_text()):
        tests, reason = ST.row_case(cell)
        names = [n for n in re.findall(r"\bkmap_\w+", entry) if n not in HANDLES]
        if reason is not None or not names:
            continue
        bad += [f"{n}: none of {tests} declares it with @covers" for n in names if not set(ST.REGISTERED.get(n, [])) & set(tests)]
        bad += [f"{t}: named by the row of {names} and covers none of them" for t in tests
                if not any(t in ST.REGISTERED.get(n, []) for n in names)]
    assert not bad, "\n".join(bad)


# source files whose exported entries take no scratch although the file calls kmap_scratch or a helper that does
NO_ROW = {"api_core.hip": "the arena itself"}
TAKERS = r"\bkmap_scratch\(|\bexclusive_scan_(u32|total)\b|\bradix_sort\(|\bpwm_pass_a\(|\bpwm_key_batches<"


def test_every_source_file_that_takes_scratch_has_a_row():
    """a source file that calls kmap_scratch, the shared scan, the radix sort or a weight-matrix helper, and defines entries that
    include/kmap_hip.h declares, has at least one of them in the audit table (or a reason in NO_ROW): a new verb in a new file
    fails here until it has a row.  A new entry in a file that already has a row is not caught by this test."""
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    declared = set(re.findall(r"\b(kmap_\w+)\s*\(", header))
    named = {n for entry, _ in ST.audit_rows((ROOT / "DESIGN.md").read_text()) for n in re.findall(r"\bkmap_\w+", entry)}
    missing = []
    for src in sorted((ROOT / "kmap_amd" / "csrc").glob("*.hip")):
        text = src.read_text()
        if not re.search(TAKERS, text) or src.name in NO_ROW:
            continue
        mine = set(re.findall(r"^(?:int|int64_t)\s+(kmap_\w+)\s*\(", text, flags=re.M)) & declared
        if mine and not mine & named:
            missing.append(f"{src.name}: none of {sorted(mine)} has a row")
    assert not missing, "\n".join(missing)
    assert all(len(r) > 10 for r in NO_ROW.values())


def test_an_undersized_primer_is_refused():
    A = FakeArena()
    small, big = data_pair()
    with pytest.raises(ST.StaleError) as e:
        ST.states("undersized", lambda: histogram_verb(A, big), lambda: histogram_verb(A, big[:100]), reference(big), arena_=A)
    assert e.value.kind == "undersized" and e.value.state == "0x00"


def test_a_check_takes_the_place_of_the_reference():
    """for entries whose own test holds floats to a bound: the check sees the cold result, the warm ones must equal it bit for bit"""
    A = FakeArena()
    small, big = data_pair()
    seen = []
    ST.states("check", lambda: histogram_verb(A, small), lambda: histogram_verb(A, big), check=seen.append, arena_=A)
    assert len(seen) == 1 and ST.first_difference(seen[0], reference(small)) is None
    with pytest.raises(ST.StaleError) as e:
        ST.states("check", lambda: histogram_verb(A, small, "counter"), lambda: histogram_verb(A, big), check=seen.append, arena_=A)
    assert e.value.kind == "stale"
