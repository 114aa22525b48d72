"""CPU sanitizer runs of kmap_amd/csrc/host_bed.hip (threaded occurrence-CSV and BED parsers, threaded BED writer): tests/host_san_bed
compiles it host-only with -fsanitize=address,undefined and with -fsanitize=thread into a small driver; any sanitizer report fails
the run.  The parsed arrays are compared with Occurrence.from_file, the written BED with a Python formatting of the same rows, under
several KMAP_IO_THREADS / KMAP_TEXT_MIN_CHUNK settings (ranges as small as one line)."""
import os
import random
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SAN = HERE / "host_san_bed"
ENVS = [{"KMAP_IO_THREADS": "1"}, {"KMAP_IO_THREADS": "8", "KMAP_TEXT_MIN_CHUNK": "1"}, {"KMAP_IO_THREADS": "3", "KMAP_TEXT_MIN_CHUNK": "4096"}]


@pytest.fixture(scope="module")
def drivers():
    if shutil.which("/opt/rocm/bin/hipcc") is None:
        pytest.skip("hipcc not available")
    r = subprocess.run(["make", "-s", "-C", str(SAN)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return {"asan": SAN / "build" / "driver_asan", "tsan": SAN / "build" / "driver_tsan"}


def _run(exe, *args, env=None, ok=True):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
             TSAN_OPTIONS="halt_on_error=1")
    e.update(env or {})
    r = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=600, env=e)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert (r.returncode == 0) == ok, (r.returncode, r.stderr[-3000:])
    return r.stdout


def _occ_text(rng, n_rows, n_cols):
    sep = rng.choice(["\n", "\r\n"])
    lines = [";".join(["seq_ind"] + [f"m{c}" for c in range(n_cols)] + ["seq_len"])]
    for _ in range(n_rows):
        cells = [",".join(str(rng.randint(0, 9999)) for _ in range(rng.choice([0, 0, 1, 3, 9]))) for _ in range(n_cols)]
        lines.append(";".join([str(rng.randint(0, 10 ** 6))] + cells + [str(rng.randint(1, 999))]))
        if rng.random() < 0.02:
            lines.append("")
    return sep.join(lines) + (sep if rng.random() < 0.7 else "")


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_occurrence_parser_sanitized(drivers, tmp_path, san):
    from kmap_amd.reports import Occurrence
    rng = random.Random(11 if san == "asan" else 12)
    for it in range(12):
        n_rows, n_cols = rng.choice([0, 1, 7, 400, 20_000]), rng.choice([0, 1, 2, 5])
        text = _occ_text(rng, n_rows, n_cols)
        p = tmp_path / f"o{it}.csv"
        p.write_bytes(text.encode())
        want = Occurrence.from_file(p) if "\n\n" not in text and "\r\n\r\n" not in text else None
        _run(drivers[san], "occ", p, tmp_path / "o.bin", env=ENVS[it % 3])
        blob = np.fromfile(tmp_path / "o.bin", np.int64)
        n, nc = int(blob[0]), int(blob[1])
        n_pos, at = blob[2:2 + nc], 2 + nc
        assert (n, nc) == (n_rows, n_cols)
        seq_ind, seq_len = blob[at:at + n], blob[at + n:at + 2 * n]
        at += 2 * n
        if want is None:
            continue
        np.testing.assert_array_equal(seq_ind, want.seq_ind)
        np.testing.assert_array_equal(seq_len, want.seq_len)
        for c in range(nc):
            np.testing.assert_array_equal(blob[at:at + n], want.hits[c])
            np.testing.assert_array_equal(blob[at + n:at + n + n_pos[c]], want.pos[c])
            at += n + int(n_pos[c])
    (tmp_path / "bad.csv").write_text("seq_ind;m;seq_len\n" + "1;2,3;4\n" * 5000 + "1;2,x;4\n" + "1;2;4\n" * 5000)
    _run(drivers[san], "occ", tmp_path / "bad.csv", tmp_path / "o.bin", env=ENVS[1], ok=False)


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_bed_parser_and_writer_sanitized(drivers, tmp_path, san):
    rng = np.random.default_rng(4 if san == "asan" else 5)
    for it, (cols, names) in enumerate([(6, ["chr1", "chr2", "chr10", "chrX"]), (3, ["1", "2", "10", "007"]), (6, ["only"])]):
        n = 30_000
        ch, st = rng.choice(names, n), rng.integers(0, 2 ** 35, n)
        sd = rng.choice(["+", "-", "."], n)
        rows = [f"{c}\t{s}\t{s + 9}" + (f"\tn\t0\t{d}" if cols == 6 else "") for c, s, d in zip(ch, st, sd)]
        p = tmp_path / f"b{it}.bed"
        p.write_text("\r\n".join(rows) + "\n")
        out = _run(drivers[san], "bed", p, tmp_path / "o.bed", env=ENVS[it % 3])
        ints = all(x.isdigit() for x in names)
        assert out.split() == [str(n), str(cols), str(len({int(x) for x in names} if ints else set(names))), str(int(ints))]
        want = "chrom\tstart\tend\tname\tscore\tstrand\n" + "".join(
            f"{int(c) if ints else c}\t{s}\t{s + 5}\tmotif_1_{i}\t0\t{d if cols == 6 else '.'}\n" for i, (c, s, d) in enumerate(zip(ch, st, sd)))
        assert (tmp_path / "o.bed").read_text() == want
    (tmp_path / "w4.bed").write_text("c\t1\t2\t3\n")
    _run(drivers[san], "bed", tmp_path / "w4.bed", tmp_path / "o.bed", ok=False)
