"""Host side of extract_motif_locations / check_motif_co_occurence (no GPU): the CLI options against the reference's, the native
occurrence-CSV parser against Occurrence.from_file, the native BED parser (3 / 6 columns, the integer-versus-string chrom rule) and
the native BED formatter against pandas' to_csv (csrc/host_bed.hip)."""
import json
import random
from pathlib import Path

import numpy as np
import pytest

GOLD = Path(__file__).resolve().parent / "golden"
LGOLD = GOLD / "locations"
ENVS = [{"KMAP_IO_THREADS": "1"}, {"KMAP_IO_THREADS": "4", "KMAP_TEXT_MIN_CHUNK": "1"},
        {"KMAP_IO_THREADS": "7", "KMAP_TEXT_MIN_CHUNK": "97"}, {}]


def _setenv(monkeypatch, env):
    for k in ("KMAP_IO_THREADS", "KMAP_TEXT_MIN_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("verb", ["extract_motif_locations", "check_motif_co_occurence"])
def test_cli_options_match_the_reference(verb):
    """option names, defaults, required flags and types of the two verbs == the reference's click commands; --help lists them"""
    from click.testing import CliRunner
    from kmap_amd.cli import cli
    want = json.loads((LGOLD / "cli_options.json").read_text())[verb]
    cmd = cli.commands[verb]
    got = [{"name": p.name, "opts": list(p.opts), "default": p.default if isinstance(p.default, (str, int, bool)) else None,
            "required": p.required, "type": p.type.name} for p in cmd.params]
    assert got == want
    r = CliRunner().invoke(cli, [verb, "--help"])
    assert r.exit_code == 0
    for p in want:
        assert p["opts"][0] in r.output


def _same_occ(a, b):
    assert a.n_conseq == b.n_conseq
    np.testing.assert_array_equal(a.seq_ind, b.seq_ind)
    np.testing.assert_array_equal(a.seq_len, b.seq_len)
    for c in range(a.n_conseq):
        np.testing.assert_array_equal(a.hits[c], b.hits[c])
        np.testing.assert_array_equal(a.pos[c], b.pos[c])


@pytest.mark.parametrize("env", ENVS)
def test_occurrence_parser_golden(monkeypatch, env):
    from kmap_amd.locations import read_occurrence
    from kmap_amd.reports import Occurrence
    _setenv(monkeypatch, env)
    files = [GOLD / "scan_testfa" / "final.motif_occurence.csv", GOLD / "occ20" / "occ20.motif_occurence.csv",
             GOLD / "report_testfa" / "user_motif_occurence.csv", LGOLD / "synth.motif_occurence.csv",
             LGOLD / "co_readme" / "user_motif_occurence.csv"]
    for f in files:
        _same_occ(read_occurrence(f), Occurrence.from_file(f))


def _random_occ_text(rng, n_rows, n_cols):
    sep = rng.choice(["\n", "\r\n"])
    lines = [";".join(["seq_ind"] + [f"motif_{c}_X" for c in range(n_cols)] + ["seq_len"])]
    for r in range(n_rows):
        cells = []
        for _ in range(n_cols):
            k = rng.choice([0, 0, 1, 2, 3, 7])
            vals = [str(rng.randint(0, 3000)) for _ in range(k)]          # unsorted, duplicates possible
            cell = ",".join(vals)
            if rng.random() < 0.1:
                cell = " " + cell.replace(",", " , ") + " "
            cells.append(cell)
        seq_len = str(rng.randint(1, 5000)) + (".0" if rng.random() < 0.1 else "")
        lines.append(";".join([str(rng.randint(0, 10 ** 7))] + cells + [seq_len]))
    return sep.join(lines) + (sep if rng.random() < 0.8 else "")


@pytest.mark.parametrize("env", ENVS[:3])
def test_occurrence_parser_random(tmp_path, monkeypatch, env):
    """random files (empty, unsorted, padded and CRLF cells, with and without a final newline) == Occurrence.from_file"""
    from kmap_amd.locations import read_occurrence
    from kmap_amd.reports import Occurrence
    _setenv(monkeypatch, env)
    rng = random.Random(7)
    for it in range(25):
        p = tmp_path / f"o{it}.csv"
        p.write_bytes(_random_occ_text(rng, rng.choice([0, 1, 5, 200, 3000]), rng.choice([0, 1, 3])).encode())
        _same_occ(read_occurrence(p), Occurrence.from_file(p))


def test_occurrence_parser_errors(tmp_path):
    from kmap_amd.locations import read_occurrence
    bad = {"letters": "seq_ind;m;seq_len\n1;3,x;10\n", "fields": "seq_ind;m;seq_len\n1;3\n", "more": "seq_ind;m;seq_len\n1;3;4;5\n",
           "trailing_comma": "seq_ind;m;seq_len\n1;3,;10\n", "empty": ""}
    for name, text in bad.items():
        p = tmp_path / f"{name}.csv"
        p.write_text(text)
        with pytest.raises(ValueError):
            read_occurrence(p)
    with pytest.raises(OSError):
        read_occurrence(tmp_path / "missing.csv")


def test_bed_parser_widths_and_chrom_rule(tmp_path):
    from kmap_amd.locations import BedFile
    p = tmp_path / "a.bed"
    p.write_text("chr2\t100\t200\tx\t0\t+\nchr10\t5\t9\tx\t0\t-\r\n\nchrX\t7\t9\ty\t1\t.\nchr1\t3000000000\t3000000100\tz\t0\t+\n")
    b = BedFile(p)
    assert (b.n_rows, b.n_cols, b.int_chrom) == (4, 6, False)
    assert b.chroms == ["chr1", "chr10", "chr2", "chrX"]                   # code-point order
    np.testing.assert_array_equal(b.start, [100, 5, 7, 3_000_000_000])
    np.testing.assert_array_equal(b.chrom_rank, [2, 1, 3, 0])
    p.write_text("2\t100\t200\n010\t5\t9\n10\t7\t9\n-1\t0\t1\n")
    b = BedFile(p)
    assert (b.n_rows, b.n_cols, b.int_chrom) == (4, 3, True)
    assert b.chroms == ["-1", "2", "10"]                                   # by value; "010" is the integer 10
    np.testing.assert_array_equal(b.chrom_rank, [1, 2, 2, 0])
    p.write_text("2\t100\t200\n1x\t5\t9\n")
    b = BedFile(p)
    assert not b.int_chrom and b.chroms == ["1x", "2"]
    for text in ("2\t100\t200\t3\n", "c\t1\n", "c\t1\t2\t3\t4\t5\t6\n", "c\t1\t2\nc\t1\t2\t3\t4\t5\n", "c\tx\t2\n"):
        p.write_text(text)
        with pytest.raises(ValueError):
            BedFile(p)


def _pandas_expected(rows):
    pd = pytest.importorskip("pandas")
    import io
    buf = io.StringIO()
    pd.DataFrame(rows, columns=["chrom", "start", "end", "name", "score", "strand"]).to_csv(buf, sep="\t", header=True, index=False)
    return buf.getvalue().encode()


@pytest.mark.parametrize("env", ENVS[:3])
def test_bed_formatter_equals_pandas(tmp_path, monkeypatch, env):
    """kmap_bed_write_locations == pandas DataFrame.to_csv(sep='\\t', index=False) of the same rows (string and integer chroms,
    empty output, coordinates above 2^31)"""
    from kmap_amd.locations import BedFile
    _setenv(monkeypatch, env)
    rng = np.random.default_rng(3)
    for int_chrom in (False, True):
        names = ["1", "2", "10", "22"] if int_chrom else ["chr1", "chrX", "chr10", "scaffold_7"]
        n_bed = 5000
        ch = rng.choice(names, n_bed)
        st = rng.integers(0, 2 ** 33, n_bed)
        sd = rng.choice(["+", "-", "."], n_bed)
        p = tmp_path / "b.bed"
        p.write_text("".join(f"{c}\t{s}\t{s + 10}\tn\t0\t{d}\n" for c, s, d in zip(ch, st, sd)))
        b = BedFile(p)
        for n in (0, 1, 70_000):
            row = rng.integers(0, n_bed, n)
            start = st[row] + rng.integers(0, 300, n)
            end = start + rng.integers(0, 40, n)
            out = tmp_path / "o.bed"
            nb = b.write_locations(out, 3, row, start, end)
            rows = [[int(ch[r]) if int_chrom else ch[r], int(s), int(e), f"motif_3_{r}", 0, sd[r]] for r, s, e in zip(row, start, end)]
            data = out.read_bytes()
            assert data == _pandas_expected(rows) and nb == len(data)
        b.close()
