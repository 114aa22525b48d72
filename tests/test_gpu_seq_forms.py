"""Every form of the SEQ force kernel (csrc/embed_seq.hip), per row, against the host model of the reference arithmetic
(tests/_seq_model.py, tied to the oracle by tests/test_seq_model_host.py): one force evaluation per case, the gradient of the
checked rows bit for bit, the entries of other sessions' rows untouched, the loss partial against the model's float64 sum.

Every case ASSERTS the form it claims to pin through EmbedSession.seq_geometry(): shapes are written in terms of the CU count
(round = 64 rows x CUs: one quad wave on every SIMD), and a device that splits the rows differently fails here instead of
silently testing another form.  Forms and where they run:
  classic, fewer rows than a round   wide form with 64 / 32 / 16 lanes per row, quad above 12 000 rows
  quad at small N                    KMAP_SEQ_TAIL=0 (read once per process: ONE child process runs all these cases)
  behind a full round                remainders that select 64, 32, 16, 8, 8, 16 lanes and the quad form
  pair form                          three rounds + 848 rows
  producer / adder                   R = 1 .. 64 rows per block in both geometries, every (M, EA) producer layout
Rows checked: all where n <= 4096, else at most 384 (the borders of every region, wave and block, rows whose diagonal is the
first or last column of a batch or chunk, rows n - 1 and n - 2, a fixed random rest)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import _seq_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = np.float32(-7.25)                 # what the gradient buffer holds before the evaluation
MAX_ROWS = 384
LOSS_PAIRS = 5 * 10 ** 7                 # the loss is compared where nrows * n stays below this
# loss partial against the model, relative.  Starting point: the project's own 3e-6 (test_seq_forces_bit_exact_vs_oracle).  Largest
# deviation observed over the cases of this file: 1.4e-7 (wide 64, n = 8; every form lies at 2.6e-8 .. 1.4e-7, CHANGELOG), below a
# quarter of 3e-6, hence 4 x the observed maximum.  The kernel's v_log_f32 is an approximation whose error is not derived here; the
# 4 is for inputs not yet seen.
LOSS_RTOL = 5.6e-7


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _case(cid, n, row0=0, nrows=None, src="lut", coords="clustered", rowmap=False, pitch=None, form="classic", **expect):
    nrows = n - row0 if nrows is None else nrows
    if pitch is None:
        pitch = (n + 127) & ~127 if src == "lut" else n
    return dict(id=cid, n=int(n), row0=int(row0), nrows=int(nrows), src=src, coords=coords, rowmap=bool(rowmap), pitch=int(pitch),
                form=form, expect={k: int(v) for k, v in expect.items()})


def _wide(g, nrows):
    return dict(adder=0, main_rows=0 if g else nrows, pair_rows=0, tail_g=g)


def classic_cases():
    """fewer rows than one round: the wide form by row count (64 lanes to 1500 rows, 32 to 2500, 16 to 12 000), quad above"""
    out = []
    g_of = lambda r: 64 if r <= 1500 else 32 if r <= 2500 else 16 if r <= 12000 else 0
    for n in (1, 2, 7, 8, 9, 300, 701, 2049, 2052, 2560, 2561, 2688, 3001):
        out.append(_case(f"lut-n{n}", n, **_wide(g_of(n), n)))
        out.append(_case(f"lut-map-n{n}", n, rowmap=True, **_wide(g_of(n), n)))
        out.append(_case(f"f32-n{n}", n, src="f32", **_wide(g_of(n), n)))                                 # pitch n
    for n in (9, 701, 2052, 2561, 3001):
        out.append(_case(f"f32-padded-n{n}", n, src="f32", pitch=(n + 63) & ~63, **_wide(g_of(n), n)))    # pitch % 8 == 0
    for n in (701, 2052, 2561):
        out.append(_case(f"lut-pitch{n + 5}-n{n}", n, pitch=n + 5, **_wide(g_of(n), n)))                  # sums pitch % 8 != 0
    for n in (701, 2052, 2561):
        for scale in (1.0, 1e3):
            out.append(_case(f"lut-n{n}-scale{scale:g}", n, coords=scale, **_wide(g_of(n), n)))
    out.append(_case("f32-n2561-scale1000", 2561, src="f32", coords=1e3, **_wide(16, 2561)))
    out.append(_case("lut-map-n12004-quad", 12004, rowmap=True, **_wide(0, 12004)))
    for n, row0, nrows in ((1000, 100, 650), (4136, 7, 31), (3001, 2000, 1001), (701, 350, 1), (2052, 0, 2049)):
        out.append(_case(f"lut-shard-n{n}-{row0}+{nrows}", n, row0, nrows, **_wide(g_of(nrows), nrows)))
        out.append(_case(f"f32-shard-n{n}-{row0}+{nrows}", n, row0, nrows, src="f32", **_wide(g_of(nrows), nrows)))
    return out


def quad_cases():
    """KMAP_SEQ_TAIL=0: the quad form at small N -- scalar buffer loads with their three column regions and the ja / jb / jn
    clamps (LUT, n % 4 == 0, pitch % 8 == 0), 16-byte vector loads (f32, n % 4 == 0, pitch % 8 == 0), generic loads"""
    out = []
    q = lambda nrows: dict(adder=0, main_rows=nrows, pair_rows=0, tail_g=0)
    for n in (300, 1003, 1024, 1088):
        out.append(_case(f"quad-lut-n{n}", n, **q(n)))
        out.append(_case(f"quad-lut-map-n{n}", n, rowmap=True, **q(n)))
        out.append(_case(f"quad-f32-n{n}", n, src="f32", pitch=(n + 7) & ~7, **q(n)))
    out.append(_case("quad-f32-n1024-pitch1027", 1024, src="f32", pitch=1027, **q(1024)))
    out.append(_case("quad-lut-n1024-pitch1027", 1024, pitch=1027, **q(1024)))
    for n, row0 in ((1088, 1000), (1003, 900), (1024, 1023), (300, 17)):
        out.append(_case(f"quad-lut-shard-n{n}-from{row0}", n, row0, **q(n - row0)))
        out.append(_case(f"quad-f32-shard-n{n}-from{row0}", n, row0, src="f32", pitch=(n + 7) & ~7, **q(n - row0)))
    for scale in (1.0, 1e3):
        out.append(_case(f"quad-lut-n1024-scale{scale:g}", 1024, coords=scale, **q(1024)))
    return out


def round_cases(cus):
    """one full round of quad waves + a remainder (row map: a few hundred stored rows).  Costs per round of the selection rule
    (kmap_embed_seq_split): quad 9.4 per 16 rows x SIMDs, g lanes (30 / g + 1.2) per (64 / g) rows x SIMDs"""
    simds, rnd = 4 * cus, 64 * cus
    out = []
    for rem, g in ((77, 64), (simds + 5, 32), (4 * simds, 16), (4 * simds + 1, 8), (8 * simds, 8), (8 * simds + 1, 16), (12 * simds + 1, 0)):
        nrows = rnd + rem
        exp = dict(adder=0, main_rows=rnd if g else nrows, pair_rows=0, tail_g=g)
        out.append(_case(f"round+{rem}-g{g}", (nrows + 3) & ~3, 0, nrows, rowmap=True, **exp))
        if rem in (simds + 5, 4 * simds + 1):
            assert nrows % 4
            out.append(_case(f"round+{rem}-g{g}-generic", nrows, 0, nrows, rowmap=True, **exp))
    nrows = rnd + 4 * simds + 1
    for scale in (1.0, 1e3):
        out.append(_case(f"round+{4 * simds + 1}-g8-scale{scale:g}", (nrows + 3) & ~3, 0, nrows, rowmap=True, coords=scale,
                         adder=0, main_rows=rnd, pair_rows=0, tail_g=8))
    return out


def pair_cases(cus):
    rnd = 64 * cus
    nrows = 3 * rnd + 848
    exp = dict(adder=0, main_rows=3 * rnd, pair_rows=2 * rnd, tail_g=64)
    out = [_case("pair-n=nrows", (nrows + 3) & ~3, 0, nrows, rowmap=True, **exp),
           _case("pair-n=nrows+1-generic", ((nrows + 3) & ~3) + 1, 0, nrows, rowmap=True, **exp),
           _case("pair-shard-from5000", nrows + 10000, 5000, nrows, rowmap=True, **exp)]
    for scale in (1.0, 1e3):
        out.append(_case(f"pair-scale{scale:g}", (nrows + 3) & ~3, 0, nrows, rowmap=True, coords=scale, **exp))
    return out


# producer layout (M, EA) by producer steps per chunk (rows per step: 2 at RP = 32, 4 at RP = 64)
ADDER_R = {1: (32, 2, 0), 3: (32, 2, 0), 14: (32, 2, 1), 16: (32, 2, 2), 18: (32, 3, 0), 20: (32, 3, 1), 22: (32, 3, 2), 24: (32, 4, 0),
           25: (32, 4, 1), 32: (32, 4, 1), 33: (64, 3, 0), 49: (64, 4, 1), 64: (64, 4, 1)}


def adder_cases(cus):
    """KMAP_SEQ_FORM=adder: one block per CU, R = ceil(nrows / CUs) rows per block, 32 row slots up to 32 x CUs rows, else 64"""
    out = []

    def rows_for(R, last):        # a row count that gives R rows per block and `last` rows in the last block (0: full)
        for nrows in range((R - 1) * cus + 1, R * cus + 1):
            if nrows % R == last % R:
                return nrows
        raise AssertionError((R, last))

    def exp(R):
        rp, m, ea = ADDER_R[R]
        return dict(adder=1, R=R, RP=rp, M=m, EA=ea)

    out.append(_case("adder-R1-n-below-a-chunk", min(200, cus), form="adder", **exp(1)))
    nr = rows_for(3, 1)                                              # last block: one row, fewer than a producer step
    out.append(_case("adder-R3-end-shard-n-multiple-of-chunk", (nr + 255) & ~255, ((nr + 255) & ~255) - nr, nr, form="adder", **exp(3)))
    out.append(_case("adder-R3-f32-runs-classic", 1024, 0, nr, src="f32", form="adder", adder=0, R=3, RP=32, M=0, EA=0))
    for R, last, odd in ((14, 1, True), (16, 0, False), (18, 5, False), (20, 3, True), (22, 1, False), (24, 23, True), (25, 2, False),
                         (32, 0, False), (33, 1, True), (49, 3, False), (64, 0, False)):
        nr = R * cus if R in (32, 64) else rows_for(R, last)          # full blocks everywhere, n a multiple of the chunk
        n = nr + 1 if odd and (nr + 1) % 8 else nr + 3 if odd else (nr + 7) & ~7
        out.append(_case(f"adder-R{R}-last{last}-n{n}", n, 0, nr, rowmap=True, form="adder", **exp(R)))
    nr = rows_for(14, 1)
    for scale in (1.0, 1e3):
        out.append(_case(f"adder-R14-scale{scale:g}", (nr + 7) & ~7, 0, nr, rowmap=True, coords=scale, form="adder", **exp(14)))
    out.append(_case("adder-R18-end-shard-map", rows_for(18, 5) + 3000, 3000, rows_for(18, 5), rowmap=True, form="adder", **exp(18)))
    # the natural default: no switch, n >= 3072, fewer than 7 / 4 rounds of rows
    R = (3072 + cus - 1) // cus
    out.append(_case("adder-default-n3072", 3072, form=None, adder=1, R=R, RP=32))
    out.append(_case("adder-default-n3071-is-classic", 3071, form=None, adder=0, tail_g=16, main_rows=0))
    return out


# ---- data, evaluation, checks ---------------------------------------------------------------------------------------------------
def _rowmap(rng, nrows, max_stored=500):
    """session row -> stored row: runs of 1 .. 40 rows (long runs mixed in where that would store more than max_stored rows), a
    run across every wave / block border, the last rows one run"""
    runs = rng.choice([1, 1, 1, 2, 3, 5, 17, 40], size=nrows)
    if nrows > 8 * max_stored:
        runs = np.where(rng.random(nrows) < 0.5, max(40, 2 * nrows // max_stored), runs)
    rm = np.repeat(np.arange(len(runs)), runs)[:nrows]
    rm[-min(nrows, 70):] = rm[-min(nrows, 70)]
    return np.cumsum(np.concatenate([[0], np.diff(rm) != 0])).astype(np.int32)


def make_data(case):
    """the arrays of a case; deterministic in the case id"""
    n, nrows, pitch = case["n"], case["nrows"], case["pitch"]
    seed = int.from_bytes(case["id"].encode(), "little") % (2 ** 31)
    rng = np.random.default_rng(seed)
    d = {"ld": M.clustered(n, seed) if case["coords"] == "clustered" else M.uniform(n, seed, case["coords"])}
    # the points at 1e16: p = the clipped q, so that their terms are zeros and every row sum still feels each of its other terms
    # (tests/_seq_model.py::clustered; without this an order swap in the 8-lane form went unnoticed on these coordinates)
    huge = M.huge_points(d["ld"])
    if case["src"] == "lut":
        import kmap_amd.visualization as V
        d["lut"] = V.hd_prob_lut(8, 20, 3200).copy()
        d["lut"][3200] = M.Q_LO                                       # the probability of the columns `huge`, see below
        if case["rowmap"]:
            d["rowmap"] = _rowmap(rng, nrows)
        stored = int(d["rowmap"][-1]) + 1 if case["rowmap"] else nrows
        d["sums"] = rng.integers(0, 3200, size=(stored, pitch), dtype=np.uint16)      # padding columns: garbage in range of the LUT
        d["sums"][:, huge] = 3200
    else:
        P = rng.random((nrows, pitch), dtype=np.float32)
        P[rng.random((nrows, pitch)) < 0.05] = 1.0
        P[:, huge] = M.Q_LO
        d["P"] = P
    return d


def evaluate(V, case, d):
    """one force evaluation of the case -> (gradient [2, n], loss partial, geometry)"""
    from kmap_amd import _ffi
    n, row0, nrows = case["n"], case["row0"], case["nrows"]
    sess = V.EmbedSession(n, 1, 0.01, V.EMBED_SEQ, row0=row0, nrows=nrows)
    try:
        if case["src"] == "lut":
            md = _ffi.DeviceBuffer.from_numpy(d["rowmap"]) if "rowmap" in d else None
            sess.set_prob_lut(_ffi.DeviceBuffer.from_numpy(d["sums"]), case["pitch"], d["lut"], md, len(d["sums"]))
        else:
            sess.set_prob_f32(_ffi.DeviceBuffer.from_numpy(d["P"]), case["pitch"])
        sess.set_coords(d["ld"])
        geo = sess.seq_geometry()
        g_d = _ffi.DeviceBuffer.from_numpy(np.full((2, n), FILL, np.float32))
        l_d = _ffi.DeviceBuffer.from_numpy(np.full(1, -1.0, np.float64))
        sess.forces(g_d.ptr, l_d.ptr)
        _ffi.sync()
        return g_d.to_numpy(np.float32, (2, n)), float(l_d.to_numpy(np.float64, (1,))[0]), geo
    finally:
        sess.close()


def regions(geo, nrows):
    """[(name, first local row, end, rows per wave, rows per block)] of the launch the geometry describes"""
    if geo["adder"]:
        return [(f"adder R={geo['R']} RP={geo['RP']} M={geo['M']} EA={geo['EA']}", 0, nrows, geo["R"], geo["R"])]
    out = [("pair", 0, geo["pair_rows"], 32, 128), ("quad", geo["pair_rows"], geo["main_rows"], 16, 64)]
    if geo["tail_g"]:
        rw = 64 // geo["tail_g"]
        out.append((f"wide {geo['tail_g']}", geo["main_rows"], nrows, rw, 4 * rw))
    return [r for r in out if r[2] > r[1]]


def pick_rows(case, geo):
    """local rows to check: all where n <= 4096, else the borders, the batch-edge diagonals, the last rows and a random rest"""
    n, row0, nrows = case["n"], case["row0"], case["nrows"]
    if n <= 4096 or nrows <= MAX_ROWS:
        return np.arange(nrows)
    rows = []
    for _, s, e, w, b in regions(geo, nrows):
        lw, lb = s + ((e - 1 - s) // w) * w, s + ((e - 1 - s) // b) * b
        rows += [r for r in (s, s + 1, s + w - 1, s + w, s + b - 1, s + b, lw - 1, lw, lb - 1, lb, e - 2, e - 1) if s <= r < e]
    for m in (32, 64, 128, 256, 512):
        for res in (0, 1, m - 1):
            for anchor in (row0, row0 + nrows // 2, row0 + nrows - m):
                i = anchor + ((res - anchor) % m)
                if row0 <= i < row0 + nrows:
                    rows.append(i - row0)
    rows += [r for r in (n - 1 - row0, n - 2 - row0) if 0 <= r < nrows]
    rows = sorted(set(rows))
    assert len(rows) <= MAX_ROWS
    rest = np.setdiff1d(np.arange(nrows), rows)
    extra = np.random.default_rng(n + nrows).choice(rest, size=MAX_ROWS - len(rows), replace=False)
    return np.sort(np.concatenate([rows, extra]).astype(np.int64))


def _p_rows(case, d, rows):
    if case["src"] == "lut":
        return M.p_rows_lut(d["lut"], d["sums"], rows, case["n"], d.get("rowmap"))
    return np.ascontiguousarray(d["P"][rows, :case["n"]])


def check(case, d, g, loss, geo):
    n, row0, nrows = case["n"], case["row0"], case["nrows"]
    for k, v in case["expect"].items():
        assert geo[k] == v, f"{case['id']}: this device runs another form than the case pins: {k} = {geo[k]}, expected {v} ({geo})"
    regs = regions(geo, nrows)
    rows = pick_rows(case, geo)
    want = M.grad_rows(d["ld"], row0 + rows, _p_rows(case, d, rows))
    got = g[:, row0 + rows]
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=0))[0]
    if len(bad):
        where = [(int(rows[b]), next(nm for nm, s, e, _, _ in regs if s <= rows[b] < e)) for b in bad[:8]]
        b = bad[0]
        raise AssertionError(f"{case['id']}: {len(bad)} of {len(rows)} checked rows differ from the model; local rows / form: {where}; "
                             f"row {int(rows[b])}: got {got[:, b]!r} want {want[:, b]!r}")
    outside = np.concatenate([g[:, :row0], g[:, row0 + nrows:]], axis=1)
    assert (outside.view(np.uint32) == FILL.view(np.uint32)).all(), f"{case['id']}: entries of rows outside the session were written"
    assert len(rows) < 2 or np.abs(want).max() > 0
    if nrows * n <= LOSS_PAIRS:
        allr = np.arange(nrows)
        ref = M.loss_rows(d["ld"], row0 + allr, _p_rows(case, d, allr))
        dev = abs(loss - ref) / abs(ref) if ref else abs(loss)
        print(f"{case['id']}: {[r[0] for r in regs]} loss {loss!r} model {ref!r} rel {dev:.3g}")
        assert dev <= LOSS_RTOL, f"{case['id']}: loss {loss!r}, model {ref!r}, relative {dev:.3g} > {LOSS_RTOL}"


def _run_in_process(V, monkeypatch, case):
    if case["form"] is None:
        monkeypatch.delenv("KMAP_SEQ_FORM", raising=False)
    else:
        monkeypatch.setenv("KMAP_SEQ_FORM", case["form"])       # read by every kmap_embed_create
    d = make_data(case)
    g, loss, geo = evaluate(V, case, d)
    check(case, d, g, loss, geo)


@pytest.fixture(scope="module")
def V():
    import kmap_amd.visualization as vz
    return vz


@pytest.mark.parametrize("case", classic_cases(), ids=lambda c: c["id"])
def test_classic_forms_below_a_round(V, monkeypatch, case):
    _run_in_process(V, monkeypatch, case)


def _late(maker):
    """the cases of a group whose shapes depend on the CU count: made where a device exists, indexed by position"""
    return len(maker(256)), lambda i: maker(_cus())[i]


N_ROUND, _round_case = _late(round_cases)
N_PAIR, _pair_case = _late(pair_cases)
N_ADDER, _adder_case = _late(adder_cases)


@pytest.mark.parametrize("i", range(N_ROUND), ids=[c["id"] for c in round_cases(256)])
def test_forms_behind_a_full_round(V, monkeypatch, i):
    """the wide form with 8 lanes per row (remainders of 4 x SIMDs + 1 .. 8 x SIMDs rows) runs in no other test"""
    _run_in_process(V, monkeypatch, _round_case(i))


@pytest.mark.parametrize("i", range(N_PAIR), ids=[c["id"] for c in pair_cases(256)])
def test_pair_form(V, monkeypatch, i):
    _run_in_process(V, monkeypatch, _pair_case(i))


@pytest.mark.parametrize("i", range(N_ADDER), ids=[c["id"] for c in adder_cases(256)])
def test_producer_adder_form(V, monkeypatch, i):
    _run_in_process(V, monkeypatch, _adder_case(i))


# ---- the quad form at small N: one child process with KMAP_SEQ_TAIL=0 ------------------------------------------------------------
def child_main(path_in, path_out):
    """runs in the child: evaluate every case of the input file"""
    import json
    import kmap_amd.visualization as V
    inp = np.load(path_in)
    cases = json.loads(str(inp["cases"]))
    out = {}
    for k, case in enumerate(cases):
        d = {key[len(f"c{k}_"):]: inp[key] for key in inp.files if key.startswith(f"c{k}_")}
        g, loss, geo = evaluate(V, case, d)
        out[f"c{k}_g"], out[f"c{k}_loss"] = g, np.float64(loss)
        out[f"c{k}_geo"] = np.array([geo[key] for key in ("adder", "main_rows", "pair_rows", "tail_g", "R", "RP", "M", "EA")], np.int64)
    np.savez(path_out, **out)


@pytest.fixture(scope="module")
def quad_results(tmp_path_factory):
    import json
    tmp = tmp_path_factory.mktemp("seq_quad")
    cases = quad_cases()
    data = [make_data(c) for c in cases]
    arrays = {f"c{k}_{key}": v for k, d in enumerate(data) for key, v in d.items()}
    np.savez(tmp / "in.npz", cases=np.array(json.dumps(cases)), **arrays)
    code = "import sys; sys.path.insert(0, sys.argv[1]); from tests.test_gpu_seq_forms import child_main; child_main(sys.argv[2], sys.argv[3])"
    r = subprocess.run([sys.executable, "-c", code, str(ROOT), str(tmp / "in.npz"), str(tmp / "out.npz")],
                       env=dict(os.environ, KMAP_SEQ_TAIL="0", KMAP_SEQ_FORM="classic"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return cases, data, np.load(tmp / "out.npz")


@pytest.mark.parametrize("k", range(len(quad_cases())), ids=[c["id"] for c in quad_cases()])
def test_quad_form_at_small_n(quad_results, k):
    cases, data, out = quad_results
    geo = dict(zip(("adder", "main_rows", "pair_rows", "tail_g", "R", "RP", "M", "EA"), (int(v) for v in out[f"c{k}_geo"])))
    check(cases[k], data[k], out[f"c{k}_g"], float(out[f"c{k}_loss"]), geo)


def test_the_case_list_reaches_every_form():
    """by the geometry every case asserts: tail_g = 8, 16, 32, 64 and 0, a pair region, both adder geometries, every (M, EA) layout"""
    cus = _cus()
    exps = [c["expect"] for c in classic_cases() + quad_cases() + round_cases(cus) + pair_cases(cus) + adder_cases(cus)]
    assert {e["tail_g"] for e in exps if "tail_g" in e} == {0, 8, 16, 32, 64}
    assert any(e.get("pair_rows", 0) > 0 for e in exps)
    layouts = {(e["RP"], e["M"], e["EA"]) for e in exps if e["adder"] and "M" in e}
    assert {rp for rp, _, _ in layouts} == {32, 64}
    assert {(m, ea) for _, m, ea in layouts} == {(2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1)}
