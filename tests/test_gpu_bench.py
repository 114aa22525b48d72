"""bench.py as the driver runs it, on the GPU: the ONE stdout line must parse (round 5's 25-KB line did not)."""
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_bench_prints_one_compact_line_and_a_detail_file(tmp_path):
    """`python3 bench.py --gpus 1 --steps 3 --warmup 1 --full` with the long legs switched off (the C3 pipeline, the headline, `stages`,
    `c5` and a quick `cpu_baseline` still run): stdout is exactly one line of strict JSON <= 4096 bytes with the contract keys, `roofline`
    and `cpu_baseline`; the detail file it names exists, is strict JSON and holds the legs; the headline agrees with its own numbers."""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--quick", "--no-c4", "--no-embed-dist",
           "--shard-proxy", "0", "--e2e", "none", "--time-budget", "200"]
    r = subprocess.run(cmd, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    assert len(lines[0].encode()) <= 4096

    def no_const(c):
        raise AssertionError(f"non-finite constant {c} in the line")
    d = json.loads(lines[0], parse_constant=no_const)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "ranks_seen", "distinct_gpus", "detail"):
        assert key in d, key
    assert d["metric"] == "hamming_pairs_per_s" and d["unit"] == "pairs/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["dtype"] == "u8" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["higher_is_better"] is True
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and 0.3 < rf["frac"] < 1.0
    assert abs(rf["achieved"] - rf["algorithmic_bytes"] / (rf["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * rf["achieved"]
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    n = d["config"]["n_kmers"]
    assert n == 50000 and abs(d["value"] - n * n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "pairs/s" and cb["cores"] >= 1 and cb["value"] > 0
    det = json.loads((ROOT / d["detail"]).read_text(), parse_constant=no_const)
    assert det["metric"] == d["metric"] and "stages" in det["roofline"] and "c5" in det and det["leg_errors"] == []
    assert {"count_pass_k8", "count_pass_k14", "count_k14_keyspace_rank", "scan_k8_r2", "embed_iter_seq"} <= set(det["roofline"]["stages"])
    assert 0.3 < det["c5"]["frac"] < 1.0 and "oracle" in det["c5"]["spot_check"]


def test_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    """`python3 bench.py --gpus 1 --steps 7 --warmup 2 --dump-outputs DIR` (no --full): one strict-JSON line whose `steps` is the number
    asked for and whose `value` follows from `ms_per_step`; none of the --full extras (no leg, no spot-check figures, no detail file);
    DIR holds the seeded row sample of the last timed step's matrix as float32 (distances 0..k, zero on the diagonal, the sampled
    rows x sampled columns block symmetric) and its row numbers, <= 64 MB in all; rows of it equal the oracle's rows of the sample
    the whole C3 pipeline (both verbs, as --full runs it) hands over, rebuilt here"""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = tmp_path / "outputs"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]

    def no_const(c):
        raise AssertionError(f"non-finite constant {c} in the line")
    d = json.loads(lines[0], parse_constant=no_const)
    assert d["metric"] == "hamming_pairs_per_s" and d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0
    n = d["config"]["n_kmers"]
    assert n == 50000 and abs(d["value"] - n * n / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["detail"] is None and d["roofline"]["frac_of_achievable"] is None
    assert not {"cpu_baseline", "e2e_c3_s", "c5_frac", "skipped_legs", "leg_errors"} & set(d)
    rows, idx = np.load(out / "hamming_rows.npy"), np.load(out / "hamming_row_index.npy")
    assert rows.dtype == np.float32 and idx.dtype == np.float64 and rows.shape == (len(idx), n) and len(idx) > 0
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
    ri = idx.astype(np.int64)
    assert np.array_equal(ri, idx) and np.all(np.diff(ri) > 0) and 0 <= ri[0] and ri[-1] < n
    assert np.array_equal(rows, np.round(rows)) and rows.min() >= 0 and rows.max() <= d["config"]["k"]
    sub = rows[:, ri]
    assert np.all(np.diag(sub) == 0) and np.array_equal(sub, sub.T) and np.count_nonzero(sub) > 0

    sys.path.insert(0, str(ROOT))
    import bench
    from kmap_amd.e2e import run_e2e, synth_config_reads
    from oracle import oracle as O
    res_dir = run_e2e("C3", "default", reads=synth_config_reads("C3"), keep=True)["res_dir"]
    try:
        kh, lab, lens, _ = bench.pipeline_sample(res_dir, n)
    finally:
        shutil.rmtree(res_dir, ignore_errors=True)
    for i in (0, len(ri) // 2, len(ri) - 1):
        want = np.empty((1, n), np.uint8)
        O.lib().ko_hamdist_rows(np.ascontiguousarray(kh, np.uint64), lab, n, d["config"]["k"], np.ascontiguousarray(lens, np.int32), len(lens),
                                int(ri[i]), 1, want)
        np.testing.assert_array_equal(rows[i], want[0].astype(np.float32), err_msg=f"row {ri[i]}")
