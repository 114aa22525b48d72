"""`kmap refine_pwm`: iterate a base-count matrix to a fixed point on the reads (the reference has no such verb).

scan_pwm finds the occurrences of a count matrix; this module turns the occurrences back into a matrix and repeats: weights and
exact threshold of the matrix (pwm.py), the hits on the packed reads, a selection among them (every hit, or the best one per read)
and the count matrix of the selected windows' oriented bases (csrc/pwm_refine.hip), until the matrix reproduces itself.  `--flank f`
adds f empty columns on each side first, so a matrix can grow beyond the width of the Hamming ball it came from.  Everything is
integer equality: no tolerance, no random numbers, two runs write the same bytes.  Host code here is the loop and small-matrix
arithmetic; the counting has no CPU path."""
from pathlib import Path

import numpy as np

from .pwm import MAX_WIDTH, _check_counts, pwm_consensus, pwm_threshold, pwm_weights, read_count_matrix

TRACE_FILE, INFO_FILE = "refine_trace.csv", "refine_info.csv"
SELECT_MODES = ("best", "all")
STATUSES = ("converged", "cycle", "no_hits", "max_iter")


def pad_matrix(C0, flank):
    """C0 with `flank` all-zero columns on each side; ValueError when the result is wider than 31"""
    C0 = _check_counts(C0)
    f = int(flank)
    if f != flank or f < 0:
        raise ValueError(f"flank {flank} is not an integer >= 0")
    w = C0.shape[1] + 2 * f
    if w > MAX_WIDTH:
        raise ValueError(f"width {C0.shape[1]} + 2 x flank {f} = {w} is more than {MAX_WIDTH}")
    C = np.zeros((4, w), np.int64)
    C[:, f:f + C0.shape[1]] = C0
    return C


def information_bits(C, pseudocount=1.0):
    """sum over the columns of 2 + sum_b f log2 f, f = (C + a/4) / (column sum + a) as in pwm_weights (0 log 0 = 0); a column without
    counts at a = 0 says nothing and adds 0"""
    C = np.asarray(C, np.float64)
    a = float(pseudocount)
    tot = C.sum(axis=0) + a
    f = np.where(tot > 0, (C + a / 4) / np.where(tot > 0, tot, 1.0), 0.25)
    return float((2.0 + (f * np.log2(np.where(f > 0, f, 1.0))).sum(axis=0)).sum())


def refine_matrix(C0, count_fn, flank=0, p_value=1e-4, pseudocount=1.0, max_iter=20):
    """The loop of DESIGN.md section 13 over count_fn(W, t) -> (C' int64[4, w], n_hits, n_selected, n_minus):
    C = C0 padded; per iteration W = pwm_weights(C, a), t = pwm_threshold(W, p)[0], C' = count_fn(W, t); stop when C' == C
    (`converged`), C' equals an earlier matrix of the run (`cycle`), nothing was selected (`no_hits`) or after max_iter iterations
    (`max_iter`).  Returns (result, status, trace): result = the last matrix built from at least one selected window, else the padded
    input; trace = one (iteration, threshold, n_hits, n_selected, n_minus, consensus of C', information_bits of C', cells_changed)
    per iteration, cells_changed = entries in which C' differs from C."""
    C = pad_matrix(C0, flank)
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter {max_iter} is not an integer >= 1")
    result, seen, trace, status = C, [C], [], "max_iter"
    for it in range(1, int(max_iter) + 1):
        W = pwm_weights(C, pseudocount)
        t = pwm_threshold(W, p_value)[0]
        Cn, n_hits, n_sel, n_minus = count_fn(W, t)
        Cn = np.asarray(Cn, np.int64)
        if Cn.shape != C.shape:
            raise ValueError(f"count_fn returned shape {Cn.shape}, expected {C.shape}")
        trace.append((it, int(t), int(n_hits), int(n_sel), int(n_minus), pwm_consensus(Cn), information_bits(Cn, pseudocount),
                      int(np.count_nonzero(Cn != C))))
        if n_sel == 0:
            status = "no_hits"
            break
        result = Cn
        if np.array_equal(Cn, C):
            status = "converged"
            break
        if any(np.array_equal(Cn, S) for S in seen):
            status = "cycle"
            break
        seen.append(Cn)
        C = Cn
    return result, status, trace


def trace_line(motif, row):
    return "%d,%d,%d,%d,%d,%d,%s,%.3f,%d\n" % ((motif,) + tuple(row))


def _refine_pwm(res_dir, matrix_files, flank=0, select="best", p_value=1e-4, pseudocount=1.0, revcom_mode=None, max_iter=20,
                output_dir=None):
    """`kmap refine_pwm`: config.toml + the encoded reads of a preproc result directory + count matrix files -> per matrix
    refined_cntmat_motif{i}_{consensus}.csv (read_count_matrix and `scan_pwm --matrix_file` take it as it is), refine_trace.csv and
    refine_info.csv in output_dir (default res_dir/pwm_refine).  Every matrix is read, padded and its first weights and threshold found
    before the device is touched or a file is written.  Under a torch.distributed launch rank 0 works alone.
    Returns [(result, status, trace)] per matrix."""
    from .kmer_count import load_array_pickle, load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    matrix_files = [str(f) for f in matrix_files]
    if not matrix_files:
        raise ValueError("refine_pwm: no matrix file given")
    if select not in SELECT_MODES:
        raise ValueError(f"refine_pwm: select {select!r} is neither 'best' nor 'all'")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter {max_iter} is not an integer >= 1")
    _, revcom = load_config(cfg_path, revcom_mode)
    inputs = []
    for f in matrix_files:
        C0 = read_count_matrix(f)
        try:
            pwm_threshold(pwm_weights(pad_matrix(C0, flank), pseudocount), p_value)
        except ValueError as exc:
            raise ValueError(f"{f}: {exc}") from None
        inputs.append((f, C0))

    from .motif_discovery import DeviceSeq
    dev_seq = DeviceSeq(load_array_pickle(seq_path), load_array_pickle(border_path))
    try:
        runs = [refine_matrix(C0, lambda W, t: dev_seq.pwm_counts(W, t, revcom, select == "best"), flank, p_value, pseudocount, max_iter)
                for _, C0 in inputs]
    finally:
        dev_seq.close()
    out = res / "pwm_refine" if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / TRACE_FILE, "w") as tr, open(out / INFO_FILE, "w") as info:
        tr.write("motif,iteration,threshold,n_hits,n_selected,n_minus,consensus,information_bits,cells_changed\n")
        info.write("motif,matrix_file,width_in,flank,width,select,pseudocount,p_value,status,iterations,consensus_in,consensus,refined_file\n")
        for i, ((f, C0), (result, status, trace)) in enumerate(zip(inputs, runs)):
            cons = pwm_consensus(result)
            name = f"refined_cntmat_motif{i}_{cons}.csv"
            np.savetxt(out / name, result, delimiter=",", fmt="%d")
            for row in trace:
                tr.write(trace_line(i, row))
            info.write(f"{i},{f},{C0.shape[1]},{int(flank)},{result.shape[1]},{select},{float(pseudocount)!r},{float(p_value)!r},{status},"
                       f"{len(trace)},{pwm_consensus(C0)},{cons},{name}\n")
            last = trace[-1]
            print(f"motif {i} {pwm_consensus(C0)} -> {cons}: {status} after {len(trace)} iteration{'s' if len(trace) != 1 else ''}, "
                  f"{last[3]} windows selected of {last[2]} hits ({last[4]} on '-'), {information_bits(result, pseudocount):.3f} bits")
    print(f"refine_pwm: {len(inputs)} {'matrix' if len(inputs) == 1 else 'matrices'}, select {select}, "
          f"{'both strands' if revcom else 'forward strand'}: {out}")
    return runs
