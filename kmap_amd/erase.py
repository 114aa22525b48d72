"""`kmap erase_pwm_sites`: the reads without the sites of known motifs (the reference has no such verb).

The library is read and its thresholds are found as the library verbs do it; csrc/pwm_erase.hip marks every position inside a hit of
any of its matrices invalid in one call, and the reads are written back as FASTA with N at every invalid position -- a --fasta_file
for `preproc`, so scan_motif or any other verb runs on what is left.  Host code here is argument checking and the two files; the
erasure has no CPU path."""
from pathlib import Path

import numpy as np

from .library import load_library
from .pwm import min_score_threshold, pwm_consensus

OUTPUT_FILE, INFO_FILE = "erased_reads.fa", "erase_info.csv"
INFO_HEADER = "name,width,consensus,threshold,hits,covered\n"


def write_erase_info(path, motifs, ts, n_hits, n_covered, n_new):
    """erase_info.csv: one row per motif, then the total line: all hits, and the positions erased (the union of the covers)"""
    with open(path, "w") as fh:
        fh.write(INFO_HEADER)
        for m, t, h, c in zip(motifs, ts, n_hits, n_covered):
            fh.write(f"{m.name},{m.counts.shape[1]},{pwm_consensus(m.counts)},{int(t)},{int(h)},{int(c)}\n")
        fh.write(f"total,,,,{int(np.sum(n_hits))},{int(n_new)}\n")


def _erase_pwm_sites(res_dir, library_files, p_value=1e-4, min_score=None, pseudocount=1.0, nsites_default=20, revcom_mode=None,
                     output_file=None):
    """`kmap erase_pwm_sites`: config.toml + the encoded reads of a preproc result directory + library files -> the reads with N at
    every position inside a hit of a library motif (default res_dir/erased_reads.fa, shuffle_reads' writer and read names) and
    erase_info.csv beside it.  Every file is parsed, every threshold found and every ValueError raised before the device is touched
    or a file is written.  Under a torch.distributed launch rank 0 works alone.  Returns (motifs, thresholds, n_hits, n_covered,
    n_new)."""
    from .kmer_count import load_array_pickle, load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    library_files = [str(f) for f in library_files]
    if not library_files:
        raise ValueError("erase_pwm_sites: no library file given")
    t_fixed = None if min_score is None else min_score_threshold(min_score)
    _, revcom = load_config(cfg_path, revcom_mode)
    motifs, _, Ws, plans = load_library("erase_pwm_sites", library_files, nsites_default, pseudocount, p_value, t_fixed)
    ts = [p[0] for p in plans]
    out = res / OUTPUT_FILE if output_file is None else Path(output_file)

    from .motif_discovery import DeviceSeq
    from .shuffle import write_fasta_records
    borders = np.asarray(load_array_pickle(border_path), np.int64).reshape(-1, 2)
    ds = DeviceSeq(load_array_pickle(seq_path), borders)
    try:
        n_hits, n_covered, n_new = ds.erase_sites(Ws, ts, revcom, use_work=False)
        left = ds.download()
    finally:
        ds.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "wb") as fh:
        write_fasta_records(fh, left, borders, 0)
    write_erase_info(out.parent / INFO_FILE, motifs, ts, n_hits, n_covered, n_new)
    print(f"erase_pwm_sites: {len(motifs)} {'motif' if len(motifs) == 1 else 'motifs'}, {int(np.sum(n_hits))} hits, {n_new} positions "
          f"erased in {len(borders)} reads, {'both strands' if revcom else 'forward strand'}: {out}")
    return motifs, ts, n_hits, n_covered, n_new
