"""`kmap shuffle_reads`: control reads for enrich_kmers and evaluate_pwm from the reads themselves (the reference
has no such verb).

Every maximal run of valid bases of a read -- a segment; N stays where it is -- is shuffled on the GPU (csrc/shuffle.hip): klet 1 keeps
the segment's base counts, klet 2 its first base and its 16 dinucleotide counts (Altschul-Erickson), uniformly over everything that
does.  Motifs are destroyed; length, GC content, CpG depletion and low-complexity runs stay.  The random draws are counter-based, so a
(res_dir, klet, seed) names one file.  Host code here is argument checking, the seeds of the copies and the FASTA writer; the shuffle
has no CPU path."""
from pathlib import Path

import numpy as np

OUTPUT_FILE = "shuffled_control.fa"
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
KLETS = (1, 2)
WRITE_CHUNK = 1 << 16           # reads per write
_LETTERS = np.full(256, ord("N"), np.uint8)
_LETTERS[:4] = np.frombuffer(b"ACGT", np.uint8)


def mix64(x):
    """the splitmix64 finaliser of csrc/shuffle.hip and csrc/synth.hip on a Python integer"""
    x = (x + GOLDEN) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def copy_seed(seed, copy):
    """the seed the kernel gets for copy number `copy` of a run with `seed`: mix64(seed + copy * GOLDEN mod 2^64)"""
    return mix64((int(seed) + int(copy) * GOLDEN) & MASK64)


def unchanged_by_definition(seq, klet):
    """(segments, bases, segments that a klet shuffle returns as they are: at most 3 bases for klet 2, one base for klet 1) of an
    encoded array"""
    valid = np.asarray(seq) < 4
    edge = np.diff(np.concatenate([[False], valid, [False]]).astype(np.int8))
    lens = np.nonzero(edge == -1)[0] - np.nonzero(edge == 1)[0]
    return len(lens), int(lens.sum()), int((lens <= (3 if klet == 2 else 1)).sum())


def write_fasta_records(fh, seq, borders, copy):
    """one record per read to the binary file fh: `>shuffled_{copy}_{seq_ind}`, then the read on one line, N for every invalid position"""
    seq, borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
    for a in range(0, len(borders), WRITE_CHUNK):
        part = borders[a:a + WRITE_CHUNK]
        lo = int(part[0, 0])
        letters = _LETTERS[seq[lo:int(part[:, 1].max(initial=lo))]].tobytes()
        fh.write(b"".join(b">shuffled_%d_%d\n%s\n" % (copy, a + i, letters[s - lo:e - lo]) for i, (s, e) in enumerate(part.tolist())))


def _shuffle_reads(res_dir, klet=2, seed=0, n_copies=1, output_file=None):
    """`kmap shuffle_reads`: the encoded reads of a preproc result directory -> n_copies shuffled copies of every read in one FASTA
    file (default res_dir/shuffled_control.fa), copy-major, copy c shuffled with copy_seed(seed, c).  Every ValueError is raised
    before the library is loaded or a file is written.  Under a torch.distributed launch rank 0 works alone.  Returns (reads,
    segments, bases, segments unchanged by definition) of one copy."""
    from .kmer_count import load_array_pickle, rank0_only, result_paths
    if not rank0_only():
        return None
    res, seq_path, border_path = result_paths(res_dir, config=False, reads=True)
    if isinstance(klet, bool) or int(klet) != klet or int(klet) not in KLETS:
        raise ValueError(f"klet {klet}: 1 (base counts) or 2 (dinucleotide counts) expected")
    if isinstance(n_copies, bool) or int(n_copies) != n_copies or n_copies < 1:
        raise ValueError(f"n_copies {n_copies} < 1")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed <= MASK64:
        raise ValueError(f"seed {seed} outside 0 .. 2^64 - 1")
    klet, seed, n_copies = int(klet), int(seed), int(n_copies)
    out = res / OUTPUT_FILE if output_file is None else Path(output_file)

    from .motif_discovery import DeviceSeq
    seq, borders = load_array_pickle(seq_path), np.asarray(load_array_pickle(border_path), np.int64).reshape(-1, 2)
    n_seg, n_bases, n_same = unchanged_by_definition(seq, klet)
    src = DeviceSeq(seq, borders)
    try:
        out.parent.mkdir(parents=True, exist_ok=True)
        with open(out, "wb") as fh:
            for c in range(n_copies):
                shuffled = src.shuffled(klet, copy_seed(seed, c))
                try:
                    if shuffled.shuffle_stats != (n_seg, n_bases):
                        raise RuntimeError(f"shuffle_reads: the device found {shuffled.shuffle_stats} (segments, bases), the host "
                                           f"{(n_seg, n_bases)}")
                    write_fasta_records(fh, shuffled.download(), borders, c)
                finally:
                    shuffled.close()
    finally:
        src.close()
    print(f"shuffle_reads: klet {klet}, seed {seed}, {n_copies} {'copy' if n_copies == 1 else 'copies'} of {len(borders)} reads, "
          f"{n_seg} segments, {n_bases} bases, {n_same} segments unchanged by definition: {out}")
    return len(borders), n_seg, n_bases, n_same
