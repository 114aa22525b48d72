"""`kmap` command line: the three verbs of the reference's CLI that sit on the GPU hot path
(reference cli.py:9-36, kmer_count.py:70-101, motif_discovery.py:29-53, visualization.py:18-33),
with the same option names, plus `ex_hamball` (motif_discovery.py:74-108; Hamming-ball extraction on the GPU),
`extract_motif_locations` (util.py:42-71; motif hits mapped to genome coordinates through a BED file, merged and sorted on the GPU)
and `check_motif_co_occurence` (motif_discovery.py:111-177; occurrence scan of two user motifs and their co-occurrence tables, no
figures), and ten verbs the reference does not have: `project_kmers`, new k-mers placed on the map `visualize_kmers` wrote, without moving
its points (projection.py), and `scan_pwm`, every read position scored against the base-count matrices scan_motif and ex_hamball
write, with a strand, a score and a p-value threshold per hit (pwm.py), and `enrich_kmers`, the k-mers and motifs of a result
directory scored against control reads instead of the uniform null: both read sets counted on the GPU, the tables joined there, a
pooled two-proportion z per k-mer and an exact top-N selection (enrichment.py), and `refine_pwm`, a count matrix iterated on the
reads -- scan, select, count the selected windows' bases -- until it reproduces itself (refine.py), and `evaluate_pwm`, the best
window score of every read and of every control read under a count matrix, compared by a rank statistic (AUROC, Mann-Whitney z) and
by the two-proportion z at every score threshold (evaluate.py), and `shuffle_reads`, the control reads for those two when there is
no second read set: every read shuffled on the GPU so that its length, its N and its base or dinucleotide counts stay (shuffle.py), and
`rank_motif_library`, evaluate_pwm's comparison for a whole library of known motifs (MEME text or count matrices) in batched passes
over the reads, ranked, with Benjamini-Hochberg q-values (library.py), and `match_motifs`, count matrices compared with a library of
count matrices column by column, at every offset and on both strands, with a p-value from the library's own columns: the nearest
known motif of a discovered one, and the families of a library matched against itself (motif_match.py), and `motif_centrality`,
where in the reads the best site of every motif of a library lies: the sites within a half-width of the read centre against a site
placed uniformly, the half-width with the largest z, ranked, with q-values, no control needed (centrality.py), and `motif_spacing`,
at which distance, on which side and on which relative strand of a primary motif's site the best non-overlapping site of every motif
of a library lies: pair reads per (side, strand, gap) bin against a uniformly placed site, a Poisson tail for the best bin, ranked,
with q-values (spacing.py).  An eleventh, `motif_cooccurrence`, asks which pairs of motifs of a library share reads more or less often
than their own frequencies predict: one presence bit per motif and read, the shared reads of all pairs counted on the GPU, a
hypergeometric z per pair, two-sided p-values and q-values (cooccurrence.py).  A twelfth, `discover_pwms`, makes the library the others
consume: the k-mers most enriched against control reads become seeds, every seed grows from the Hamming ball around it into a
count matrix by refine_pwm's iteration -- all seeds in lockstep, one batched counting pass over the reads per round --, and the
matrices are evaluated against the control and grouped into families, one representative each (discover.py); with `--erase_rounds R`
it erases the sites of what a round found from reads and control and discovers again on what is left, so that a weaker motif behind
a dominant one gets seeds of its own.  A thirteenth, `erase_pwm_sites`, is that erasure for a library of known motifs: every position
inside a hit becomes N, and the reads that are left are written as FASTA for `preproc` (erase.py).  The reference's plotting / alignment verbs (draw_logo, align_conseq, plot_network) are out of scope here (SURVEY.md
section 2).  `scan_motif` and `visualize_kmers` shard over the
GPUs of a node when launched through `python -m torch.distributed.run --nproc-per-node G -m kmap_amd <verb> ...`."""
import click

from . import __version__


@click.group()
def cli():
    """KMAP on MI355X: k-mer counting, motif scan and 2-D k-mer embedding (HIP kernels)."""


def display_paper_info():
    print()
    print(f"kmap_amd {__version__} -- MI355X/gfx950 implementation of the kmap hot path")
    print("method: KMAP, Fu et al., bioRxiv 2024, doi:10.1101/2024.04.12.589197")
    print()


@cli.command(name="preproc")
@click.option("--fasta_file", type=str, required=True, help="Input fasta file")
@click.option("--res_dir", type=str, default=".", required=False, help="Result directory for storing all outputs")
@click.option("--gpu_mode", type=bool, default=True, required=False, help="kept for CLI compatibility (always GPU)")
@click.option("--debug", type=bool, default=False, required=False, help="display debug information.")
def preproc(fasta_file, res_dir=".", gpu_mode=True, debug=False):
    from .kmer_count import _preproc
    _preproc(fasta_file, res_dir, debug)


@cli.command(name="scan_motif")
@click.option("--res_dir", type=str, required=True, help="Result directory for storing all outputs")
@click.option("--gpu_mode", type=bool, default=True, required=False, help="kept for CLI compatibility (always GPU)")
@click.option("--debug", type=bool, default=False, required=False, help="display debug information.")
def scan_motif(res_dir, gpu_mode=True, debug=False):
    from .motif_discovery import _scan_motif
    _scan_motif(res_dir, debug)


@cli.command(name="visualize_kmers")
@click.option("--res_dir", type=str, required=True, help="Result directory for storing all outputs")
@click.option("--debug", type=bool, default=False, required=False, help="display debug information.")
def visualize_kmers(res_dir, debug=False):
    from .visualization import _visualize_kmers
    _visualize_kmers(res_dir, debug)


@cli.command(name="ex_hamball")
@click.option("--res_dir", type=str, required=True, help="Result directory for storing all outputs")
@click.option("--conseq", type=str, required=True, help="the consensus sequence")
@click.option("--return_type", type=str, required=True, help='output file form, can be ["hash" | "kmer" | "matrix"]')
@click.option("--output_file", type=str, required=True, help="output file name, including the suffix")
@click.option("--max_ham_dist", type=int, default=-1, required=False,
              help="The radius of the Hamming ball. -1 means taking the radius from motif_def_table.csv")
def ex_hamball(res_dir, conseq, return_type, output_file, max_ham_dist=-1):
    from .reports import _ex_hamball
    _ex_hamball(res_dir, conseq, return_type, output_file, max_ham_dist)


@cli.command(name="extract_motif_locations")
@click.option("--bed_file", type=str, required=True,
              help="Input bed file with no header, each line corresponds to each read in the input fasta file")
@click.option("--conseq_file", type=str, default="./final_conseq.txt", required=False, help="Input conseq file")
@click.option("--motif_occurrence_file", type=str, default="./final.motif_occurence.csv", required=False,
              help="Input motif occurrence file")
@click.option("--output_dir", type=str, default="./motif_locations", required=False,
              help="Output directory for storing motif locations")
def extract_motif_locations(bed_file, conseq_file="./final_conseq.txt", motif_occurrence_file="./final.motif_occurence.csv",
                            output_dir="./motif_locations"):
    from .locations import _extract_motif_locations
    _extract_motif_locations(bed_file, conseq_file, motif_occurrence_file, output_dir)


@cli.command(name="check_motif_co_occurence")
@click.option("--input_fasta_file", type=str, required=True, help="Input FASTA file")
@click.option("--motif1", type=str, required=True, help="First motif sequence")
@click.option("--motif2", type=str, required=True, help="Second motif sequence")
@click.option("--max_ham_dist1", type=int, required=True, help="Maximum Hamming distance for first motif")
@click.option("--max_ham_dist2", type=int, required=True, help="Maximum Hamming distance for second motif")
@click.option("--output_dir", type=str, required=True, help="Output directory")
@click.option("--revcom_mode", type=bool, default=True, required=False, help="Consider reverse complements")
def check_motif_co_occurence(input_fasta_file, motif1, motif2, max_ham_dist1, max_ham_dist2, output_dir, revcom_mode=True):
    from .locations import check_motif_co_occurence as run
    run(input_fasta_file, motif1, motif2, max_ham_dist1, max_ham_dist2, output_dir, revcom_mode)


@cli.command(name="project_kmers")
@click.option("--res_dir", type=str, required=True, help="Result directory of scan_motif / visualize_kmers (holds low_dim_data.tsv)")
@click.option("--kmer_file", type=str, required=True, help="Input file, one k-mer per line, of the sampled k-mers' length")
@click.option("--output_file", type=str, default=None, required=False,
              help="output file name, including the suffix (default: projected_kmers.tsv in res_dir)")
@click.option("--n_iter", type=int, default=100, required=False, help="gradient steps per projected k-mer")
def project_kmers(res_dir, kmer_file, output_file=None, n_iter=100):
    from .projection import _project_kmers
    _project_kmers(res_dir, kmer_file, output_file, n_iter)


@cli.command(name="scan_pwm")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--matrix_file", type=str, required=True, multiple=True,
              help="4 x w base-count matrix (rows A, C, G, T; comma-separated, as scan_motif and `ex_hamball --return_type matrix` "
                   "write them); may be given several times")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="a window is a hit when at most this share of all 4^w sequences scores as high; per strand and per position "
                   "(not corrected for the two strands or the number of positions)")
@click.option("--min_score", type=float, default=None, required=False,
              help="score threshold in bits; replaces the threshold derived from --p_value")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and report the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: pwm_scan in res_dir)")
def scan_pwm(res_dir, matrix_file, p_value=1e-4, min_score=None, pseudocount=1.0, revcom_mode=None, output_dir=None):
    from .pwm import _scan_pwm
    _scan_pwm(res_dir, list(matrix_file), p_value, min_score, pseudocount, revcom_mode, output_dir)


@cli.command(name="refine_pwm")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--matrix_file", type=str, required=True, multiple=True,
              help="4 x w base-count matrix to start from (rows A, C, G, T; comma-separated, as scan_motif and `ex_hamball "
                   "--return_type matrix` write them); may be given several times")
@click.option("--flank", type=int, default=0, required=False,
              help="empty columns added on each side before the first iteration (width + 2 x flank <= 31)")
@click.option("--select", type=click.Choice(["best", "all"]), default="best", required=False,
              help="windows counted per iteration: the best hit of every read (ties: the smallest loc), or every hit -- on a motif "
                   "with a reverse-palindromic core `all` counts both strands of one site and drifts")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="hit threshold of every iteration, as scan_pwm's: per strand and per position")
@click.option("--pseudocount", type=float, default=1.0, required=False,
              help="pseudocount added to every column (a quarter per base); must be > 0 with --flank")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and count the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--max_iter", type=int, default=20, required=False, help="largest number of iterations")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: pwm_refine in res_dir)")
def refine_pwm(res_dir, matrix_file, flank=0, select="best", p_value=1e-4, pseudocount=1.0, revcom_mode=None, max_iter=20,
               output_dir=None):
    from .refine import _refine_pwm
    _refine_pwm(res_dir, list(matrix_file), flank, select, p_value, pseudocount, revcom_mode, max_iter, output_dir)


@cli.command(name="enrich_kmers")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--control_fasta_file", type=str, required=True,
              help="FASTA file of the control reads (input DNA, flanks, round 0, shuffled reads); counted like the reads of res_dir")
@click.option("--kmer_len", type=int, multiple=True, required=False,
              help="k-mer length to rank, 1..31; may be given several times (default: none, the motif table only)")
@click.option("--top_n", type=int, default=1000, required=False, help="rows per enriched_kmers_k{k}.tsv: the k-mers with the largest z")
@click.option("--min_count", type=int, default=2, required=False, help="smallest foreground count of a ranked k-mer")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount of the log2 fold change")
@click.option("--conseq_file", type=str, default=None, required=False,
              help="consensus sequences, one per line, for motif_enrichment.csv (default: final_conseq.txt in res_dir, when it exists)")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: kmer_enrichment in res_dir)")
def enrich_kmers(res_dir, control_fasta_file, kmer_len=(), top_n=1000, min_count=2, pseudocount=1.0, conseq_file=None, output_dir=None):
    from .enrichment import _enrich_kmers
    _enrich_kmers(res_dir, control_fasta_file, list(kmer_len), top_n, min_count, pseudocount, conseq_file, output_dir)


@cli.command(name="evaluate_pwm")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--control_fasta_file", type=str, required=True,
              help="FASTA file of the control reads (input DNA, flanks, round 0, shuffled reads); scored like the reads of res_dir")
@click.option("--matrix_file", type=str, required=True, multiple=True,
              help="4 x w base-count matrix (rows A, C, G, T; comma-separated, as scan_motif, `ex_hamball --return_type matrix` and "
                   "refine_pwm write them); may be given several times")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="the reads above scan_pwm's threshold of this p-value are compared too (per strand and per position)")
@click.option("--min_score", type=float, default=None, required=False,
              help="score threshold in bits; replaces the threshold derived from --p_value")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and keep the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--min_reads", type=int, default=10, required=False,
              help="the best threshold is sought among those that at least this many reads (of both sets together) reach")
@click.option("--read_scores", is_flag=True, default=False, help="also write the best score, loc and strand of every read")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: pwm_eval in res_dir)")
def evaluate_pwm(res_dir, control_fasta_file, matrix_file, p_value=1e-4, min_score=None, pseudocount=1.0, revcom_mode=None,
                 min_reads=10, read_scores=False, output_dir=None):
    from .evaluate import _evaluate_pwm
    _evaluate_pwm(res_dir, control_fasta_file, list(matrix_file), p_value, min_score, pseudocount, revcom_mode, min_reads, read_scores,
                  output_dir)


@cli.command(name="rank_motif_library")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--control_fasta_file", type=str, required=True,
              help="FASTA file of the control reads (input DNA, flanks, round 0, shuffled reads); scored like the reads of res_dir")
@click.option("--library_file", type=str, required=True, multiple=True,
              help="motif library: a MEME minimal text file, a 4 x w base-count matrix CSV (as for evaluate_pwm), or a directory of "
                   "*.meme and *.csv files; may be given several times")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="the reads above scan_pwm's threshold of this p-value are compared too (per strand and per position)")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--nsites_default", type=int, default=20, required=False,
              help="sites behind a MEME motif without nsites= (its probabilities become counts of this many sites)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and keep the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--min_reads", type=int, default=10, required=False,
              help="the best threshold is sought among those that at least this many reads (of both sets together) reach")
@click.option("--top_hist", type=int, default=0, required=False, help="also write the score histograms of this many best-ranked motifs")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: pwm_library in res_dir)")
def rank_motif_library(res_dir, control_fasta_file, library_file, p_value=1e-4, pseudocount=1.0, nsites_default=20, revcom_mode=None,
                       min_reads=10, top_hist=0, output_dir=None):
    from .library import _rank_motif_library
    _rank_motif_library(res_dir, control_fasta_file, list(library_file), p_value, pseudocount, nsites_default, revcom_mode, min_reads,
                        top_hist, output_dir)


@cli.command(name="match_motifs")
@click.option("--query_file", type=str, required=True, multiple=True,
              help="query motifs: a 4 x w base-count matrix CSV, a MEME minimal text file, or a directory of *.meme and *.csv files; "
                   "may be given several times")
@click.option("--library_file", type=str, required=False, multiple=True,
              help="motif library, in the same formats; may be given several times (default: the queries are matched against "
                   "themselves and grouped into families)")
@click.option("--revcom_mode", type=bool, default=True, required=False, help="also try the reverse complement of every target")
@click.option("--min_overlap", type=int, default=5, required=False,
              help="fewest columns two motifs overlap in (at least 1; a motif narrower than this overlaps in all its columns)")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--nsites_default", type=int, default=20, required=False,
              help="sites behind a MEME motif without nsites= (its probabilities become counts of this many sites)")
@click.option("--top_n", type=int, default=10, required=False, help="targets listed per query")
@click.option("--family_e_value", type=float, default=0.01, required=False,
              help="all against all: two motifs are linked when each finds the other with an E-value of at most this")
@click.option("--output_dir", type=str, default="./motif_matches", required=False, help="Output directory")
def match_motifs(query_file, library_file=(), revcom_mode=True, min_overlap=5, pseudocount=1.0, nsites_default=20, top_n=10,
                 family_e_value=0.01, output_dir="./motif_matches"):
    from .motif_match import _match_motifs
    _match_motifs(list(query_file), list(library_file), revcom_mode, min_overlap, pseudocount, nsites_default, top_n, family_e_value,
                  output_dir)


@cli.command(name="motif_centrality")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--library_file", type=str, required=True, multiple=True,
              help="motif library: a MEME minimal text file, a 4 x w base-count matrix CSV (as for evaluate_pwm), or a directory of "
                   "*.meme and *.csv files; may be given several times")
@click.option("--control_fasta_file", type=str, default=None, required=False,
              help="FASTA file of control reads: the share of sites inside the best region is compared with theirs (optional)")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="a read is a site read when its best window reaches scan_pwm's threshold of this p-value (per strand and per position)")
@click.option("--min_score", type=float, default=None, required=False,
              help="score threshold in bits; replaces the threshold derived from --p_value")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--nsites_default", type=int, default=20, required=False,
              help="sites behind a MEME motif without nsites= (its probabilities become counts of this many sites)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and keep the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--min_half", type=int, default=0, required=False,
              help="smallest half-width tried, in half bases (the doubled distance of a site's centre from the read's centre)")
@click.option("--min_sites", type=int, default=10, required=False, help="a motif with fewer site reads gets no z (p = 1)")
@click.option("--top_hist", type=int, default=5, required=False, help="also write the site offsets of this many best-ranked motifs")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: motif_centrality in res_dir)")
def motif_centrality(res_dir, library_file, control_fasta_file=None, p_value=1e-4, min_score=None, pseudocount=1.0, nsites_default=20,
                     revcom_mode=None, min_half=0, min_sites=10, top_hist=5, output_dir=None):
    from .centrality import _motif_centrality
    _motif_centrality(res_dir, list(library_file), control_fasta_file, p_value, min_score, pseudocount, nsites_default, revcom_mode,
                      min_half, min_sites, top_hist, output_dir)


@cli.command(name="motif_spacing")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--primary_file", type=str, required=True,
              help="the primary motif: a 4 x w base-count matrix CSV or a MEME minimal text file with exactly one motif that can be "
                   "scored (or --primary_name)")
@click.option("--primary_name", type=str, default=None, required=False, help="the motif of --primary_file to take, by its name")
@click.option("--library_file", type=str, required=True, multiple=True,
              help="motif library: a MEME minimal text file, a 4 x w base-count matrix CSV (as for evaluate_pwm), or a directory of "
                   "*.meme and *.csv files; may be given several times")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="a window is a site when it reaches scan_pwm's threshold of this p-value (per strand and per position); for the "
                   "primary motif and the library")
@click.option("--primary_min_score", type=float, default=None, required=False,
              help="score threshold of the primary motif in bits; replaces the threshold derived from --p_value")
@click.option("--min_score", type=float, default=None, required=False,
              help="score threshold of the library motifs in bits; replaces the thresholds derived from --p_value")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--nsites_default", type=int, default=20, required=False,
              help="sites behind a MEME motif without nsites= (its probabilities become counts of this many sites)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and keep the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--max_gap", type=int, default=150, required=False,
              help="largest number of bases between the two sites that gets a bin (0..511); pairs further apart are counted as far")
@click.option("--min_pairs", type=int, default=10, required=False, help="a motif with fewer pair reads within --max_gap gets no bin (p = 1)")
@click.option("--top_hist", type=int, default=5, required=False, help="also write the gap histograms of this many best-ranked motifs")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: motif_spacing in res_dir)")
def motif_spacing(res_dir, primary_file, library_file, primary_name=None, p_value=1e-4, primary_min_score=None, min_score=None,
                  pseudocount=1.0, nsites_default=20, revcom_mode=None, max_gap=150, min_pairs=10, top_hist=5, output_dir=None):
    from .spacing import _motif_spacing
    _motif_spacing(res_dir, primary_file, list(library_file), primary_name, p_value, primary_min_score, min_score, pseudocount,
                   nsites_default, revcom_mode, max_gap, min_pairs, top_hist, output_dir)


@cli.command(name="motif_cooccurrence")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--library_file", type=str, required=True, multiple=True,
              help="motif library: a MEME minimal text file, a 4 x w base-count matrix CSV (as for evaluate_pwm), or a directory of "
                   "*.meme and *.csv files; may be given several times")
@click.option("--control_fasta_file", type=str, default=None, required=False,
              help="FASTA file of control reads: every written pair's shared count is compared with theirs (optional)")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="a read holds a motif when its best window reaches scan_pwm's threshold of this p-value (per strand and per position)")
@click.option("--min_score", type=float, default=None, required=False,
              help="score threshold in bits; replaces the threshold derived from --p_value")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--nsites_default", type=int, default=20, required=False,
              help="sites behind a MEME motif without nsites= (its probabilities become counts of this many sites)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and keep the better one (default: kmer_count.revcom_mode of config.toml)")
@click.option("--min_expected", type=float, default=5.0, required=False,
              help="a pair is tested when the expected shared count, and either motif's reads beyond it, are at least this")
@click.option("--top_n", type=int, default=1000, required=False,
              help="rows of cooccurrence_pairs.csv: the tested pairs with the largest |z|; 0 writes every pair")
@click.option("--write_matrix", is_flag=True, default=False, help="also write the matrix of shared read counts, pair_counts.tsv")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: motif_cooccurrence in res_dir)")
def motif_cooccurrence(res_dir, library_file, control_fasta_file=None, p_value=1e-4, min_score=None, pseudocount=1.0, nsites_default=20,
                       revcom_mode=None, min_expected=5.0, top_n=1000, write_matrix=False, output_dir=None):
    from .cooccurrence import _motif_cooccurrence
    _motif_cooccurrence(res_dir, list(library_file), control_fasta_file, p_value, min_score, pseudocount, nsites_default, revcom_mode,
                        min_expected, top_n, write_matrix, output_dir)


@cli.command(name="discover_pwms")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--control_fasta_file", type=str, required=True,
              help="FASTA file of the control reads (input DNA, flanks, round 0, shuffled reads); counted and scored like the reads of res_dir")
@click.option("--seed_len", type=int, default=8, required=False, help="length of the seed k-mers (at least 4; seed_len + 2 x flank <= 31)")
@click.option("--n_seeds", type=int, default=64, required=False, help="seeds: the k-mers with the largest z > 0 against the control, 1..1024")
@click.option("--seed_mismatches", type=int, default=1, required=False,
              help="the first iteration selects the windows within this many mismatches of the seed (0 .. seed_len - 1)")
@click.option("--seed_count", type=int, default=20, required=False, help="the count a seed's matrix holds at the k-mer's base of every column")
@click.option("--flank", type=int, default=2, required=False, help="empty columns added on each side of a seed")
@click.option("--min_count", type=int, default=2, required=False, help="smallest foreground count of a seed k-mer")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="hit threshold of the later iterations and of the evaluation, as scan_pwm's: per strand and per position")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base); > 0")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="count, score and match on both strands (default: kmer_count.revcom_mode of config.toml)")
@click.option("--max_iter", type=int, default=20, required=False, help="largest number of iterations")
@click.option("--min_overlap", type=int, default=5, required=False, help="fewest columns two matrices overlap in when they are matched")
@click.option("--family_e_value", type=float, default=0.01, required=False,
              help="two matrices are linked when each finds the other with an E-value of at most this")
@click.option("--output_dir", type=str, default=None, required=False, help="Output directory (default: pwm_discovery in res_dir)")
@click.option("--erase_rounds", type=int, default=1, required=False,
              help="rounds of discovery, 1..16: after every round but the last the sites of the round's representatives are erased "
                   "from reads and control, and the next round takes its seeds from what is left (1: no erasure)")
def discover_pwms(res_dir, control_fasta_file, seed_len=8, n_seeds=64, seed_mismatches=1, seed_count=20, flank=2, min_count=2,
                  p_value=1e-4, pseudocount=1.0, revcom_mode=None, max_iter=20, min_overlap=5, family_e_value=0.01, output_dir=None,
                  erase_rounds=1):
    from .discover import _discover_pwms
    rounds = () if erase_rounds == 1 else (erase_rounds,)        # one round is the call this verb has always made
    _discover_pwms(res_dir, control_fasta_file, seed_len, n_seeds, seed_mismatches, seed_count, flank, min_count, p_value, pseudocount,
                   revcom_mode, max_iter, min_overlap, family_e_value, output_dir, *rounds)


@cli.command(name="erase_pwm_sites")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds config.toml and the encoded reads)")
@click.option("--library_file", type=str, required=True, multiple=True,
              help="motif library: a MEME minimal text file, a 4 x w base-count matrix CSV (as for evaluate_pwm), or a directory of "
                   "*.meme and *.csv files; may be given several times")
@click.option("--p_value", type=float, default=1e-4, required=False,
              help="every window that reaches scan_pwm's threshold of this p-value is erased (per strand and per position)")
@click.option("--min_score", type=float, default=None, required=False,
              help="score threshold in bits; replaces the threshold derived from --p_value")
@click.option("--pseudocount", type=float, default=1.0, required=False, help="pseudocount added to every column (a quarter per base)")
@click.option("--nsites_default", type=int, default=20, required=False,
              help="sites behind a MEME motif without nsites= (its probabilities become counts of this many sites)")
@click.option("--revcom_mode", type=bool, default=None, required=False,
              help="score both strands and erase on the better one's score (default: kmer_count.revcom_mode of config.toml)")
@click.option("--output_file", type=str, default=None, required=False,
              help="output FASTA file (default: erased_reads.fa in res_dir), a --fasta_file for preproc")
def erase_pwm_sites(res_dir, library_file, p_value=1e-4, min_score=None, pseudocount=1.0, nsites_default=20, revcom_mode=None,
                    output_file=None):
    from .erase import _erase_pwm_sites
    _erase_pwm_sites(res_dir, list(library_file), p_value, min_score, pseudocount, nsites_default, revcom_mode, output_file)


@cli.command(name="shuffle_reads")
@click.option("--res_dir", type=str, required=True, help="Result directory of preproc (holds the encoded reads)")
@click.option("--klet", type=int, default=2, required=False,
              help="what every read keeps: 1 its base counts, 2 its first base and its dinucleotide counts (hence its last base)")
@click.option("--seed", type=int, default=0, required=False, help="0 .. 2^64 - 1; the same seed writes the same file")
@click.option("--n_copies", type=int, default=1, required=False, help="shuffled copies of every read, written copy after copy")
@click.option("--output_file", type=str, default=None, required=False,
              help="output FASTA file (default: shuffled_control.fa in res_dir), a --control_fasta_file for enrich_kmers / evaluate_pwm")
def shuffle_reads(res_dir, klet=2, seed=0, n_copies=1, output_file=None):
    from .shuffle import _shuffle_reads
    _shuffle_reads(res_dir, klet, seed, n_copies, output_file)
