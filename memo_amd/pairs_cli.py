"""`memo pairs`: how much match length with the pivot every pair of genomes shares over a window, k-free.

`memo matrix` counts the positions two genomes share at one k, which saturates; this sums, per pair, the largest k both still hold
at each position -- `memo matrix` added up over every k of [-l, -K] -- and so does not.  One N x N matrix S, genome 0 the pivot,
the diagonal each genome's own sum (`memo breaks -m -s`'s); with -j the weighted Jaccard (Ruzicka) distances
1 - S[g][h] / (S[g][g] + S[h][h] - S[g][h]), a metric; with -f the mean shared match length S / positions.  No -k, as for
`memo maxk`.  The lengths are `memo lengths`', reduced on the GPU where they lie (memo_amd/pairs.py, memo_amd/csrc/memo_pairs.hip),
and only the matrix leaves the device.  One GPU.
"""
from . import _cli

N_MAX = 2048
CAP_MAX = 2 ** 31 - 1

USAGE = """
MEMO pairs - k-free pairwise shared match length between the genomes of a pivot genome region
Usage: ./memo pairs [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -n [INT]               total number of documents in pangenome (include the pivot), at most 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: N tab-separated rows of N sums, genome 0 (the pivot) first
  -l [INT]               KMIN: the smallest k that is counted [1]
  -K [INT]               KMAX: the largest k that is counted, the cap of the match lengths [2147483647]
                         (up to 33554431 values of k, -K minus -l plus 1, are added in 32 bits per tile; more in 64 bits)
  -j                     write weighted Jaccard distances 1 - sum of min / sum of max instead of sums
  -f                     write the mean shared match length, the sums divided by the window's positions; not with -j
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): label rows and columns by file name

"""


cli = _cli.Cli("pairs", USAGE, "b:n:r:o:l:K:jfg:")
refuse, read_labels = cli.refuse, cli.read_labels


def main(argv):
    """bin/memo pairs [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    if "-j" in val and "-f" in val:
        refuse("-j cannot be combined with -f: a distance has no positions to be divided by")
    n_docs = cli.integer("-n", val["-n"], 1, N_MAX, f"[1, {N_MAX}]")
    kmax = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    kmin = cli.integer("-l", val.get("-l", "1"), 1, kmax, f"[1, {kmax}]")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import matrix, pairs
    from ._window import parse_region

    def run():
        _, qs, qe = parse_region(val["-r"])
        sums = pairs.region_pairs(val["-b"], val["-r"], n_docs, kmin=kmin, kmax=kmax, device=_cli.device())
        if qe == qs:                                       # an empty window: an empty file
            return _cli.write_text(val["-o"], "")
        if "-j" in val:
            sums = matrix.jaccard(sums)
        elif "-f" in val:
            sums = pairs.mean_lengths(sums, qe - qs)
        _cli.write_text(val["-o"], matrix.format_matrix(sums, labels))
    cli.guarded(run)
