"""`memo matrix`: how many k-mer positions of a pivot genome region every pair of genomes shares.

`memo query`'s flags (-b -k -n -r -o) with another product: instead of one membership line per position, one N x N matrix --
C[g][h] = the positions at which genome g and genome h both hold the pivot's k-mer (genome 0 is the pivot, the diagonal each
genome's own count), or with -j the Jaccard distances 1 - C[g][h] / (C[g][g] + C[h][h] - C[g][h]).  The window is swept as
`memo query -m` sweeps it, in slices, each slice is reduced where it lies (memo_amd/matrix.py, memo_amd/csrc/memo_cooc.hip),
and only the matrix leaves the device.  One GPU.
"""
from . import _cli

USAGE = """
MEMO matrix - pairwise k-mer sharing between the genomes of a pivot genome region
Usage: ./memo matrix [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: N tab-separated rows of N counts, genome 0 (the pivot) first
  -j                     write Jaccard distances instead of counts
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): label rows and columns by file name

"""


cli = _cli.Cli("matrix", USAGE, "b:k:n:r:o:jg:", {"-k": "31"})
label_of, read_labels = _cli.label_of, cli.read_labels


def main(argv):
    """bin/memo matrix [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    n_docs, k = cli.integers(val, "-n", "-k")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import matrix

    def run():
        counts = matrix.region_matrix(val["-b"], val["-r"], k, n_docs, _cli.device())
        _cli.write_text(val["-o"], matrix.format_matrix(matrix.jaccard(counts) if "-j" in val else counts, labels))
    cli.guarded(run)
