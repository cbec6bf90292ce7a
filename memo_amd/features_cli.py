"""`memo features`: which genomes hold every feature of a BED file, or how conserved it is.

The other sub-commands answer for one `-r CHR:START-END` window; the question a user brings is usually shaped like an annotation:
for each gene, exon or sliding window of this BED file.  This reads the file once, sweeps every record it names once per batch of
features and writes one line per feature, in the file's order: with -m (a membership index) how many of the feature's k-mers each
genome holds -- with -p the presence/absence matrix most pangenome analyses start from -- and without it (a conservation index) the
sum of the conservation values and the positions shared by at least -t genomes.  Features may overlap, nest, repeat and come in any
order; the table is counted per elementary segment between their endpoints and summed per feature on the GPU
(memo_amd/features.py, memo_amd/csrc/memo_features.hip).  One GPU.
"""
from . import _cli

N_MAX = 2048

USAGE = """
MEMO features - per-feature k-mer presence or conservation, for the features of a BED file
Usage: ./memo features [options]

Basic options:
  -b [FILE]              parquet membership or conservation MEMO index (nothing in the file tells them apart: -m says which)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot), at most 2048 with -m
  -a [FILE]              BED file of features: tab-separated chrom, start, end[, name], 0-indexed, half open '[)' coordinates
  -o [FILE]              output file: tab-separated, a header line, then one line per feature in the BED file's order
  -m                     the index is a MEMBERSHIP index: one column per genome, genome 0 (the pivot) first, the positions of the
                         feature at which the genome holds the pivot's k-mer (on a conservation index the numbers mean nothing)
                         without -m the index is a conservation index: the sum of the values, and the positions shared by at least -t
  -f                     write fractions of the feature's positions instead of counts (nan for a feature of no positions)
  -p [FLOAT]             with -m: write 1 where a genome holds at least this fraction (0 < p <= 1) of the feature's k-mers, else 0
  -t [INT]               without -m: a position is shared when at least this many genomes hold its k-mer [-n]
  -i                     count only k-mers that lie wholly inside the feature: the positions [start, end - k + 1)
  -g [FILE]              with -m: the genome list `memo index -g` took (first line the pivot): name the columns by file name

"""


cli = _cli.Cli("features", USAGE, "b:k:n:a:o:mfp:t:ig:", {"-k": "31"})
refuse, read_labels = cli.refuse, cli.read_labels


def main(argv):
    """bin/memo features [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-a", "-n", "-o"))
    cli.one_gpu_only()
    n_docs, k = cli.integers(val, "-n", "-k")
    membership = "-m" in val
    if n_docs < 1 or (membership and n_docs > N_MAX):
        refuse(f"-n must be in [1, {N_MAX}] with -m, and at least 1 without (got {n_docs})")
    if k < 1:
        refuse(f"-k must be at least 1 (got {k})")
    if "-f" in val and "-p" in val:
        refuse("-f and -p together: fractions or calls, not both")
    for flag in ("-p", "-g"):
        if flag in val and not membership:
            refuse(f"{flag} needs -m: a conservation index has no genome columns")
    if "-t" in val and membership:
        refuse("-t has no meaning with -m: it is the threshold of a conservation index")
    fraction = None
    if "-p" in val:
        try:
            fraction = float(val["-p"])
        except ValueError:
            fraction = 0.0
        if not 0.0 < fraction <= 1.0:               # (nan fails both)
            refuse(f"-p must be a fraction in (0, 1] (got {val['-p']!r})")
    threshold = cli.integer("-t", val["-t"], 1, n_docs, f"[1, {n_docs}]") if "-t" in val else None
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import features
    try:
        bed = features.read_bed(val["-a"])
    except OSError as exc:
        refuse(f"cannot read the BED file {val['-a']}: {exc.strerror}")
    except ValueError as exc:                       # (a line that is refused, with its number; bytes that are no text)
        refuse(str(exc))

    def run():
        table, positions = features.bed_features(val["-b"], bed, k, n_docs, membership, threshold, "-i" in val, _cli.device())
        if fraction is not None:
            table = features.calls(table, positions, fraction)
        elif "-f" in val:
            table = features.shares(table, positions)
        _cli.write_text(val["-o"], features.format_features(bed, positions, table, membership, labels))
    cli.guarded(run)
