"""`memo breaks`: where every genome's matches with the pivot break, and how long they are, per bin or per BED feature.

`memo tracks` and `memo features` count presence at one k, which saturates; this counts what does not: the maximal matches that start
in a bin -- a genome differs from the pivot where one match ends and the next begins, so this is a variant-density track -- or with
-s the sum of the match lengths over the bin's positions, with -f divided by the bin's width: the mean match length.  No -k, as for
`memo maxk`.  With -m (a membership index) one row per genome along a `-r` window in `memo view`'s bins, or one column per genome
and one line per feature of a `-a` BED file; without it (a conservation index) the stretches at least -t genomes share.  The numbers
are the histogram of `memo mems`' starts and the bin sums of `memo lengths`' columns, counted on the GPU where the lengths lie
(memo_amd/breaks.py, memo_amd/csrc/memo_breaks.hip).  One GPU.
"""
from . import _cli

N_MAX = 2048
CAP_MAX = 2 ** 31 - 1

USAGE = """
MEMO breaks - k-free match starts and match lengths per genome, in bins or per feature of a BED file
Usage: ./memo breaks [options]

Basic options:
  -b [FILE]              parquet membership or conservation MEMO index (nothing in the file tells them apart: -m says which)
  -n [INT]               total number of documents in pangenome (include the pivot), at most 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates), cut into -B bins; or
  -a [FILE]              BED file of features: tab-separated chrom, start, end[, name]; exactly one of -r and -a
  -o [FILE]              output file: tab-separated; with -r a header of bins (START-END), then one row per genome;
                         with -a a header line, then one line per feature in the BED file's order
  -B [INT]               with -r: number of genomic bins, those of memo view and memo tracks [500]
  -m                     the index is a MEMBERSHIP index: one row (-r) or column (-a) per genome, genome 0 (the pivot) first
                         (on a conservation index the numbers mean nothing)
  -t [INT]               without -m, a conservation index: the stretches at least this many genomes share [-n];
                         one row labelled >=T with -r, one column (starts, or sum with -s) with -a
  -l [INT]               the shortest match whose start is counted [1] (the length sums do not depend on it)
  -K [INT]               cap: no match is longer, a run of positions at the cap is one match [2147483647]
  -s                     write the sums of the match lengths over the positions instead of the match starts
  -f                     divide by the bin's width or the feature's positions (nan for a feature of no positions)
  -g [FILE]              with -m: the genome list `memo index -g` took (first line the pivot): label genomes by file name

"""


cli = _cli.Cli("breaks", USAGE, "b:n:r:a:o:B:mt:l:K:sfg:")
refuse, read_labels = cli.refuse, cli.read_labels


def main(argv):
    """bin/memo breaks [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-n", "-o"))
    cli.one_gpu_only()
    membership = "-m" in val
    if ("-r" in val) == ("-a" in val):
        refuse("exactly one of -r (a window in bins) and -a (the features of a BED file)")
    if "-B" in val and "-a" in val:
        refuse("-B has no meaning with -a: a feature is its own bin")
    if "-t" in val and membership:
        refuse("-t cannot be combined with -m: the threshold-th largest of the genomes' lengths is not built")
    if "-g" in val and not membership:
        refuse("-g needs -m: a conservation index has no genome rows")
    n_docs = cli.integer("-n", val["-n"], 1, N_MAX, f"[1, {N_MAX}]")
    threshold = None if membership else cli.integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    min_len = cli.integer("-l", val.get("-l", "1"), 1, cap, f"[1, {cap}]")
    n_bins = cli.integer("-B", val.get("-B", "500"), 1, CAP_MAX, "[1, the positions of the window]")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    which = 1 if "-s" in val else 0
    from . import breaks, features, tracks
    how = dict(membership=membership, threshold=threshold, min_len=min_len, cap=cap, device=_cli.device())
    if "-a" in val:
        try:
            bed = features.read_bed(val["-a"])
        except OSError as exc:
            refuse(f"cannot read the BED file {val['-a']}: {exc.strerror}")
        except ValueError as exc:                       # (a line that is refused, with its number; bytes that are no text)
            refuse(str(exc))

    def run_bed():
        table, positions = breaks.bed_breaks(val["-b"], bed, n_docs, **how)
        table = features.shares(table[which], positions) if "-f" in val else table[which]
        names = labels if membership else ["sum" if which else "starts"]
        _cli.write_text(val["-o"], features.format_features(bed, positions, table, True, names))

    def run_region():
        table, edges, qs = breaks.region_breaks(val["-b"], val["-r"], n_docs, n_bins, **how)
        if table.shape[2] == 0:                            # an empty window: an empty file
            return _cli.write_text(val["-o"], "")
        table = tracks.fractions(table[which], edges) if "-f" in val else table[which]
        _cli.write_text(val["-o"], tracks.format_tracks(table, qs, edges, labels if membership else [f">={threshold}"]))
    cli.guarded(run_bed if "-a" in val else run_region)
