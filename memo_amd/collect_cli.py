"""`memo collect`: how the core and the covered k-mers of a pivot genome region change as genomes are added (the collector's curve).

`memo query`'s flags (-b -k -n -r -o) with another product: instead of one membership line per position, one line per number of
genomes -- core = the positions whose k-mer is in every genome added so far, covered = those whose k-mer is in at least one of
them -- for the index order 1 .. N - 1, or with -p over random orders, as a band (minimum, mean, maximum) or with -a order by
order.  The window is swept as `memo query -m` sweeps it, in slices, each slice is reduced where it lies (memo_amd/collect.py,
memo_amd/csrc/memo_collect.hip), and only the curves leave the device.  One GPU.
"""
from . import _cli

USAGE = """
MEMO collect - core and covered k-mers of a pivot genome region as genomes are added (collector's curve)
Usage: ./memo collect [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: tab-separated, a header line, then one line per number of genomes (the pivot alone first)
  -p [INT]               random orders of the genomes instead of the index order: minimum, mean and maximum over them [0]
  -s [INT]               seed of the random orders [0]
  -a                     with -p: every order in turn instead of the band over them
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): name the genome each line adds (not with a band)

"""

cli = _cli.Cli("collect", USAGE, "b:k:n:r:o:p:s:ag:", {"-k": "31", "-p": "0", "-s": "0"})
refuse, read_labels = cli.refuse, cli.read_labels


def main(argv):
    """bin/memo collect [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    n_docs, k, perms, seed = cli.integers(val, "-n", "-k", "-p", "-s")
    if perms < 0:
        refuse(f"-p {perms}: the number of random orders cannot be negative")
    form = "curve" if perms == 0 else "long" if "-a" in val else "band"
    if "-g" in val and form == "band":
        refuse("-g names the genome a line adds: a band over random orders (-p without -a) has none")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import collect

    def run():
        device = _cli.device()
        _, qs, qe = collect.parse_region(val["-r"])
        order_rows = collect.orders(n_docs, perms, seed)
        core, covered = collect.region_curves(val["-b"], val["-r"], k, n_docs, order_rows, device)
        _cli.write_text(val["-o"], collect.format_curves(qe - qs, core, covered, form, order_rows, labels))
    cli.guarded(run)
