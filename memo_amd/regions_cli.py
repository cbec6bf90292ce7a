"""`memo regions`: the conservation or membership of a pivot genome region as intervals.

`memo query`'s flags (-b -k -n -r -o -m) with another product: instead of one line per position, one line per maximal run
of equal values -- a bedGraph for a genome browser, a BED3 of the regions inside a band of conservation values (-t / -T) for
bedtools, or a BED with one 0/1 character per genome (-m).  The window is swept as `memo query` sweeps it, the result is
run-coded where it lies (memo_amd/regions.py, memo_amd/csrc/memo_runs.hip), and only the runs leave the device.  One GPU.
"""
from . import _cli

USAGE = """
MEMO regions - k-mer conservation or membership of a pivot genome region as intervals
Usage: ./memo regions [options]

Basic options:
  -b [FILE]              parquet membership or conservation MEMO index
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: bedGraph (CHR START END VALUE), one line per run of equal conservation
  -t [INT]               only the intervals with conservation >= MIN, as BED3 (-t N: what every genome shares)
  -T [INT]               only the intervals with conservation <= MAX, as BED3 (with -t: MIN <= conservation <= MAX)
  -m                     membership index: CHR START END and one 0/1 character per genome, one line per run of equal rows

"""


cli = _cli.Cli("regions", USAGE, "b:k:n:r:o:mt:T:", {"-k": "31"})
refuse = cli.refuse


def _bound(flag, text, n_docs):
    return cli.integer(flag, text, 0, n_docs, f"[0, {n_docs}]")


def main(argv):
    """bin/memo regions [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    if _cli.sharded_launch():
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported -- use memo query")
    membership, band = "-m" in val, "-t" in val or "-T" in val
    if membership and band:
        refuse("-m cannot be combined with -t / -T: a band is a question about conservation values")
    n_docs, k = cli.integers(val, "-n", "-k")
    lo = hi = None
    if band:
        lo = _bound("-t", val["-t"], n_docs) if "-t" in val else 0
        hi = _bound("-T", val["-T"], n_docs) if "-T" in val else n_docs
        if lo > hi:
            refuse(f"-t {lo} is above -T {hi}: no value lies in that band")
    from . import regions

    def run():
        result = regions.region_runs(val["-b"], val["-r"], k, n_docs, membership, lo, hi, _cli.device())
        _cli.write_bytes(val["-o"], regions.emit(result))
    cli.guarded(run)
