"""`memo maxk`: from every position of a pivot genome region, how long a stretch is still shared.

`memo query`'s flags without -k: instead of the conservation or membership at one k-mer size, one integer per position -- the
largest k (up to -K) at which the k-mer starting there is shared by at least -t genomes (a conservation index; -t defaults to
-n: shared by all), or is held by genome -d (-m: a membership index).  `memo query -k K` says "shared" at a position exactly
when K is at most that position's line.  Every k is answered by one pass over the index rows (memo_amd/maxk.py,
memo_amd/csrc/memo_maxk.hip).  One GPU.
"""
from . import _cli

CAP_MAX = 2 ** 31 - 1

USAGE = """
MEMO maxk - longest shared k-mer from every position of a pivot genome region
Usage: ./memo maxk [options]

Basic options:
  -b [FILE]              parquet conservation MEMO index (with -m: membership MEMO index)
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: one line per position, the largest k at which its k-mer is still shared
  -t [INT]               shared means: by at least T genomes [the -n value: by all]
  -m                     membership index: shared means held by the genome of -d
  -d [INT]               with -m: the genome, 0 (the pivot: every line is the cap) to N - 1
  -K [INT]               cap: no line is larger [2147483647]

"""


cli = _cli.Cli("maxk", USAGE, "b:n:r:o:t:md:K:")
refuse = cli.refuse


def main(argv):
    """bin/memo maxk [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    membership = "-m" in val
    if membership and "-d" not in val:
        refuse("-m needs -d: the genome whose match length is asked for")
    if "-d" in val and not membership:
        refuse("-d is a genome of a membership index: it needs -m")
    if membership and "-t" in val:
        refuse("-t cannot be combined with -m: a threshold is a question about conservation values")
    n_docs, = cli.integers(val, "-n")
    threshold = genome = None
    if membership:
        genome = cli.integer("-d", val["-d"], 0, n_docs - 1, f"[0, {n_docs})")
    else:
        threshold = cli.integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    from . import maxk

    def run():
        text = maxk.emit(maxk.region_maxk(val["-b"], val["-r"], n_docs, threshold, genome, cap, _cli.device()))
        _cli.write_bytes(val["-o"], text)
    cli.guarded(run)
