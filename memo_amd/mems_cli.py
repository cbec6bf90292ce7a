"""`memo mems`: the maximal shared matches of a pivot genome region, as intervals.

`memo maxk`'s flags and a list instead of one line per position: every stretch that at least -t genomes share (a conservation
index, or with -m a membership index; -t defaults to -n: shared by all), or in which genome -d follows the pivot (-m -d), or that of
every genome (-m -a, a fourth column names the genome), as REC start end lines, 0-based and half open.  A match is written by the
window it starts in and is not clipped at the window's end; -l drops the matches shorter than MINLEN; -u writes the bases that lie in
a stretch of at least MINLEN instead, as maximal intervals.  The list is compacted on the GPU from the lengths of `memo maxk` /
`memo lengths` where they lie (memo_amd/mems.py, memo_amd/csrc/memo_mems.hip).  One GPU.
"""
from . import _cli

CAP_MAX = 2 ** 31 - 1

USAGE = """
MEMO mems - maximal shared matches of a pivot genome region, as intervals
Usage: ./memo mems [options]

Basic options:
  -b [FILE]              parquet conservation MEMO index (with -m: membership MEMO index)
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: one line per match that starts in the region, CHR START END (a match is not clipped)
  -t [INT]               shared means: by at least T genomes [the -n value: by all]
  -m                     membership index
  -d [INT]               with -m: the matches of one genome with the pivot, 0 (the pivot: one match of the cap) to N - 1
  -a                     with -m: the matches of every genome 1 to N - 1, a fourth column names the genome
  -l [INT]               the shortest match that is written [1]
  -K [INT]               cap: no match is longer, a run of positions at the cap is one match [2147483647]
  -u                     the bases covered by a stretch of at least -l instead, as maximal intervals (no -K)

"""


cli = _cli.Cli("mems", USAGE, "b:n:r:o:t:md:al:K:u")
refuse = cli.refuse


def main(argv):
    """bin/memo mems [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    membership, every, union = "-m" in val, "-a" in val, "-u" in val
    if "-d" in val and not membership:
        refuse("-d is a genome of a membership index: it needs -m")
    if every and not membership:
        refuse("-a is every genome of a membership index: it needs -m")
    if "-d" in val and every:
        refuse("-d cannot be combined with -a: one genome or all of them")
    if "-t" in val and ("-d" in val or every):
        refuse("-t cannot be combined with -d or -a: a threshold counts genomes, -d and -a name them")
    if union and "-K" in val:
        refuse("-K cannot be combined with -u: the covered bases do not depend on a cap")
    n_docs, = cli.integers(val, "-n")
    threshold = genome = None
    if "-d" in val:
        genome = cli.integer("-d", val["-d"], 0, n_docs - 1, f"[0, {n_docs})")
    elif not every:
        threshold = cli.integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = None if union else cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    top = CAP_MAX if union else cap
    min_len = cli.integer("-l", val.get("-l", "1"), 1, top, f"[1, {top}]")
    from . import mems

    def run():
        text = mems.emit(mems.region_mems(val["-b"], val["-r"], n_docs, threshold=threshold, genome=genome, membership=membership,
                                          all_genomes=every, min_len=min_len, cap=cap, union=union, device=_cli.device()))
        _cli.write_bytes(val["-o"], text)
    cli.guarded(run)
