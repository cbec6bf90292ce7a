"""`memo convert`: the conservation index of a pangenome from its membership index, without going back to the genomes.

`memo index -m` and `memo index` build their two indexes from the same matching statistics, and those are the whole cost.  The
membership index still holds them: this reads every genome's match lengths back (`memo lengths`), and feeds them to the row builder
`memo index` ends with.  Without -m the output is the conservation index (`memo query`, `memo maxk -t`, `memo view`, `memo regions`
answer from it as from any other); with -m it is the membership index in canonical form, the row builder run without --order
(memo_amd/convert.py, memo_amd/csrc/memo_convert.hip).  One GPU.
"""
from . import _cli

N_MAX = 2048

USAGE = """
MEMO convert - a conservation index from a membership index
Usage: ./memo convert [options]

Basic options:
  -b [FILE]              parquet membership MEMO index
  -n [INT]               total number of documents in pangenome (include the pivot), 2 to 2048
  -o [FILE]              output file: the parquet conservation MEMO index of the same pangenome
  -m                     write the membership index in canonical form instead
  -f [FILE]              .fai of the pivot: record lengths, where a record is longer than its largest row start

"""


cli = _cli.Cli("convert", USAGE, "b:n:o:mf:")


def main(argv):
    """bin/memo convert [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched and before anything is written
    cli.require(val, ("-b", "-n", "-o"))
    cli.one_gpu_only()
    n_docs, = cli.integers(val, "-n")
    if not 2 <= n_docs <= N_MAX:
        cli.refuse(f"-n must be in [2, {N_MAX}] (got {n_docs})")
    from . import convert
    cli.guarded(lambda: convert.convert_index(val["-b"], val["-o"], n_docs, order="-m" not in val, fai=val.get("-f"),
                                              device=_cli.device(), log=lambda line: None))
