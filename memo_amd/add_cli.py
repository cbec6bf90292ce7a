"""`memo add`: grow a membership index by new genomes, without going back to the old ones.

`memo index` spends almost all of its time on matching statistics, one suffix array per genome, and a pangenome grows one assembly at a
time.  The membership index still holds the old genomes' statistics (`memo lengths` reads them back, `memo convert` feeds them to the row
builder), so this computes the new genomes' only, puts them beside the columns read back and runs the row builder once: -o is the
membership index of all N + m genomes in canonical form (the form `memo convert -m` writes), -c the conservation index of the same
genomes, from the same matrix in the same run (memo_amd/add.py, memo_amd/csrc/memo_add.hip).  One GPU.
"""
from . import _cli

N_MAX = 2048

USAGE = """
MEMO add - grow a membership index by new genomes
Usage: ./memo add [options]

Basic options:
  -b [FILE]              parquet membership MEMO index
  -n [INT]               total number of documents in that index (include the pivot), 2 to 2047
  -g [FILE]              document list: the pivot the index was built on, then the new genomes only
  -o [FILE]              output file: the parquet membership MEMO index of all genomes, in canonical form
  -c [FILE]              output file: the parquet conservation MEMO index of all genomes
                         (at least one of -o and -c)

"""


cli = _cli.Cli("add", USAGE, "b:n:g:o:c:")


def main(argv):
    """bin/memo add [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched and before anything is written
    cli.require(val, ("-b", "-n", "-g"))
    if val.get("-o", "") == "" and val.get("-c", "") == "":
        cli.refuse("-o or -c required", 2)
    cli.one_gpu_only()
    n_docs, = cli.integers(val, "-n")
    if not 2 <= n_docs <= N_MAX - 1:
        cli.refuse(f"-n must be in [2, {N_MAX - 1}] (got {n_docs})")
    from . import add, build_index
    cli.guarded(lambda: add.add_index(val["-b"], val["-g"], n_docs, out_path=val.get("-o") or None, cons_path=val.get("-c") or None,
                                      device=_cli.device(), log=lambda line: None, piece_bytes=build_index.piece_bytes_from_env(),
                                      layout=build_index.dap_layout_from_env(), walk_budget=build_index.walk_budget_from_env()))
