"""`memo add`: grow a membership index by new genomes, without going back to the old ones.

`memo index` spends almost all of its time on matching statistics, one suffix array per genome, and a pangenome grows one assembly at a
time.  The membership index still holds the old genomes' statistics (`memo lengths` reads them back, `memo convert` feeds them to the row
builder), so this computes the new genomes' only, puts them beside the columns read back and runs the row builder once: -o is the
membership index of all N + m genomes in canonical form (the form `memo convert -m` writes), -c the conservation index of the same
genomes, from the same matrix in the same run (memo_amd/add.py, memo_amd/csrc/memo_add.hip).  One GPU.
"""
import getopt
import os
import sys

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


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo add: {message}\n")
    sys.exit(status)


def main(argv):
    """bin/memo add [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:n:g:o:c:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {}
    for o, a in opts:
        val[o] = a
    print("MEMO - add", flush=True)
    # everything that can be refused is refused before the device is touched and before anything is written
    missing = [f for f in ("-b", "-n", "-g") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if val.get("-o", "") == "" and val.get("-c", "") == "":
        refuse("-o or -c required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    try:
        n_docs = int(val["-n"])
    except ValueError as exc:
        refuse(str(exc))
    if not 2 <= n_docs <= N_MAX - 1:
        refuse(f"-n must be in [2, {N_MAX - 1}] (got {n_docs})")
    from . import add, build_index
    from ._lib import MemoError
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        add.add_index(val["-b"], val["-g"], n_docs, out_path=val.get("-o") or None, cons_path=val.get("-c") or None, device=device,
                      log=lambda line: None, piece_bytes=build_index.piece_bytes_from_env(), layout=build_index.dap_layout_from_env(),
                      walk_budget=build_index.walk_budget_from_env())
    # an index, a list or a FASTA that is refused (pyarrow's errors are ValueErrors and OSErrors, build_index's are ValueErrors), a
    # device call that fails.  Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
