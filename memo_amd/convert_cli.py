"""`memo convert`: the conservation index of a pangenome from its membership index, without going back to the genomes.

`memo index -m` and `memo index` build their two indexes from the same matching statistics, and those are the whole cost.  The
membership index still holds them: this reads every genome's match lengths back (`memo lengths`), and feeds them to the row builder
`memo index` ends with.  Without -m the output is the conservation index (`memo query`, `memo maxk -t`, `memo view`, `memo regions`
answer from it as from any other); with -m it is the membership index in canonical form, the row builder run without --order
(memo_amd/convert.py, memo_amd/csrc/memo_convert.hip).  One GPU.
"""
import getopt
import os
import sys

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


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo convert: {message}\n")
    sys.exit(status)


def main(argv):
    """bin/memo convert [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:n:o:mf:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {}
    for o, a in opts:
        val[o] = a
    print("MEMO - convert", flush=True)
    # everything that can be refused is refused before the device is touched and before anything is written
    missing = [f for f in ("-b", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    try:
        n_docs = int(val["-n"])
    except ValueError as exc:
        refuse(str(exc))
    if not 2 <= n_docs <= N_MAX:
        refuse(f"-n must be in [2, {N_MAX}] (got {n_docs})")
    from . import convert
    from ._lib import MemoError
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        convert.convert_index(val["-b"], val["-o"], n_docs, order="-m" not in val, fai=val.get("-f"), device=device, log=lambda line: None)
    # an index or a .fai that is refused (pyarrow's errors are ValueErrors and OSErrors), a device call that fails.
    # Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
