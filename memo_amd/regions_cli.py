"""`memo regions`: the conservation or membership of a pivot genome region as intervals.

`memo query`'s flags (-b -k -n -r -o -m) with another product: instead of one line per position, one line per maximal run
of equal values -- a bedGraph for a genome browser, a BED3 of the regions inside a band of conservation values (-t / -T) for
bedtools, or a BED with one 0/1 character per genome (-m).  The window is swept as `memo query` sweeps it, the result is
run-coded where it lies (memo_amd/regions.py, memo_amd/csrc/memo_runs.hip), and only the runs leave the device.  One GPU.
"""
import getopt
import os
import sys

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


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo regions: {message}\n")
    sys.exit(status)


def _bound(flag, text, n_docs):
    try:
        value = int(text)
    except ValueError:
        value = -1
    if not 0 <= value <= n_docs:
        refuse(f"{flag} must be an integer in [0, {n_docs}] (got {text!r})")
    return value


def main(argv):
    """bin/memo regions [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:k:n:r:o:mt:T:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {"-k": "31"}
    for o, a in opts:
        val[o] = a
    print("MEMO - regions", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported -- use memo query")
    membership, band = "-m" in val, "-t" in val or "-T" in val
    if membership and band:
        refuse("-m cannot be combined with -t / -T: a band is a question about conservation values")
    try:
        n_docs, k = int(val["-n"]), int(val["-k"])
    except ValueError as exc:
        refuse(str(exc))
    lo = hi = None
    if band:
        lo = _bound("-t", val["-t"], n_docs) if "-t" in val else 0
        hi = _bound("-T", val["-T"], n_docs) if "-T" in val else n_docs
        if lo > hi:
            refuse(f"-t {lo} is above -T {hi}: no value lies in that band")
    from . import regions
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        result = regions.region_runs(val["-b"], val["-r"], k, n_docs, membership, lo, hi, device)
        text = regions.emit(result)

        def write(tmp):
            with open(tmp, "wb") as fh:
                fh.write(memoryview(text))
        _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), the sweep's own IndexError
    # (index.check), a record that is not there.  Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
