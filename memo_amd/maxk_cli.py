"""`memo maxk`: from every position of a pivot genome region, how long a stretch is still shared.

`memo query`'s flags without -k: instead of the conservation or membership at one k-mer size, one integer per position -- the
largest k (up to -K) at which the k-mer starting there is shared by at least -t genomes (a conservation index; -t defaults to
-n: shared by all), or is held by genome -d (-m: a membership index).  `memo query -k K` says "shared" at a position exactly
when K is at most that position's line.  Every k is answered by one pass over the index rows (memo_amd/maxk.py,
memo_amd/csrc/memo_maxk.hip).  One GPU.
"""
import getopt
import os
import sys

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


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo maxk: {message}\n")
    sys.exit(status)


def _integer(flag, text, lo, hi, what):
    try:
        value = int(text)
    except ValueError:
        value = lo - 1
    if not lo <= value <= hi:
        refuse(f"{flag} must be an integer in {what} (got {text!r})")
    return value


def main(argv):
    """bin/memo maxk [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:n:r:o:t:md:K:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {}
    for o, a in opts:
        val[o] = a
    print("MEMO - maxk", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    membership = "-m" in val
    if membership and "-d" not in val:
        refuse("-m needs -d: the genome whose match length is asked for")
    if "-d" in val and not membership:
        refuse("-d is a genome of a membership index: it needs -m")
    if membership and "-t" in val:
        refuse("-t cannot be combined with -m: a threshold is a question about conservation values")
    try:
        n_docs = int(val["-n"])
    except ValueError as exc:
        refuse(str(exc))
    threshold = genome = None
    if membership:
        genome = _integer("-d", val["-d"], 0, n_docs - 1, f"[0, {n_docs})")
    else:
        threshold = _integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = _integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    from . import maxk
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        text = maxk.emit(maxk.region_maxk(val["-b"], val["-r"], n_docs, threshold, genome, cap, device))

        def write(tmp):
            with open(tmp, "wb") as fh:
                fh.write(memoryview(text))
        _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), a record that is not there.
    # Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
