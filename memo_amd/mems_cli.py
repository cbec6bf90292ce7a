"""`memo mems`: the maximal shared matches of a pivot genome region, as intervals.

`memo maxk`'s flags and a list instead of one line per position: every stretch that at least -t genomes share (a conservation
index, or with -m a membership index; -t defaults to -n: shared by all), or in which genome -d follows the pivot (-m -d), or that of
every genome (-m -a, a fourth column names the genome), as REC start end lines, 0-based and half open.  A match is written by the
window it starts in and is not clipped at the window's end; -l drops the matches shorter than MINLEN; -u writes the bases that lie in
a stretch of at least MINLEN instead, as maximal intervals.  The list is compacted on the GPU from the lengths of `memo maxk` /
`memo lengths` where they lie (memo_amd/mems.py, memo_amd/csrc/memo_mems.hip).  One GPU.
"""
import getopt
import os
import sys

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


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo mems: {message}\n")
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
    """bin/memo mems [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:n:r:o:t:md:al:K:u")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {}
    for o, a in opts:
        val[o] = a
    print("MEMO - mems", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
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
    try:
        n_docs = int(val["-n"])
    except ValueError as exc:
        refuse(str(exc))
    threshold = genome = None
    if "-d" in val:
        genome = _integer("-d", val["-d"], 0, n_docs - 1, f"[0, {n_docs})")
    elif not every:
        threshold = _integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = None if union else _integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    top = CAP_MAX if union else cap
    min_len = _integer("-l", val.get("-l", "1"), 1, top, f"[1, {top}]")
    from . import mems
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        text = mems.emit(mems.region_mems(val["-b"], val["-r"], n_docs, threshold=threshold, genome=genome, membership=membership,
                                          all_genomes=every, min_len=min_len, cap=cap, union=union, device=device))

        def write(tmp):
            with open(tmp, "wb") as fh:
                fh.write(memoryview(text))
        _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), a record that is not there.
    # Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
