"""`memo lengths`: from every position of a pivot genome region, how far every genome of a membership index still matches.

`memo maxk -m -d G` answers that for one genome a call.  This answers it for all of them in one pass over the index rows: with -a
one line per position holds N integers, genome 0 (the pivot) first; without it one integer per position, the T-th largest of
them -- the largest k (up to -K) at which at least -t genomes hold the k-mer starting there (-t defaults to -n: held by all).
`memo query -m -k K` sets genome g's bit at a position exactly when K is at most that genome's integer there, and at least T bits
exactly when K is at most the -t line (memo_amd/lengths.py, memo_amd/csrc/memo_lengths.hip).  One GPU.
"""
import getopt
import os
import sys

CAP_MAX = 2 ** 31 - 1
N_MAX = 2048

USAGE = """
MEMO lengths - every genome's match length from every position of a pivot genome region
Usage: ./memo lengths [options]

Basic options:
  -b [FILE]              parquet membership MEMO index
  -n [INT]               total number of documents in pangenome (include the pivot), at most 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: one line per position
  -t [INT]               the line is the largest k at which at least T genomes hold the k-mer [the -n value: all]
  -a                     the line is N integers instead: the largest k at which genome 0 (the pivot), 1 ... N - 1 holds it
  -K [INT]               cap: no integer is larger [2147483647]

"""


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo lengths: {message}\n")
    sys.exit(status)


def _integer(flag, text, lo, hi, what):
    try:
        value = int(text)
    except ValueError:
        value = lo - 1
    if not lo <= value <= hi:
        refuse(f"{flag} must be an integer in {what} (got {text!r})")
    return value


def _write_all(tmp, slices):
    """the -a text of slices that arrive FROM THE RIGHT, in position order: a window of one slice is written as it comes; else every
    slice's text goes to a file beside the output as it arrives and is copied from there back to front.  One slice's text is in
    memory at a time, and the file beside is gone when this returns or raises."""
    import contextlib
    from . import lengths
    beside = tmp + ".slices"
    try:
        with contextlib.ExitStack() as stack:
            fh = stack.enter_context(open(tmp, "wb"))
            ph, pieces, first = None, [], None

            def keep(text):
                pieces.append((ph.tell(), len(text)))
                ph.write(memoryview(text))
            for _a, _b, planes in slices:
                text = lengths.emit_rows(planes)
                if first is None and ph is None:
                    first = text                                  # (the only slice, unless another follows)
                    continue
                if ph is None:
                    ph = stack.enter_context(open(beside, "w+b"))
                    keep(first)
                    first = None
                keep(text)
            if first is not None:
                fh.write(memoryview(first))
            for at, size in reversed(pieces):
                ph.seek(at)
                while size:
                    block = ph.read(min(size, 1 << 24))
                    if not block:
                        raise OSError(f"{beside} ended early")
                    fh.write(block)
                    size -= len(block)
    finally:
        if os.path.exists(beside):
            os.unlink(beside)


def main(argv):
    """bin/memo lengths [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:n:r:o:t:aK:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {}
    for o, a in opts:
        val[o] = a
    print("MEMO - lengths", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    every = "-a" in val
    if every and "-t" in val:
        refuse("-t cannot be combined with -a: a line holds every genome's length or the T-th largest of them")
    try:
        n_docs = int(val["-n"])
    except ValueError as exc:
        refuse(str(exc))
    if not 1 <= n_docs <= N_MAX:
        refuse(f"-n must be in [1, {N_MAX}] (got {n_docs})")
    threshold = None if every else _integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = _integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    # (tests force a window into several slices with it; the result does not depend on it)
    slice_positions = _integer("MEMO_LENGTHS_SLICE", os.environ["MEMO_LENGTHS_SLICE"], 1, 2 ** 31, "[1, 2^31]") if os.environ.get("MEMO_LENGTHS_SLICE") else None
    from . import lengths, maxk
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        if every:
            _replace_into(val["-o"], lambda tmp: _write_all(tmp, lengths.region_slices(val["-b"], val["-r"], n_docs, cap, device, slice_positions)))
        else:
            text = maxk.emit(lengths.region_kth(val["-b"], val["-r"], n_docs, threshold, cap, device, slice_positions))

            def write(tmp):
                with open(tmp, "wb") as fh:
                    fh.write(memoryview(text))
            _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), a record that is not there.
    # Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
