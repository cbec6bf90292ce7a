"""`memo lengths`: from every position of a pivot genome region, how far every genome of a membership index still matches.

`memo maxk -m -d G` answers that for one genome a call.  This answers it for all of them in one pass over the index rows: with -a
one line per position holds N integers, genome 0 (the pivot) first; without it one integer per position, the T-th largest of
them -- the largest k (up to -K) at which at least -t genomes hold the k-mer starting there (-t defaults to -n: held by all).
`memo query -m -k K` sets genome g's bit at a position exactly when K is at most that genome's integer there, and at least T bits
exactly when K is at most the -t line (memo_amd/lengths.py, memo_amd/csrc/memo_lengths.hip).  One GPU.
"""
import os

from . import _cli

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


cli = _cli.Cli("lengths", USAGE, "b:n:r:o:t:aK:")
refuse = cli.refuse


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
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    every = "-a" in val
    if every and "-t" in val:
        refuse("-t cannot be combined with -a: a line holds every genome's length or the T-th largest of them")
    n_docs, = cli.integers(val, "-n")
    if not 1 <= n_docs <= N_MAX:
        refuse(f"-n must be in [1, {N_MAX}] (got {n_docs})")
    threshold = None if every else cli.integer("-t", val.get("-t", str(n_docs)), 1, n_docs, f"[1, {n_docs}]")
    cap = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    # (tests force a window into several slices with it; the result does not depend on it)
    slice_positions = cli.integer("MEMO_LENGTHS_SLICE", os.environ["MEMO_LENGTHS_SLICE"], 1, 2 ** 31, "[1, 2^31]") if os.environ.get("MEMO_LENGTHS_SLICE") else None
    from . import lengths, maxk

    def run():
        device = _cli.device()
        if every:
            _cli.replace_into(val["-o"], lambda tmp: _write_all(tmp, lengths.region_slices(val["-b"], val["-r"], n_docs, cap, device, slice_positions)))
        else:
            _cli.write_bytes(val["-o"], maxk.emit(lengths.region_kth(val["-b"], val["-r"], n_docs, threshold, cap, device, slice_positions)))
    cli.guarded(run)
