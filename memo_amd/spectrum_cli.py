"""`memo spectrum`: how much of a pivot genome region is shared by how many genomes, at every k-mer size at once.

`memo query` and `memo view` answer that for one k a call.  This writes the whole table from one pass over the index rows: one line
per k from 1 to -K, and in it the number of positions of the region whose k-mer is held by exactly 0, 1 ... N genomes -- the histogram
of what `memo query -k k` would write -- or, with -c, by at least 1 ... N genomes.  It reads either kind of index; nothing in the file
tells them apart, so -m says that it is a membership index (memo_amd/spectrum.py, memo_amd/csrc/memo_spectrum.hip).  One GPU.
"""
import getopt
import os
import sys

KMAX_MAX = 1024
N_MAX = 2048

USAGE = """
MEMO spectrum - conservation histogram of a pivot genome region at every k-mer size
Usage: ./memo spectrum [options]

Basic options:
  -b [FILE]              parquet membership or conservation MEMO index
  -n [INT]               total number of documents in pangenome (include the pivot), at most 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: tab-separated, a header line, then one line per k-mer size
  -m                     the index is a membership index (instead of a conservation index)
  -K [INT]               largest k-mer size, at most 1024 [128]
  -c                     cumulative: positions held by at least 1 ... N genomes (instead of by exactly 0 ... N)

"""


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo spectrum: {message}\n")
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
    """bin/memo spectrum [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:n:r:o:mK:c")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {}
    for o, a in opts:
        val[o] = a
    print("MEMO - spectrum", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    try:
        n_docs = int(val["-n"])
    except ValueError as exc:
        refuse(str(exc))
    if not 1 <= n_docs <= N_MAX:
        refuse(f"-n must be in [1, {N_MAX}] (got {n_docs})")
    kmax = _integer("-K", val.get("-K", "128"), 1, KMAX_MAX, f"[1, {KMAX_MAX}]")
    # (tests force a window into several slices with it; the result does not depend on it)
    slice_positions = _integer("MEMO_LENGTHS_SLICE", os.environ["MEMO_LENGTHS_SLICE"], 1, 2 ** 31, "[1, 2^31]") if os.environ.get("MEMO_LENGTHS_SLICE") else None
    from . import lengths, spectrum
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        _, qs, L, _ = lengths._region(val["-r"], kmax)
        # an empty window is an empty file
        text = spectrum.emit(spectrum.region_exact(val["-b"], val["-r"], n_docs, kmax, "-m" in val, device, slice_positions), "-c" in val) if L else b""

        def write(tmp):
            with open(tmp, "wb") as fh:
                fh.write(text)
        _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), a record that is not there.
    # Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
