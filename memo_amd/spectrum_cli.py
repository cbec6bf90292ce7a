"""`memo spectrum`: how much of a pivot genome region is shared by how many genomes, at every k-mer size at once.

`memo query` and `memo view` answer that for one k a call.  This writes the whole table from one pass over the index rows: one line
per k from 1 to -K, and in it the number of positions of the region whose k-mer is held by exactly 0, 1 ... N genomes -- the histogram
of what `memo query -k k` would write -- or, with -c, by at least 1 ... N genomes.  It reads either kind of index; nothing in the file
tells them apart, so -m says that it is a membership index (memo_amd/spectrum.py, memo_amd/csrc/memo_spectrum.hip).  One GPU.
"""
import os

from . import _cli

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


cli = _cli.Cli("spectrum", USAGE, "b:n:r:o:mK:c")
refuse = cli.refuse


def main(argv):
    """bin/memo spectrum [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    n_docs, = cli.integers(val, "-n")
    if not 1 <= n_docs <= N_MAX:
        refuse(f"-n must be in [1, {N_MAX}] (got {n_docs})")
    kmax = cli.integer("-K", val.get("-K", "128"), 1, KMAX_MAX, f"[1, {KMAX_MAX}]")
    # (tests force a window into several slices with it; the result does not depend on it)
    slice_positions = cli.integer("MEMO_LENGTHS_SLICE", os.environ["MEMO_LENGTHS_SLICE"], 1, 2 ** 31, "[1, 2^31]") if os.environ.get("MEMO_LENGTHS_SLICE") else None
    from . import lengths, spectrum

    def run():
        device = _cli.device()
        _, qs, L, _ = lengths.region_window(val["-r"], kmax)
        # an empty window is an empty file
        text = spectrum.emit(spectrum.region_exact(val["-b"], val["-r"], n_docs, kmax, "-m" in val, device, slice_positions), "-c" in val) if L else b""
        _cli.write_bytes(val["-o"], text)
    cli.guarded(run)
