"""`memo matrix`: how many k-mer positions of a pivot genome region every pair of genomes shares.

`memo query`'s flags (-b -k -n -r -o) with another product: instead of one membership line per position, one N x N matrix --
C[g][h] = the positions at which genome g and genome h both hold the pivot's k-mer (genome 0 is the pivot, the diagonal each
genome's own count), or with -j the Jaccard distances 1 - C[g][h] / (C[g][g] + C[h][h] - C[g][h]).  The window is swept as
`memo query -m` sweeps it, in slices, each slice is reduced where it lies (memo_amd/matrix.py, memo_amd/csrc/memo_cooc.hip),
and only the matrix leaves the device.  One GPU.
"""
import getopt
import os
import sys

USAGE = """
MEMO matrix - pairwise k-mer sharing between the genomes of a pivot genome region
Usage: ./memo matrix [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: N tab-separated rows of N counts, genome 0 (the pivot) first
  -j                     write Jaccard distances instead of counts
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): label rows and columns by file name

"""


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo matrix: {message}\n")
    sys.exit(status)


def label_of(path):
    """a genome's label: its file's base name without extension (a trailing .gz goes first: g1.fa.gz and g1.fa are both g1)"""
    name = os.path.basename(path.strip())
    if name.endswith(".gz"):
        name = name[:-3]
    return os.path.splitext(name)[0]


def read_labels(path, n_docs):
    try:
        with open(path) as fh:
            lines = [ln.strip() for ln in fh if ln.strip()]
    except OSError as exc:
        refuse(f"cannot read the genome list {path}: {exc.strerror}")
    if len(lines) != n_docs:
        refuse(f"-g {path} names {len(lines)} genomes, -n says {n_docs}")
    return [label_of(ln) for ln in lines]


def main(argv):
    """bin/memo matrix [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:k:n:r:o:jg:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {"-k": "31"}
    for o, a in opts:
        val[o] = a
    print("MEMO - matrix", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    try:
        n_docs, k = int(val["-n"]), int(val["-k"])
    except ValueError as exc:
        refuse(str(exc))
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import matrix
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        counts = matrix.region_matrix(val["-b"], val["-r"], k, n_docs, device)
        text = matrix.format_matrix(matrix.jaccard(counts) if "-j" in val else counts, labels)

        def write(tmp):
            with open(tmp, "w") as fh:
                fh.write(text)
        _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), the sweep's own IndexError
    # (index.check), a record that is not there.  Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
