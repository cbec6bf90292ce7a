"""`memo collect`: how the core and the covered k-mers of a pivot genome region change as genomes are added (the collector's curve).

`memo query`'s flags (-b -k -n -r -o) with another product: instead of one membership line per position, one line per number of
genomes -- core = the positions whose k-mer is in every genome added so far, covered = those whose k-mer is in at least one of
them -- for the index order 1 .. N - 1, or with -p over random orders, as a band (minimum, mean, maximum) or with -a order by
order.  The window is swept as `memo query -m` sweeps it, in slices, each slice is reduced where it lies (memo_amd/collect.py,
memo_amd/csrc/memo_collect.hip), and only the curves leave the device.  One GPU.
"""
import getopt
import os
import sys

from .matrix_cli import label_of

USAGE = """
MEMO collect - core and covered k-mers of a pivot genome region as genomes are added (collector's curve)
Usage: ./memo collect [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: tab-separated, a header line, then one line per number of genomes (the pivot alone first)
  -p [INT]               random orders of the genomes instead of the index order: minimum, mean and maximum over them [0]
  -s [INT]               seed of the random orders [0]
  -a                     with -p: every order in turn instead of the band over them
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): name the genome each line adds (not with a band)

"""


def usage():
    sys.stdout.write(USAGE)
    sys.exit(0)


def refuse(message, status=1):
    sys.stderr.write(f"memo collect: {message}\n")
    sys.exit(status)


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
    """bin/memo collect [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    if not argv or argv[0] == "-h":
        usage()
    try:
        opts, _ = getopt.getopt(argv, "b:k:n:r:o:p:s:ag:")
    except getopt.GetoptError as exc:
        what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
        sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
        usage()
    val = {"-k": "31", "-p": "0", "-s": "0"}
    for o, a in opts:
        val[o] = a
    print("MEMO - collect", flush=True)
    # everything that can be refused is refused before the device is touched
    missing = [f for f in ("-b", "-r", "-n", "-o") if val.get(f, "") == ""]
    if missing:
        refuse(f"{', '.join(missing)} required", 2)
    if int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or os.environ.get("MEMO_FORCE_SHARDED"):
        refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")
    try:
        n_docs, k, perms, seed = int(val["-n"]), int(val["-k"]), int(val["-p"]), int(val["-s"])
    except ValueError as exc:
        refuse(str(exc))
    if perms < 0:
        refuse(f"-p {perms}: the number of random orders cannot be negative")
    form = "curve" if perms == 0 else "long" if "-a" in val else "band"
    if "-g" in val and form == "band":
        refuse("-g names the genome a line adds: a band over random orders (-p without -a) has none")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import collect
    from ._lib import MemoError
    from .view_cli import _replace_into
    try:
        device = int(os.environ.get("MEMO_DEVICE", "0"))   # as `memo query` chooses its GPU
        _, qs, qe = collect.parse_region(val["-r"])
        order_rows = collect.orders(n_docs, perms, seed)
        core, covered = collect.region_curves(val["-b"], val["-r"], k, n_docs, order_rows, device)
        text = collect.format_curves(qe - qs, core, covered, form, order_rows, labels)

        def write(tmp):
            with open(tmp, "w") as fh:
                fh.write(text)
        _replace_into(val["-o"], write)
    # a window or a Parquet file that is refused (pyarrow's errors are ValueErrors and OSErrors), the sweep's own IndexError
    # (index.check), a record that is not there.  Anything else is a defect and leaves as a traceback, as from `memo query`.
    except (MemoError, OSError, LookupError, ValueError) as exc:
        refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))
