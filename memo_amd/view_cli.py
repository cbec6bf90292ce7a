"""`memo view`: bin a conservation result and write the table, or plot it.

Front end of src/view.sh (:29-67: flags, usage, banner) and src/plot_conservation.py (:67-115: the plot), with one
extension: `-r CHR:START-END` (and `-k`) makes `-i` a Parquet conservation index, and the window goes from the sweep to
the histogram without the text file in between (memo_amd/view.py: preprocess_region).

What `-o` is called decides what is written: a name ending in `.tsv` gets the table itself (bin, No. Genomes, value: the
reference's melted DataFrame, floats by repr so that they read back bit for bit), any other name a plot.  plotnine is
not a dependency of this build: the plot is drawn with matplotlib (Agg) after plot_conservation.py:67-86 -- stacked bars
of width 1, the fill from #000000 to #c6dbef over 1 .. n_docs - 1, y from 0 to 1, the same title and labels, 20 x 4 in --
and is not byte-compatible with the reference's.
"""
import os
import sys

import numpy as np

from . import _cli

USAGE = """
MEMO query - query k-mer membership or conservation on pivot genome region
Usage: ./memo query [options]

Basic options:
  -i [FILE]              input conservation.out from MEMO conservation query
  -o [FILE]              output plot.png
  -n [INT]               total number of documents in pangenome (include the pivot)
  -b [INT]               number of genomic bins to visualize conservation [500]
  -d [INT]               plot DPI [600]

"""

# what follows the reference's bytes (which are view.sh's own, `MEMO query` heading included)
EXTENSION = """Beyond the reference, in this build of memo view:
  -r [CHR:START-END]     -i is a parquet conservation MEMO index: query this region and bin it on the GPU
  -k [INT]               k-mer size for -r [31]
  -o [FILE].tsv          write the table (bin, No. Genomes, value) instead of a plot

"""

TSV_HEADER = "bin\tNo. Genomes\tvalue\n"
LOW, HIGH, OUTSIDE = "#000000", "#c6dbef", "#7f7f7f"     # scale_fill_gradient(low, high); ggplot's na.value for what lies outside its limits


cli = _cli.Cli("view", USAGE + EXTENSION, "i:o:n:b:d:r:k:", {"-b": "500", "-d": "600", "-k": "31"},        # view.sh:9-10; query.sh:7
               banner="MEMO - plotting sequence conservation")


def write_tsv(table, path):
    """the table as text: one header line, rows in melt order, floats by repr"""
    def write(tmp):
        with open(tmp, "w") as fh:
            fh.write(TSV_HEADER)
            fh.write("".join(f"{int(b)}\t{float(g)!r}\t{float(v)!r}\n"
                             for b, g, v in zip(table["bin"], table["No. Genomes"], table["value"])))
    _cli.replace_into(path, write)


def fill_colours(n_docs):
    """per order 0 .. n_docs - 1: linear from LOW to HIGH over the scale's limits 1 .. n_docs - 1 (plot_conservation.py:81-82)"""
    from matplotlib.colors import to_rgb
    lo, hi = np.array(to_rgb(LOW)), np.array(to_rgb(HIGH))
    span = max(n_docs - 2, 1)
    return [to_rgb(OUTSIDE) if order < 1 else tuple(lo + (hi - lo) * min((order - 1) / span, 1.0)) for order in range(n_docs)]


def render(table, n_docs, n_bins, path, dpi=600):
    """plot_conservation.py:67-90 with matplotlib; raises ImportError where matplotlib is missing"""
    import matplotlib
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.cm import ScalarMappable
    from matplotlib.colors import LinearSegmentedColormap, Normalize
    from matplotlib.figure import Figure
    value = np.asarray(table["value"], np.float64).reshape(n_docs, n_bins)     # melt order: orders outermost
    with matplotlib.rc_context({"font.size": 18, "font.family": "sans-serif"}):
        fig = Figure(figsize=(20, 4), dpi=dpi)
        canvas = FigureCanvasAgg(fig)
        ax = fig.add_subplot()
        x, bottom, colours = np.arange(n_bins), np.zeros(n_bins), fill_colours(n_docs)
        for order in range(n_docs - 1, -1, -1):           # position = stack: the first level ends up on top
            ax.bar(x, value[order], width=1, bottom=bottom, color=colours[order], linewidth=0)
            bottom = bottom + value[order]
        ax.set_title("K-mer Conservation")
        ax.set_xlabel("Genomic bin (n =" + str(n_bins) + ")")
        ax.set_ylabel("Proportion of\nconserved k-mers")
        ax.set_ylim(0, 1)
        ax.set_yticks(np.linspace(0, 1, 5), labels=['0', '0.25', '0.50', '0.75', '1'])
        ax.set_xlim(-0.5, n_bins - 0.5)
        for side in ("top", "right"):
            ax.spines[side].set_visible(False)
        scale = ScalarMappable(Normalize(1, max(n_docs - 1, 2)), LinearSegmentedColormap.from_list("memo", [LOW, HIGH]))
        fig.colorbar(scale, ax=ax, label="No. Genomes", pad=0.01)
        fig.subplots_adjust(left=0.08, right=1.0, bottom=0.24, top=0.86)
        ext = os.path.splitext(path)[1][1:].lower()
        fmt = ext if ext in canvas.get_supported_filetypes() else "png"
        _cli.replace_into(path, lambda tmp: fig.savefig(tmp, format=fmt, dpi=dpi))


def main(argv):
    """bin/memo view [options]: usage handling of view.sh (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    missing = [f for f in ("-i", "-o", "-n") if val.get(f, "") == ""]
    if missing:                                           # (plot_conservation.py's argparse: required=True, status 2)
        sys.stderr.write(f"memo view: {', '.join(missing)} required\n")
        sys.exit(2)
    as_table = val["-o"].lower().endswith(".tsv")
    try:
        n_docs, n_bins, dpi, k = (int(val[f]) for f in ("-n", "-b", "-d", "-k"))
        if not as_table:
            try:
                import matplotlib  # noqa: F401  (before the device is touched)
            except ImportError:
                sys.stderr.write("memo view: matplotlib is not installed, so no plot can be drawn -- "
                                 "name the output FILE.tsv (-o) to get the table instead\n")
                sys.exit(1)
        from . import view
        from ._lib import MemoError
        try:
            device = _cli.device()
            if "-r" in val:
                table = view.preprocess_region(val["-i"], val["-r"], k, n_docs, n_bins, device)
            else:
                table = view.preprocess_data(val["-i"], n_docs, n_bins, device)
            if as_table:
                write_tsv(table, val["-o"])
            else:
                render(table, n_docs, n_bins, val["-o"], dpi)
        except (MemoError, OSError, LookupError) as exc:  # LookupError: the sweep's own IndexError (index.check), a record that is not there
            sys.stderr.write(f"memo view: {type(exc).__name__}: {exc}\n" if isinstance(exc, LookupError) else f"memo view: {exc}\n")
            sys.exit(1)
    # more bins than positions; text that is no integer; a window or a Parquet file that is refused (pyarrow's errors are ValueErrors
    # and OSErrors).  Anything else is a defect and leaves as a traceback, as it does from `memo query`.
    except (ZeroDivisionError, ValueError) as exc:
        sys.stderr.write(f"memo view: {exc}\n")
        sys.exit(1)
