"""`memo tracks`: which genome holds how much of every stretch of a pivot genome region.

`memo query`'s flags (-b -k -n -r -o) with another product: instead of one membership line per position, one row per genome and
one column per bin along the window -- the positions of the bin at which the genome holds the pivot's k-mer, or with -f their
share of the bin.  The bins are `memo view`'s (-B of them, its linspace rule), so this is the per-genome picture beside its
folded one: the presence/absence heat map of a pangenome browser.  The window is swept as `memo query -m` sweeps it, in slices,
each slice is counted where it lies (memo_amd/tracks.py, memo_amd/csrc/memo_tracks.hip), and only the table leaves the device.
What `-o` is called decides what is written, as for `memo view`: a name ending in `.tsv` gets the table, any other name a
matplotlib plot.  One GPU.
"""
import os

from . import _cli

USAGE = """
MEMO tracks - per-genome k-mer presence along a pivot genome region, in bins
Usage: ./memo tracks [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot)
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output plot.png: genomes down, bins across, the share of each bin's k-mers a genome holds
  -o [FILE].tsv          write the table instead: a header of bins (START-END), then one row per genome, genome 0 (the pivot) first
  -B [INT]               number of genomic bins, those of memo view [500]
  -f                     write fractions of the bin instead of counts (the plot always shows fractions)
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): label rows by file name
  -d [INT]               plot DPI [600]

"""


cli = _cli.Cli("tracks", USAGE, "b:k:n:r:o:B:fg:d:", {"-k": "31", "-B": "500", "-d": "600"})
refuse, read_labels = cli.refuse, cli.read_labels


def render(share, qs, edges, path, labels=None, dpi=600):
    """the heat map: genomes down, bins across, view_cli's LOW to HIGH over 0 .. 1; raises ImportError where matplotlib is missing"""
    import matplotlib
    import numpy as np
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.colors import LinearSegmentedColormap, Normalize
    from matplotlib.figure import Figure
    from .view_cli import HIGH, LOW
    share = np.asarray(share, np.float64)
    n_docs, n_bins = share.shape
    with matplotlib.rc_context({"font.size": 18, "font.family": "sans-serif"}):
        fig = Figure(figsize=(20, max(4.0, 0.25 * n_docs + 2.0)), dpi=dpi)
        canvas = FigureCanvasAgg(fig)
        ax = fig.add_subplot()
        image = ax.imshow(share, aspect="auto", interpolation="nearest", norm=Normalize(0, 1),
                          cmap=LinearSegmentedColormap.from_list("memo", [LOW, HIGH]),
                          extent=(-0.5, n_bins - 0.5, n_docs - 0.5, -0.5))
        ax.set_title("K-mer Membership")
        ax.set_xlabel(f"Genomic bin (n ={n_bins}), {int(qs) + int(edges[0])}-{int(qs) + int(edges[-1])}")
        ax.set_ylabel("Genome")
        if labels is not None:
            ax.set_yticks(np.arange(n_docs), labels=list(labels))
        fig.colorbar(image, ax=ax, label="Proportion of\nk-mers held", pad=0.01)
        fig.tight_layout()
        ext = os.path.splitext(path)[1][1:].lower()
        fmt = ext if ext in canvas.get_supported_filetypes() else "png"
        _cli.replace_into(path, lambda tmp: fig.savefig(tmp, format=fmt, dpi=dpi))


def main(argv):
    """bin/memo tracks [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    n_docs, k, n_bins, dpi = cli.integers(val, "-n", "-k", "-B", "-d")
    if n_bins < 1:
        refuse(f"-B {n_bins}: the number of bins must be at least 1")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    as_table = val["-o"].lower().endswith(".tsv")
    if not as_table:
        try:
            import matplotlib  # noqa: F401  (before the device is touched)
        except ImportError:
            refuse("matplotlib is not installed, so no plot can be drawn -- name the output FILE.tsv (-o) to get the table instead")
    from . import tracks

    def run():
        result = tracks.region_tracks(val["-b"], val["-r"], k, n_docs, n_bins, _cli.device())
        (counts, edges), qs = result, result.qs
        if counts.shape[1] == 0:                           # an empty window: an empty file
            _cli.write_text(val["-o"], "")
        elif as_table:
            _cli.write_text(val["-o"], tracks.format_tracks(tracks.fractions(counts, edges) if "-f" in val else counts, qs, edges, labels))
        else:
            render(tracks.fractions(counts, edges), qs, edges, val["-o"], labels, dpi)
    cli.guarded(run)
