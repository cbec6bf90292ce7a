"""`memo mosaic`: the pivot as the fewest pieces copied whole from the genomes of a membership index, as intervals or per bin.

Which haplotypes is the pivot made of, and where are the breakpoints?  `memo nearest -i` paints every position with its own winner,
which flips wherever two genomes' lengths cross; here the window is parsed greedily by longest match -- from the window's left end
the genome that matches longest is copied to the end of its match, then the question is asked again there -- and one CHR START END
GENOME line is written per piece (`.` where no genome reaches -l: consecutive such pieces are one line; two pieces of one genome
stay two lines).  The number of lines is a k-free distance of the pivot to the panel, the boundaries are the candidate recombination
breakpoints.  With -B the bases of every bin that lie inside pieces of each genome, in `memo view`'s bins, and a last row with the
pieces that start in the bin.  No -k, and no -m: the index must be a membership index.  Parsed on the GPU where the lengths of `memo
lengths` lie (memo_amd/mosaic.py, memo_amd/csrc/memo_mosaic.hip).  One GPU.
"""
from . import _cli

N_MIN, N_MAX = 2, 2048
CAP_MAX = 2 ** 31 - 1

USAGE = """
MEMO mosaic - the pivot as the fewest pieces copied whole from the genomes (greedy parse by longest match)
Usage: ./memo mosaic [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (nothing in the file can tell: on a conservation index the numbers
                         mean nothing)
  -n [INT]               total number of documents in pangenome (include the pivot), 2 to 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates); the parse starts at START
  -o [FILE]              output file: one CHR START END GENOME line (tab-separated) per piece, the genome the piece is
                         copied from (ties go to the lowest annot), `.` where no genome reaches -l
  -l [INT]               the shortest match that is copied; below it the position is a piece of one base of no genome [1]
  -K [INT]               cap: no match is longer, genomes at the cap tie [2147483647]
  -s [LIST]              candidate genomes, as memo merge -s writes them (1-3,7,5) [all]
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): label genomes by file name
  -B [INT]               a table instead of the intervals: per bin of memo view and memo tracks a row `none`, one row per
                         genome 1 .. N-1 (the bases of the bin inside its pieces) and a last row `phrases` (the pieces
                         that start in the bin)
  -f                     with -B: divide by the bin's width

"""


cli = _cli.Cli("mosaic", USAGE, "b:n:r:o:l:K:s:g:B:f")
refuse, read_labels = cli.refuse, cli.read_labels


def main(argv):
    """bin/memo mosaic [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-n", "-r", "-o"))
    cli.one_gpu_only()
    table = "-B" in val
    if "-f" in val and not table:
        refuse("-f has no meaning without -B: it divides the rows of the table by the bin's width")
    n_docs = cli.integer("-n", val["-n"], N_MIN, N_MAX, f"[{N_MIN}, {N_MAX}]")
    cap = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    min_len = cli.integer("-l", val.get("-l", "1"), 1, cap, f"[1, {cap}]")
    n_bins = cli.integer("-B", val["-B"], 1, CAP_MAX, "[1, the positions of the window]") if table else 0
    from .merge import parse_selection
    try:
        candidates = parse_selection(val["-s"], n_docs) if "-s" in val else None
    except ValueError as exc:
        refuse(f"-s: {exc}")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import mosaic, nearest, tracks
    from ._window import parse_region

    def run():
        record, qs, qe = parse_region(val["-r"])
        edges = tracks.region_edges(qe - qs, n_bins) if table and qe > qs else None     # (more bins than positions: refused here)
        starts, genomes, qs, qe = mosaic.region_mosaic(val["-b"], val["-r"], n_docs, candidates=candidates, min_len=min_len, cap=cap,
                                                       device=_cli.device())
        if qe == qs:                                          # an empty window: an empty file
            return _cli.write_text(val["-o"], "")
        if not table:
            return _cli.write_text(val["-o"], nearest.format_intervals(record, qs, qe, starts, genomes, labels))
        bases, lines = mosaic.bin_phrases(starts, genomes, qe - qs, edges, n_docs)
        if "-f" in val:
            bases, lines = tracks.fractions(bases, edges), tracks.fractions(lines[None, :], edges)[0]
        _cli.write_text(val["-o"], mosaic.format_mosaic(bases, lines, qs, edges, labels))
    cli.guarded(run)
