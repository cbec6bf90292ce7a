"""`memo nearest`: which genome of a membership index the pivot matches longest, bin by bin or as intervals.

The first question of a user with a new assembly and a pangenome: which genome is the pivot closest to, and where along the pivot
does that change -- haplotype painting.  `memo tracks` cannot answer it: presence at one k saturates, and every near-identical genome
looks the same.  Here every position goes to the genomes whose match with the pivot is the longest there (every tied genome wins;
-u: only a genome that wins alone), counted per genome in `memo view`'s bins, with a row `none` for the positions where no genome
reaches -l and a row `best` for the sum (-f: the mean) of the longest match; or with -i one interval per maximal run of equal winner,
ties to the lowest annot.  No -k, and no -m: the index must be a membership index.  Counted on the GPU where the lengths of `memo
lengths` lie (memo_amd/nearest.py, memo_amd/csrc/memo_nearest.hip).  One GPU.
"""
from . import _cli

N_MIN, N_MAX = 2, 2048
CAP_MAX = 2 ** 31 - 1

USAGE = """
MEMO nearest - which genome matches the pivot longest, per bin or as intervals (haplotype painting)
Usage: ./memo nearest [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (nothing in the file can tell: on a conservation index the numbers
                         mean nothing)
  -n [INT]               total number of documents in pangenome (include the pivot), 2 to 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: tab-separated; a header of bins (START-END), a row `none` (no genome reaches -l),
                         one row per genome 1 .. N-1 (the positions of the bin where it matches the pivot longest; every
                         tied genome counts) and a last row `best` (the sum of the longest match over the bin)
  -B [INT]               number of genomic bins, those of memo view and memo tracks [500]
  -l [INT]               the shortest longest-match that counts as a win; below it the position goes to `none` [1]
  -K [INT]               cap: no match is longer, genomes at the cap tie [2147483647]
  -s [LIST]              candidate genomes, as memo merge -s writes them (1-3,7,5); the others get empty rows [all]
  -u                     count a position only for a genome that wins it alone
  -f                     divide by the bin's width: the share of the bin a genome wins, `best` as the mean
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): label genomes by file name
  -i                     intervals instead of the table: one CHR START END GENOME line per maximal run of equal winner
                         (ties go to the lowest annot, `.` where no genome reaches -l); not with -B, -u or -f

"""


cli = _cli.Cli("nearest", USAGE, "b:n:r:o:B:l:K:s:ufg:i")
refuse, read_labels = cli.refuse, cli.read_labels


def main(argv):
    """bin/memo nearest [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-n", "-r", "-o"))
    cli.one_gpu_only()
    intervals = "-i" in val
    for flag in ("-B", "-u", "-f"):
        if intervals and flag in val:
            refuse(f"{flag} has no meaning with -i: the intervals are runs of the winner, not bins")
    n_docs = cli.integer("-n", val["-n"], N_MIN, N_MAX, f"[{N_MIN}, {N_MAX}]")
    cap = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    min_len = cli.integer("-l", val.get("-l", "1"), 1, cap, f"[1, {cap}]")
    n_bins = cli.integer("-B", val.get("-B", "500"), 1, CAP_MAX, "[1, the positions of the window]")
    from .merge import parse_selection
    try:
        candidates = parse_selection(val["-s"], n_docs) if "-s" in val else None
    except ValueError as exc:
        refuse(f"-s: {exc}")
    labels = read_labels(val["-g"], n_docs) if "-g" in val else None
    from . import nearest, tracks
    from ._window import parse_region
    how = dict(candidates=candidates, min_len=min_len, cap=cap, device=_cli.device())

    def run_intervals():
        starts, winners, qs, qe = nearest.region_winners(val["-b"], val["-r"], n_docs, **how)
        _cli.write_text(val["-o"], nearest.format_intervals(parse_region(val["-r"])[0], qs, qe, starts, winners, labels))

    def run_table():
        wins, sums, edges, qs = nearest.region_nearest(val["-b"], val["-r"], n_docs, n_bins, **how)
        if wins.shape[2] == 0:                              # an empty window: an empty file
            return _cli.write_text(val["-o"], "")
        wins = wins[1 if "-u" in val else 0]
        if "-f" in val:
            wins, sums = tracks.fractions(wins, edges), tracks.fractions(sums[None, :], edges)[0]
        _cli.write_text(val["-o"], nearest.format_nearest(wins, sums, qs, edges, labels))
    cli.guarded(run_intervals if intervals else run_table)
