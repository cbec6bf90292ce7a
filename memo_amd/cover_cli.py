"""`memo cover`: which genomes cover a pivot genome region's matches, in which order, at every k (`memo panel` without the -k).

`memo panel` chooses at one k-mer size, which the user has to guess and on which the order depends; this sums panel's scores over
every k of [-l, -K] -- a genome counts with how LONG it matches the pivot at each position, not with whether it does at one k -- and
so needs none.  The flags are `memo panel`'s otherwise: the fewest genomes that together hold a given share (-f), the most
informative genomes to add to a panel that exists (-i), the order in which the core shrinks slowest (-O core).  The lengths are `memo
lengths`', turned into weights that stay on the device for the genomes -s and -i name, and every step is a stream over them
(memo_amd/cover.py, memo_amd/csrc/memo_cover.hip); only scores and sums leave the device.  One GPU.
"""
from . import _cli

N_MIN, N_MAX = 2, 2048
CAP_MAX = 2 ** 31 - 1
OBJECTIVES = ("covered", "core")

USAGE = """
MEMO cover - the genomes that cover a pivot genome region's matches at every k-mer size, chosen greedily (memo panel, k-free)
Usage: ./memo cover [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -n [INT]               total number of documents in pangenome (include the pivot), 2 to 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: tab-separated, a header line, the pivot alone, then one line per genome taken
                         (genomes core covered added: `memo collect -g`'s curve summed over every k of -l to -K)
  -l [INT]               KMIN: the smallest k that is counted [1]
  -K [INT]               KMAX: the largest k that is counted, the cap of the match lengths [2147483647]
                         (up to 65535 values of k, -K minus -l plus 1, are kept in 2 bytes per genome and position; more in 4)
  -O [covered|core]      what a step maximises: the k-mers newly covered, ties by the core kept, or the core kept, ties by the
                         k-mers newly covered; further ties go to the lowest annot [covered]
  -s [LIST]              the candidates: annots and ranges of annots as in 1-3,7,5 [every genome but the pivot]
  -i [LIST]              a panel that exists already: these genomes are taken first, in the order written [none]
  -m [INT]               stop after this many genomes beyond the pivot, those of -i included
  -f [FRACTION]          stop once this share of the region's k-mers of -l to -K is covered, 0 to 1; needs -K
                         (-f 0: the genomes of -i and no more)
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): name the genomes instead of numbering them

"""

cli = _cli.Cli("cover", USAGE, "b:n:r:o:l:K:O:s:i:m:f:g:k:", {"-O": "covered"})
refuse = cli.refuse


def main(argv):
    """bin/memo cover [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    if "-k" in val:
        refuse("there is no -k: every k of -l KMIN to -K KMAX is counted (`memo panel` takes one k)")
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    n_docs = cli.integer("-n", val["-n"], N_MIN, N_MAX, f"[{N_MIN}, {N_MAX}]")
    kmax = cli.integer("-K", val.get("-K", str(CAP_MAX)), 1, CAP_MAX, f"[1, {CAP_MAX}]")
    kmin = cli.integer("-l", val.get("-l", "1"), 1, kmax, f"[1, {kmax}]")
    if val["-O"] not in OBJECTIVES:
        refuse(f"-O must be one of {', '.join(OBJECTIVES)} (got {val['-O']!r})")
    most = cli.integer("-m", val["-m"], 0, N_MAX, f"[0, {N_MAX}]") if "-m" in val else None
    if "-f" in val and "-K" not in val:
        refuse("-f needs -K: against the default cap of 2147483647 no share is ever reached")
    from . import panel
    try:
        panel.plan(n_docs, val["-O"], val.get("-s"), val.get("-i"), most)
        if "-f" in val:
            panel.threshold(val["-f"], 0)
        panel.parse_region(val["-r"])
    except ValueError as exc:
        refuse(str(exc).replace("max_genomes = ", "-m ").replace("the fraction", "-f"))
    labels = cli.read_labels(val["-g"], n_docs) if "-g" in val else [str(g) for g in range(n_docs)]

    def run():
        from . import cover
        order, core, covered, L, span = cover.region_cover(val["-b"], val["-r"], n_docs, kmin, kmax, val["-O"], val.get("-s"), val.get("-i"), most, val.get("-f"),
                                                           _cli.device())
        _cli.write_text(val["-o"], cover.format_cover(L, span, order, core, covered, labels))
    cli.guarded(run)
