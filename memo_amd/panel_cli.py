"""`memo panel`: which genomes cover a pivot genome region, in which order (the greedy set cover behind the collector's curve).

`memo collect`'s flags (-b -k -n -r -o -g) with the order chosen and not given: the fewest genomes that together hold a given
share of the pivot's k-mers (-f), the most informative genomes to add to a panel that exists (-i), the order in which the core
shrinks slowest (-O core).  The window is swept as `memo query -m` sweeps it, in slices, the slices stay on the device as
per-genome bit planes, and every step is a stream over them (memo_amd/panel.py, memo_amd/csrc/memo_panel.hip); only scores and
counts leave the device.  One GPU.
"""
from . import _cli

USAGE = """
MEMO panel - the genomes that cover a pivot genome region, chosen greedily (which genomes give the collector's curve, in which order)
Usage: ./memo panel [options]

Basic options:
  -b [FILE]              parquet MEMBERSHIP MEMO index (on a conservation index the numbers mean nothing, and nothing can tell)
  -k [INT]               k-mer size [31]
  -n [INT]               total number of documents in pangenome (include the pivot), 2 to 2048
  -r [CHR:START-END]     query region (0-indexed, half open '[)' coordinates)
  -o [FILE]              output file: tab-separated, a header line, the pivot alone, then one line per genome taken
                         (genomes core covered added, as `memo collect -g` writes its curve)
  -O [covered|core]      what a step maximises: the k-mers newly covered, ties by the core kept, or the core kept, ties by the
                         k-mers newly covered; further ties go to the lowest annot [covered]
  -s [LIST]              the candidates: annots and ranges of annots as in 1-3,7,5 [every genome but the pivot]
  -i [LIST]              a panel that exists already: these genomes are taken first, in the order written [none]
  -m [INT]               stop after this many genomes beyond the pivot, those of -i included
  -f [FRACTION]          stop once this share of the region's k-mers is covered, 0 to 1 (-f 0: the genomes of -i and no more)
  -g [FILE]              the genome list `memo index -g` took (first line the pivot): name the genomes instead of numbering them

"""

cli = _cli.Cli("panel", USAGE, "b:k:n:r:o:O:s:i:m:f:g:", {"-k": "31", "-O": "covered"})
refuse = cli.refuse


def main(argv):
    """bin/memo panel [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    val = cli.parse(argv)
    # everything that can be refused is refused before the device is touched
    cli.require(val, ("-b", "-r", "-n", "-o"))
    cli.one_gpu_only()
    from . import panel
    n_docs = cli.integer("-n", val["-n"], panel.N_MIN, panel.N_MAX, f"[{panel.N_MIN}, {panel.N_MAX}]")
    k, = cli.integers(val, "-k")
    if val["-O"] not in panel.OBJECTIVES:
        refuse(f"-O must be one of {', '.join(panel.OBJECTIVES)} (got {val['-O']!r})")
    most = cli.integer("-m", val["-m"], 0, panel.N_MAX, f"[0, {panel.N_MAX}]") if "-m" in val else None
    try:
        panel.plan(n_docs, val["-O"], val.get("-s"), val.get("-i"), most)
        if "-f" in val:
            panel.threshold(val["-f"], 0)
        panel.parse_region(val["-r"])
    except ValueError as exc:
        refuse(str(exc).replace("max_genomes = ", "-m ").replace("the fraction", "-f"))
    labels = cli.read_labels(val["-g"], n_docs) if "-g" in val else None

    def run():
        order, core, covered, L = panel.region_panel(val["-b"], val["-r"], k, n_docs, val["-O"], val.get("-s"), val.get("-i"), most, val.get("-f"),
                                                     _cli.device())
        if labels is None:
            text = panel.format_panel(L, order, core, covered, [str(g) for g in range(n_docs)])
        else:
            text = panel.format_panel(L, order, core, covered, labels)
        _cli.write_text(val["-o"], text)
    cli.guarded(run)
