"""`memo merge`: the index of chosen genomes from one or more membership indexes on one pivot, without going back to the genomes.

A membership index still holds every genome's matching statistics (`memo lengths` reads them back, `memo convert` feeds them to the row
builder, `memo add` puts new columns beside them).  This chooses among them: a sub-cohort of one index (-s), its genomes in another
order, or the cohorts of several indexes on the same pivot together.  Every -b opens an input, and the -n, -s and -g that follow belong
to it; the output's genomes are annot 1, 2 ... in command order.  -o is the membership index of the chosen genomes in canonical form (the
form `memo convert -m` writes), -c their conservation index, from the same matrix in the same run (memo_amd/merge.py,
memo_amd/csrc/memo_merge.hip).  One GPU.
"""
from . import _cli

N_MAX = 2048

USAGE = """
MEMO merge - index of chosen genomes from membership indexes on one pivot
Usage: ./memo merge -b A -n NA [-s SEL] [-g LIST] [-b B -n NB [-s SEL] [-g LIST]] ... [options]

Per input (every -b opens one; the -n, -s and -g after it are its own):
  -b [FILE]              parquet membership MEMO index
  -n [INT]               total number of documents in that index (include the pivot), 2 to 2048
  -s [LIST]              that index's genomes to take, in this order: annots and ranges, as in 1-3,7,5 [all, ascending]
  -g [FILE]              the document list that index was built on (for -G)

Basic options:
  -o [FILE]              output file: the parquet membership MEMO index of the chosen genomes, in canonical form
  -c [FILE]              output file: the parquet conservation MEMO index of the chosen genomes
                         (at least one of -o and -c)
  -G [FILE]              output file: the document list of the output (needs -g for every input)
  -f [FILE]              .fai of the pivot: record lengths, where a record is longer than its largest row start

"""


cli = _cli.Cli("merge", USAGE, "b:n:s:g:o:c:G:f:")
refuse = cli.refuse


def inputs_of(opts):
    """[{-b, -n, -s, -g}, ...] in command order and the other flags; what is out of place is refused with status 2"""
    inputs, val = [], {}
    for o, a in opts:
        if o == "-b":
            inputs.append({"-b": a})
        elif o in ("-n", "-s", "-g"):
            if not inputs:
                refuse(f"{o} before any -b: every -b opens an input, and the -n, -s and -g after it are its own", 2)
            if o in inputs[-1]:
                refuse(f"{o} is given twice for {inputs[-1]['-b']}", 2)
            inputs[-1][o] = a
        else:
            val[o] = a
    return inputs, val


def main(argv):
    """bin/memo merge [options]: usage handling as the other sub-commands (getopts messages on stderr, then the usage, exit 0)"""
    opts = cli.options(argv)
    cli.banner()
    # everything that can be refused is refused before the device is touched and before anything is written
    inputs, val = inputs_of(opts)
    if not inputs or any(i["-b"] == "" for i in inputs):
        refuse("-b required", 2)
    for i in inputs:
        if i.get("-n", "") == "":
            refuse(f"-n required for {i['-b']}", 2)
    if val.get("-o", "") == "" and val.get("-c", "") == "":
        refuse("-o or -c required", 2)
    cli.one_gpu_only()
    sources = []
    for i in inputs:
        n_docs, = cli.integers(i, "-n")
        if not 2 <= n_docs <= N_MAX:
            refuse(f"-n must be in [2, {N_MAX}] (got {n_docs} for {i['-b']})")
        sources.append((i["-b"], n_docs, i.get("-s"), i.get("-g") or None))
    from . import merge
    cli.guarded(lambda: merge.merge_index(sources, out_path=val.get("-o") or None, cons_path=val.get("-c") or None,
                                          list_out=val.get("-G") or None, fai=val.get("-f"), device=_cli.device(), log=lambda line: None))
