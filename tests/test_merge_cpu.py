"""`memo merge` without a GPU: the definition (tests/merge_oracle.py) on the example's golden indexes, the `-s` parser, the bookkeeping of
`-G`, and the command line: the usage bytes and every refusal, with the library pointed at a file that is not there -- no refusal may need
the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import convert_oracle, merge_oracle
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
MEMB = os.path.join(G.GOLD, "example_memb.parquet")
FASTA = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def memb():
    return G.index_columns("example_memb.parquet", "ref_1")


# ---------------------------------------------------------------------------------------
# the oracle's facts on the example
# ---------------------------------------------------------------------------------------
def test_the_example_is_in_canonical_form(memb):
    assert len(memb[0]) == 48 and int(memb[0].max()) == 26
    assert _same(convert_oracle.rows(*memb, 5, order=False), memb)


@pytest.mark.parametrize("chosen,members,conserved", (([1, 2, 3], 34, 38), ([3, 1], 26, 27), ([2], 8, 8), ([4, 3, 2, 1], 48, 56)))
def test_a_selection_of_the_example(memb, chosen, members, conserved):
    got = merge_oracle.rows([(*memb, 5, chosen)], 26, False)
    assert len(got[0]) == members and len(merge_oracle.rows([(*memb, 5, chosen)], 26, True)[0]) == conserved
    # the canonical rows whose annot is chosen, renumbered: neither the planes nor the matrix
    assert _same(got, merge_oracle.renumbered([(memb, 5, chosen)]))
    assert set(got[2].tolist()) == set(range(1, len(chosen) + 1))


def test_conservation_does_not_depend_on_the_order_and_reversing_twice_gives_the_index_back(memb):
    cons = G.index_columns("example_cons.parquet", "ref_1")
    assert _same(merge_oracle.rows([(*memb, 5, [4, 3, 2, 1])], 26, True), cons)
    assert _same(merge_oracle.rows([(*memb, 5, None)], 26, True), cons)
    back = merge_oracle.rows([(*memb, 5, [4, 3, 2, 1])], 26, False)
    assert not _same(back, memb)
    assert _same(merge_oracle.rows([(*back, 5, [4, 3, 2, 1])], 26, False), memb)


def test_the_example_split_in_two_and_merged_is_both_committed_indexes(memb):
    first, second = (merge_oracle.rows([(*memb, 5, chosen)], 26, False) for chosen in ([1, 2], [3, 4]))
    assert int(first[0].max()) == 26 and int(second[0].max()) == 26          # every sub-index still closes the record at start 26
    for order, name in ((False, "example_memb.parquet"), (True, "example_cons.parquet")):
        assert _same(merge_oracle.rows([(*first, 3, None), (*second, 3, None)], 26, order), G.index_columns(name, "ref_1")), order
    assert _same(merge_oracle.rows([(*first, 3, None), (*second, 3, None)], 26, False),
                 merge_oracle.renumbered([(first, 3, None), (second, 3, None)]))
    # the other order of the inputs is another membership index and the same conservation index
    swapped = merge_oracle.rows([(*second, 3, None), (*first, 3, None)], 26, False)
    assert _same(swapped, merge_oracle.rows([(*memb, 5, [3, 4, 1, 2])], 26, False)) and not _same(swapped, memb)


def test_index_rows_keeps_the_records_of_the_first_input(memb):
    index = {"ref_1": memb}
    names, *got = merge_oracle.index_rows([(index, 5, [1, 2, 3])], False)
    assert names == ["ref_1"] * 34 and _same(got, merge_oracle.rows([(*memb, 5, [1, 2, 3])], 26, False))
    assert merge_oracle.by_record(names, *got)["ref_1"][0].dtype == np.int64


# ---------------------------------------------------------------------------------------
# -s and -G
# ---------------------------------------------------------------------------------------
def test_the_selection_parser():
    from memo_amd import merge
    assert merge.parse_selection(None, 5) == [1, 2, 3, 4] and merge.parse_selection(None, 2) == [1]
    assert merge.parse_selection("1-3,7,5", 8) == [1, 2, 3, 7, 5]
    assert merge.parse_selection("4,3,2,1", 5) == [4, 3, 2, 1] and merge.parse_selection("2", 5) == [2]
    assert merge.parse_selection("3-3,1-2", 4) == [3, 1, 2] and merge.parse_selection("1-2047", 2048) == list(range(1, 2048))
    assert merge.parse_selection([3, 1], 5) == [3, 1] and merge.parse_selection(np.asarray([2, 4]), 5) == [2, 4]
    for text in ("", ",", "1,", ",1", "1,,2", "a", "1-", "-1", "1--2", "1-2-3", "3-1", "1 2", "1;2", "+1", "1.0", "0x2", "١"):
        with pytest.raises(ValueError, match="does not parse"):
            merge.parse_selection(text, 9)
    for text in ("0", "5", "1-5", "0-2", "4,9", "99999999999999999999", "1-99999999999"):
        with pytest.raises(ValueError, match=r"outside \[1, 4\]"):
            merge.parse_selection(text, 5)
    with pytest.raises(ValueError, match=r"outside \[1, 4\]"):
        merge.parse_selection([1, 5], 5)
    for text, twice in (("1,1", 1), ("1-3,2", 2), ("4,1-4", 4), ([2, 3, 2], 2)):
        with pytest.raises(ValueError, match=f"names annot {twice} twice"):
            merge.parse_selection(text, 5)


def test_the_plan_of_the_columns():
    from memo_amd import merge
    sizes, chosen, plane_of = merge._plan([5, 3, 4], ["3,1", None, "2"])
    assert sizes == [5, 3, 4] and chosen == [[3, 1], [1, 2], [2]]
    assert plane_of.dtype == np.int32 and plane_of.tolist() == [3, 1, 6, 7, 10]          # the pivots' planes 0, 5 and 8 are never named
    for sizes, selections, message in (([], [], "no input"), ([1], [None], "n_docs must be in"), ([2049], [None], "n_docs must be in"),
                                       ([2048] * 33, [[1]] * 33, "67584 genomes together: the limit is 65536"),
                                       ([5, 5], [[], []], "no genome is chosen"),
                                       ([2048, 3], [None, "1"], "2048 genomes are chosen: the limit is 2047")):
        with pytest.raises(ValueError, match=message):
            merge._plan(sizes, selections)
    assert len(merge._plan([2048] * 32, [[1]] * 32)[2]) == 32 and len(merge._plan([2048, 5], [None, []])[2]) == 2047


def test_the_genome_list_of_the_output(tmp_path):
    from memo_amd import merge
    first, second = tmp_path / "first.txt", tmp_path / "second.txt"
    first.write_text("pivot.fa\n\n  a.fa  \nb.fa\nc.fa\n\n")
    second.write_text("other/pivot.fa\nd.fa\ne.fa")
    lists = [merge.read_list(str(first), 4), merge.read_list(str(second), 3)]
    assert lists == [["pivot.fa", "a.fa", "b.fa", "c.fa"], ["other/pivot.fa", "d.fa", "e.fa"]]
    assert merge.merged_list(lists, [[3, 1], [2]]) == ["pivot.fa", "c.fa", "a.fa", "e.fa"]
    assert merge.merged_list(lists, [[1, 2, 3], [1, 2]]) == ["pivot.fa", "a.fa", "b.fa", "c.fa", "d.fa", "e.fa"]
    with pytest.raises(ValueError, match="names 4 genomes, -n says 5"):
        merge.read_list(str(first), 5)
    with pytest.raises(ValueError, match="cannot read the genome list"):
        merge.read_list(str(tmp_path / "no.txt"), 5)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def test_usage_bytes():
    from memo_amd import merge_cli
    usage = _fixture("memo_merge_usage.txt")
    assert usage == merge_cli.USAGE.encode() and usage.startswith(b"\nMEMO merge - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("merge", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-s [LIST]", b"-g [FILE]", b"-o [FILE]", b"-c [FILE]", b"-G [FILE]", b"-f [FILE]"):
        assert flag in usage
    r = _memo("merge", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("merge", "-b", "x", "-n")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- n\n")


def test_the_other_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"merge" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README
    assert _memo("convert").stdout == _fixture("memo_convert_usage.txt") and _memo("add").stdout == _fixture("memo_add_usage.txt")


def test_flags_out_of_place_are_status_two():
    for argv, message in ((("-o", "y", "-c", "z"), b"-b required"),
                          (("-n", "5", "-b", "x.parquet", "-o", "y"), b"-n before any -b"),
                          (("-s", "1", "-b", "x.parquet", "-n", "5", "-o", "y"), b"-s before any -b"),
                          (("-g", "l", "-b", "x.parquet", "-n", "5", "-o", "y"), b"-g before any -b"),
                          (("-b", "x.parquet", "-o", "y"), b"-n required for x.parquet"),
                          (("-b", "x.parquet", "-n", "5", "-b", "z.parquet", "-c", "y"), b"-n required for z.parquet"),
                          (("-b", "x.parquet", "-b", "z.parquet", "-n", "5", "-c", "y"), b"-n required for x.parquet"),
                          (("-b", "x.parquet", "-n", "5", "-n", "6", "-c", "y"), b"-n is given twice for x.parquet"),
                          (("-b", "x.parquet", "-n", "5", "-s", "1", "-s", "2", "-c", "y"), b"-s is given twice"),
                          (("-b", "x.parquet", "-n", "5"), b"-o or -c required"),
                          (("-b", "x.parquet", "-n", "5", "-G", "list"), b"-o or -c required")):
        r = _memo("merge", *argv)
        assert r.returncode == 2 and r.stdout == b"MEMO - merge\n", (argv, r.stderr)
        assert r.stderr.startswith(b"memo merge: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (argv, r.stderr)


def _write(path, f0, s, e, a):
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table({"f0": pa.array(f0, pa.utf8()), "f1": pa.array(s, pa.int64()), "f2": pa.array(e, pa.int64()),
                             "f3": pa.array(a, pa.int64())}), path)


def test_refusals_before_the_library_is_touched_and_before_anything_is_written(tmp_path, memb):
    out, cons, listed = str(tmp_path / "never.parquet"), str(tmp_path / "never_cons.parquet"), str(tmp_path / "never.txt")

    def text(name, *lines):
        path = str(tmp_path / name)
        open(path, "w").write("".join(line + "\n" for line in lines))
        return path
    five, three, four = text("five.txt", *FASTA), text("three.txt", *FASTA[:3]), text("four.txt", *FASTA[:4])
    fai, short_fai, other_fai = text("p.fai", "ref_1\t30\t7\t30\t31"), text("short.fai", "ref_1\t25\t7\t25\t26"), text("other.fai", "chr9\t30\t7\t30\t31")
    s, e, a = memb
    copy, small, renamed, more, shorter = (str(tmp_path / name) for name in ("copy.parquet", "small.parquet", "renamed.parquet", "more.parquet", "shorter.parquet"))
    with open(copy, "wb") as fh:
        fh.write(open(MEMB, "rb").read())
    first = merge_oracle.rows([(s, e, a, 5, [1, 2])], 26, False)
    _write(small, ["ref_1"] * len(first[0]), *first)                                   # three genomes, the same pivot
    _write(renamed, ["chr9"] * len(first[0]), *first)
    _write(more, ["ref_1"] * len(first[0]) + ["ref_2"], *(np.append(c, v) for c, v in zip(first, (4, 8, 1))))
    keep = first[0] < 26
    _write(shorter, ["ref_1"] * int(keep.sum()), *(c[keep] for c in first))             # the same record, its largest row start below 26
    far, long = str(tmp_path / "far.parquet"), str(tmp_path / "long.parquet")
    _write(far, ["ref_1", "ref_1"], [5, 2 ** 31], [9, 2 ** 31 + 4], [1, 1])
    _write(long, ["ref_1", "ref_1"], [5, 2 ** 30], [9, 2 ** 30 + 4], [1, 1])
    before = sorted(os.listdir(tmp_path))
    A, B, outs = ("-b", MEMB, "-n", "5"), ("-b", small, "-n", "3"), ("-o", out, "-c", cons)
    ok = (*A, "-s", "1-3", *B, *outs)
    for argv, env, message in ((ok, {"WORLD_SIZE": "2"}, b"sharded launch"),
                               (ok, {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                               ((*A[:3], "five", *outs), None, b"invalid literal for int()"),
                               ((*A[:3], "1", *outs), None, b"-n must be in [2, 2048] (got 1 for "),
                               ((*A, *B[:3], "2049", *outs), None, b"-n must be in [2, 2048] (got 2049 for "),
                               # everything convert.scan_index refuses, for every input
                               ((*A[:3], "4", *outs), None, b"has annot 4 outside [1, 3]"),
                               ((*B, *A[:3], "4", "-c", cons), None, b"-n value is probably wrong"),
                               ((*B, "-b", os.path.join(G.GOLD, "rnd_negoverlap.parquet"), "-n", "12", *outs), None, b"ends before it starts"),
                               (("-b", far, "-n", "2", *outs), None, b"above 2^31 - 1"),
                               ((*A, "-b", long, "-n", "2", "-o", out), None, b"above 2^30 - 1"),
                               ((*A, "-b", str(tmp_path / "no.parquet"), "-n", "3", *outs), None, b"no.parquet"),
                               ((*A, *outs, "-f", short_fai), None, b"the length 25 of 'ref_1' is below its largest row start 26"),
                               ((*A, *outs, "-f", other_fai), None, b"is not in " + other_fai.encode()),
                               ((*A, *outs, "-f", str(tmp_path / "no.fai")), None, b"no.fai"),
                               # the genomes
                               ((*A, "-s", "", *outs), None, b"does not parse"),
                               ((*A, "-s", "1-3,x", *outs), None, b"does not parse at 'x'"),
                               ((*A, *B, "-s", "2-1", *outs), None, b"a range runs upwards"),
                               ((*A, "-s", "0", *outs), None, b"names annot 0, outside [1, 4]"),
                               ((*A, "-s", "1-5", *outs), None, b"names annot 5, outside [1, 4]"),
                               ((*A, *B, "-s", "3", "-o", out), None, b"names annot 3, outside [1, 2]"),
                               ((*A, "-s", "2,1-3", *outs), None, b"names annot 2 twice"),
                               ((*A, *A, *outs), None, MEMB.encode() + b" is given as two inputs"),
                               ((*A, "-b", os.path.join(G.GOLD, ".", "example_memb.parquet"), "-n", "5", *outs), None, b"is given as two inputs"),
                               # the pivot
                               ((*A, "-b", renamed, "-n", "3", *outs), None, b"record 'ref_1' of " + MEMB.encode() + b" has no rows in " + renamed.encode()),
                               (("-b", renamed, "-n", "3", *A, *outs), None, b"is this the same pivot?"),
                               ((*A, "-b", more, "-n", "3", *outs), None, b"record 'ref_2' of " + more.encode() + b" has no rows in " + MEMB.encode()),
                               ((*A, "-b", shorter, "-n", "3", *outs), None, b"record 'ref_1' has 26 positions in " + MEMB.encode()),
                               ((*A, "-b", shorter, "-n", "3", "-c", cons), None, b"is this the same pivot?"),
                               # the outputs
                               (("-b", copy, "-n", "5", *B, "-o", copy), None, b"copy.parquet is an input file"),
                               ((*B, "-b", copy, "-n", "5", "-c", os.path.join(str(tmp_path), ".", "copy.parquet")), None, b"is an input file"),
                               ((*A, "-o", out, "-c", out), None, b"is named for two outputs"),
                               ((*A, "-o", out, "-c", os.path.join(str(tmp_path), ".", "never.parquet")), None, b"is named for two outputs"),
                               ((*A, "-g", five, *outs, "-G", out), None, b"is named for two outputs"),
                               ((*A, "-g", five, *outs, "-G", five), None, b"five.txt is an input file"),
                               # the lists
                               ((*A, "-g", five, *B, *outs, "-G", listed), None, b"-G needs the genome list (-g) of every input"),
                               ((*A, *outs, "-G", listed), None, b"-G needs the genome list"),
                               ((*A, "-g", four, *outs), None, b"four.txt names 4 genomes, -n says 5"),
                               ((*A, "-g", five, *B, "-g", four, *outs, "-G", listed), None, b"four.txt names 4 genomes, -n says 3"),
                               ((*A, "-g", str(tmp_path / "no.txt"), *outs), None, b"cannot read the genome list"),
                               # the settings
                               (ok, {"MEMO_MERGE_SLICE": "0"}, b"MEMO_MERGE_SLICE must be"),
                               (ok, {"MEMO_MERGE_BATCH": "many"}, b"MEMO_MERGE_BATCH must be")):
        r = _memo("merge", *argv, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - merge\n", (argv, env, r.stderr)
        assert r.stderr.startswith(b"memo merge: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (argv, env, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (argv, env)
    assert open(copy, "rb").read() == open(MEMB, "rb").read()
    # the same command with nothing to refuse does reach the library, which is not there
    for argv in (ok, (*A, "-o", out), (*A, "-s", "4,3,2,1", "-c", cons), (*A, "-g", five, *B, "-g", three, *outs, "-G", listed), (*A, *outs, "-f", fai)):
        r = _memo("merge", *argv)
        assert r.returncode == 1 and (b"Traceback" in r.stderr or b"memo merge: " in r.stderr), (argv, r.stderr)
        assert b"must be" not in r.stderr and b"libmemo_amd.so" in r.stderr, (argv, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before


def test_too_many_genomes_are_refused_on_the_host():
    """more than 2047 chosen and more than 65 536 in all: through the function, which checks them before it opens a file"""
    from memo_amd import merge
    with pytest.raises(ValueError, match="2048 genomes are chosen: the limit is 2047"):
        merge.merge_index([("a.parquet", 2048, None), ("b.parquet", 3, "1")], out_path="o.parquet")
    with pytest.raises(ValueError, match="the limit is 65536"):
        merge.merge_index([(f"{i}.parquet", 2048, "1") for i in range(33)], out_path="o.parquet")
    with pytest.raises(ValueError, match="no genome is chosen"):
        merge.merge_index([("a.parquet", 5, [])], cons_path="o.parquet")


def test_the_library_functions_refuse_what_the_command_refuses(memb):
    from memo_amd import merge
    s, e, a = memb
    for bad, message in ((lambda: merge.rows([(s, e, a, 1, None)]), "n_docs must be in"), (lambda: merge.rows([(s, e, a, 2049, None)]), "n_docs must be in"),
                         (lambda: merge.rows([]), "no input"), (lambda: merge.rows([(s, e, a, 5, [])]), "no genome is chosen"),
                         (lambda: merge.rows([(s, e, a, 5, "1,1")]), "twice"), (lambda: merge.rows([(s, e, a, 5, [5])]), "outside"),
                         (lambda: merge.rows([(s, e, a, 4, None)]), "annot 4 outside"), (lambda: merge.rows([(s, s - 1, a, 5, None)]), "ends before it starts"),
                         (lambda: merge.rows([(s, e, a[:-1], 5, None)]), "differ in length"),
                         (lambda: merge.rows([(s, e, a, 5, None)], 25), "below its largest row start"),
                         (lambda: merge.rows([(s, e, a, 5, None), (s[s < 26], e[s < 26], a[s < 26], 5, None)]), "is this the same pivot"),
                         (lambda: merge.rows([(s, e, a, 5, None)], slice_positions=0), "slice_positions must be"),
                         (lambda: merge.rows([(s, e, a, 5, None)], batch_positions=-3), "batch_positions must be"),
                         (lambda: merge.dap(np.zeros(8, np.uint32), [0], 0, 4, 8), "planes must be"),
                         (lambda: merge.dap(np.zeros((0, 8), np.uint32), [0], 0, 4, 8), "the planes must be 1 to 65536"),
                         (lambda: merge.dap(np.zeros((3, 8), np.uint32), [], 0, 4, 8), "plane_of must name 1 to 2047 columns"),
                         (lambda: merge.dap(np.zeros((3, 8), np.uint32), [0] * 2048, 0, 4, 8), "plane_of must name 1 to 2047 columns"),
                         (lambda: merge.dap(np.zeros((3, 8), np.uint32), [2 ** 31], 0, 4, 8), "int32"),
                         (lambda: merge.dap(np.zeros((3, 8), np.uint32), [1], 0, 4, 8, pitch=4), "pitch is below"),
                         (lambda: merge.merge_index([("x.parquet", 5)]), "no output")):
        with pytest.raises(ValueError, match=message):
            bad()
    import memo_amd
    assert memo_amd.merge is merge and memo_amd.merge_index is merge.merge_index
