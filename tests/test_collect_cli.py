"""`memo collect` without a GPU: the command line (usage bytes, getopts handling, what is refused before the library is even
loaded), the host half of memo_amd/collect.py (the orders, the text of the curves) against literals, and the oracle of the GPU
tests (tests/collect_oracle.py) against the numbers worked out by hand on the README example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import collect_oracle
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def test_usage_bytes():
    from memo_amd import collect_cli
    usage = _fixture("memo_collect_usage.txt")
    assert usage == collect_cli.USAGE.encode() and usage.startswith(b"\nMEMO collect - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("collect", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-k [INT]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-p [INT]", b"-s [INT]", b"  -a  ", b"-g [FILE]"):
        assert flag in usage
    assert b"MEMBERSHIP" in usage and b"conservation index" in usage          # the index must be a membership index: said here


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_collect_usage.txt")
    r = _memo("collect", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("collect", "-n", "5", "-p")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- p\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"collect" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README
    r = _memo("query")
    assert r.returncode == 0 and r.stdout == _fixture("memo_query_usage.txt")


def _genome_list(tmp_path, lines):
    path = tmp_path / "genomes.txt"
    path.write_text("".join(ln + "\n" for ln in lines))
    return str(path)


def test_refusals_before_the_library_is_touched(tmp_path):
    """(-b names no file and the library path names none: a refusal that came later would be another message)"""
    out = str(tmp_path / "never.tsv")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-k", "3", "-o", out)
    four = _genome_list(tmp_path, ["a.fa", "", "b.fa", "c.fa", "  ", "d.fa"])
    for extra, env, message in ((("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-n", "five"), None, b"invalid literal for int()"),
                                (("-n", "5", "-k", "3.5"), None, b"invalid literal for int()"),
                                (("-n", "5", "-p", "many"), None, b"invalid literal for int()"),
                                (("-n", "5", "-p", "3", "-s", "0x1"), None, b"invalid literal for int()"),
                                (("-n", "5", "-p", "-1"), None, b"cannot be negative"),
                                (("-n", "5", "-g", four), None, b"names 4 genomes, -n says 5"),
                                (("-n", "5", "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                                (("-n", "4", "-g", four, "-p", "3"), None, b"a band over random orders")):
        r = _memo("collect", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - collect\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo collect: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same commands with nothing to refuse do reach the library, which is not there
    for extra in (("-n", "4", "-g", four), ("-n", "4", "-g", four, "-p", "3", "-a")):
        r = _memo("collect", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo collect: " in r.stderr


def test_missing_flags_are_named():
    r = _memo("collect", "-b", "x.parquet", "-k", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - collect\n" and r.stderr == b"memo collect: -r, -n, -o required\n"
    r = _memo("collect", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-p", "2")
    assert r.returncode == 2 and r.stderr == b"memo collect: -b required\n"


def test_one_genome_writes_the_pivot_row_and_needs_no_library(tmp_path):
    """N = 1: no order has a step, no kernel is called -- not even the library is loaded"""
    out = str(tmp_path / "one.tsv")
    r = _memo("collect", "-b", str(tmp_path / "no.parquet"), "-r", "ref_1:3-20", "-k", "3", "-n", "1", "-o", out)
    assert (r.returncode, r.stderr) == (0, b"")
    assert open(out).read() == "genomes\tcore\tcovered\n1\t17\t0\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import collect
    assert memo_amd.region_curves is collect.region_curves and memo_amd.collect is collect


def test_orders():
    from memo_amd import collect
    for n in (1, 2, 5, 40):
        first = collect.orders(n, 0, 7)
        assert first.dtype == np.uint16 and first.shape == (1, n - 1) and first[0].tolist() == list(range(1, n))
        for perms in (1, 3, 17):
            rows = collect.orders(n, perms, 11)
            assert rows.dtype == np.uint16 and rows.shape == (perms, n - 1)
            assert all(sorted(r.tolist()) == list(range(1, n)) for r in rows)               # every row a permutation of 1 .. N - 1
            assert np.array_equal(rows, collect.orders(n, perms, 11))                           # equal for equal seeds
            rng = np.random.default_rng(11)                                                     # drawn in sequence from one generator
            assert np.array_equal(rows, np.array([rng.permutation(n - 1) + 1 for _ in range(perms)]).reshape(perms, n - 1))
            assert np.array_equal(rows[:1], collect.orders(n, 1, 11))
    assert not np.array_equal(collect.orders(40, 3, 1), collect.orders(40, 3, 2))
    assert len({tuple(r) for r in collect.orders(40, 8, 1).tolist()}) == 8
    for bad in ((0, 0), (65536, 0), (5, -1)):
        with pytest.raises(ValueError):
            collect.orders(*bad)


def test_format_curves_against_literals():
    from memo_amd import collect
    core = np.array([[10, 8, 8], [18, 2 ** 32 + 7, 7]], np.uint64)
    covered = np.array([[10, 18, 20], [18, 2 ** 33, 2 ** 33 + 1]], np.uint64)
    orders = [[1, 2, 3], [3, 1, 2]]
    labels = ["pivot", "g1", "g2", "g3"]
    assert collect.format_curves(20, core, covered) == "genomes\tcore\tcovered\n1\t20\t0\n2\t10\t10\n3\t8\t18\n4\t8\t20\n"
    assert collect.format_curves(20, core[1:], covered[1:], "curve", orders[1:], labels) == (
        "genomes\tcore\tcovered\tadded\n1\t20\t0\tpivot\n2\t18\t18\tg3\n3\t4294967303\t8589934592\tg1\n4\t7\t8589934593\tg2\n")
    assert collect.format_curves(20, core, covered, "band") == (
        "genomes\tcore_min\tcore_mean\tcore_max\tcovered_min\tcovered_mean\tcovered_max\n"
        "1\t20\t20.0\t20\t0\t0.0\t0\n"
        "2\t10\t14.0\t18\t10\t14.0\t18\n"
        "3\t8\t2147483655.5\t4294967303\t18\t4294967305.0\t8589934592\n"
        "4\t7\t7.5\t8\t20\t4294967306.5\t8589934593\n")
    third = collect.format_curves(3, np.array([[1], [2], [2]], np.uint64), np.array([[1], [2], [3]], np.uint64), "band")
    assert third.splitlines()[2] == "2\t1\t1.6666666666666667\t2\t1\t2.0\t3"                  # means by repr(float(sum / P))
    assert collect.format_curves(20, core, covered, "long") == (
        "order\tgenomes\tcore\tcovered\n"
        "0\t1\t20\t0\n0\t2\t10\t10\n0\t3\t8\t18\n0\t4\t8\t20\n"
        "1\t1\t20\t0\n1\t2\t18\t18\n1\t3\t4294967303\t8589934592\n1\t4\t7\t8589934593\n")
    assert collect.format_curves(20, core, covered, "long", orders, labels).splitlines()[4:7] == [
        "0\t4\t8\t20\tg3", "1\t1\t20\t0\tpivot", "1\t2\t18\t18\tg3"]
    empty = np.zeros((1, 0), np.uint64)                                                       # N = 1: the pivot row alone
    assert collect.format_curves(0, empty, empty) == "genomes\tcore\tcovered\n1\t0\t0\n"
    assert collect.format_curves(5, empty, empty, "curve", np.zeros((1, 0), np.uint16), ["p"]) == "genomes\tcore\tcovered\tadded\n1\t5\t0\tp\n"
    for bad in (lambda: collect.format_curves(20, core, covered[:1]), lambda: collect.format_curves(20, core, covered, "band", orders, labels),
                lambda: collect.format_curves(20, core, covered, "curve", None, labels), lambda: collect.format_curves(20, core, covered, "wide")):
        with pytest.raises(ValueError):
            bad()


def test_the_oracle_on_the_example_by_hand():
    """ref_1:0-20 of the README example, k = 3, N = 5: the numbers of DESIGN.md 10.6"""
    from oracle import memo_oracle
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "ex_memb_k3_0_20")
    assert (c["index"], c["region"], c["k"], c["n"]) == ("example_memb.parquet", "ref_1:0-20", 3, 5)
    s, e, o = G.index_columns(c["index"], "ref_1")
    bits = memo_oracle.np_membership(*memo_oracle.filter_rows(s, e, o, 0, 20, 3), 0, 20, 3, 5)
    B = collect_oracle.unpack(bits, 5)
    assert np.array_equal(B, G.expected_matrix(c, G.load(c)))
    assert B.sum(0).tolist() == [20, 10, 16, 20, 18]                                          # the genomes' own counts
    core, covered = collect_oracle.curves(B, [[1, 2, 3, 4], [4, 3, 2, 1]])
    assert core.tolist() == [[10, 8, 8, 8], [18, 18, 16, 8]]
    assert covered.tolist() == [[10, 18, 20, 20], [18, 20, 20, 20]]
    from memo_amd import collect
    assert collect.format_curves(20, core[:1], covered[:1]) == "genomes\tcore\tcovered\n1\t20\t0\n2\t10\t10\n3\t8\t18\n4\t8\t20\n5\t8\t20\n"


def test_the_oracle_on_hand_made_bits():
    B = np.array([[1, 1, 0], [1, 0, 1], [1, 1, 1], [1, 0, 0]], np.uint8)
    core, covered = collect_oracle.curves(B, [[1, 2], [2, 2], [0, 1], [1, 1]])
    assert core.tolist() == [[2, 1], [2, 2], [4, 2], [2, 2]] and covered.tolist() == [[2, 3], [2, 2], [4, 4], [2, 2]]
    assert core.dtype == np.int64 and collect_oracle.curves(B, np.zeros((2, 0), np.int64))[0].shape == (2, 0)
    rows = np.array([[0b101], [0b110]], np.uint32)
    assert collect_oracle.unpack(rows, 3).tolist() == [[1, 0, 1], [0, 1, 1]]
