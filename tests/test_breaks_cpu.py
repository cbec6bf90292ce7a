"""`memo breaks` without a GPU: the two forms of the oracle (tests/breaks_oracle.py), the worked example of DESIGN.md 10.15 from the
goldens, the oracle's starts against a histogram of `memo mems`' list, the text writers, and the command line's refusals that never
reach the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import breaks_oracle as O
from tests import golden_util as G
from tests import lengths_oracle, mems_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
EDGES4 = np.array([0, 5, 10, 15, 20], np.int64)            # view.bin_edges(20, 4)

EXAMPLE_STARTS = [[1, 0, 0, 0], [3, 2, 2, 3], [2, 1, 2, 1], [2, 4, 2, 3], [3, 3, 3, 3]]
EXAMPLE_SUMS = [[13, 13, 14, 12], [18, 30, 14, 20], [21, 25, 17, 20], [15, 17, 16, 16]]           # genomes 1 .. 4
EXAMPLE_L3 = [[1, 0, 0, 0], [3, 1, 2, 2], [2, 1, 2, 1], [2, 4, 2, 3], [3, 3, 3, 3]]


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


# ---------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", (0, 1))
def test_the_two_forms_of_the_oracle_agree(halo):
    rng = np.random.default_rng(20261020 + halo)
    for planes, L, cap in ((1, 1, 4), (2, 2, 4), (3, 17, 4), (2, 64, 3), (1, 40, 1), (4, 33, 2 ** 31 - 1)):
        v = rng.integers(0, min(cap, 6) + 1, (planes, L + halo))
        n = L
        for first in (0, 7, 2 ** 33):
            for cuts in ([0, n], [0, n // 2, n], sorted([-5, 0, 0, 1, n - 1, n, n + 9]), sorted(rng.integers(0, n + 1, 6).tolist() + [0, n]),
                         list(range(n + 1))):
                edges = np.asarray(cuts, np.int64) + first
                for min_len in sorted({1, 2, min(cap, 6)}):
                    fast, slow = O.table(v, edges, cap, min_len, halo, first), O.naive(v, edges, cap, min_len, halo, first)
                    assert fast.dtype == np.uint64 and fast.shape == (2, planes, len(cuts) - 1) and np.array_equal(fast, slow)
                    assert np.array_equal(fast[1].sum(axis=1), v[:, halo:].sum(axis=1).astype(np.uint64))
                    if halo == 0 and min_len == 1 and L:
                        assert (fast[0].sum(axis=1) >= 1).all() or (v[:, 0] == 0).any()


def test_the_rule_branch_by_branch():
    """one hand-made plane per branch, cap = 4: rise, tie below the cap, tie at the cap, fall, below min_len, cell 0"""
    one = lambda v, **kw: O.table([v], [0, len(v) - kw.get("halo", 0)], 4, **kw)[0, 0, 0]     # noqa: E731
    assert one([0, 1, 2, 3, 4, 4, 4, 4]) == 4                       # rises; the run at the cap is the match that began at its first cell
    assert one([2, 2, 2, 2, 2, 2, 2, 2]) == 8                       # ties below the cap: every cell starts one
    assert one([4, 4, 4, 4, 4, 4, 4, 4]) == 1                       # a tie at the cap: only cell 0, position 0 of its record
    assert one([4, 4, 4, 4, 4, 4, 4, 4], halo=1) == 0               # ... and with a neighbour, none
    assert one([4, 3, 2, 1, 0, 0, 0, 0]) == 1                       # falls start nothing; zeros are below min_len = 1
    assert one([3, 2, 3, 2, 3, 2, 3, 2], min_len=3) == 4 and one([3, 2, 3, 2, 3, 2, 3, 2], min_len=2) == 4 and one([3, 2, 3, 2, 3, 2, 3, 2], min_len=4) == 0
    assert one([1, 1, 2, 2, 3, 3, 4, 4], min_len=2) == 5 and one([1, 1, 2, 2, 3, 3, 4, 4], min_len=2, halo=1) == 5
    assert one([0, 3, 0, 3, 0, 3, 0, 3], halo=1) == 4 and one([0, 3, 0, 3, 0, 3, 0, 3]) == 4
    assert O.table([[1, 2, 3, 4, 4, 4, 0, 9]], [0, 8], 4)[1, 0, 0] == 27            # the sum takes the cells as they are


def test_the_worked_example_from_the_goldens():
    """ref_1:0-20 of the example pair, N = 5, -B 4, the default cap: the tables of the README and of DESIGN.md 10.15"""
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    t = O.window_table(s, e, a, 0, 20, EDGES4, CAP_MAX, 5)
    assert t[0].tolist() == EXAMPLE_STARTS and t[1, 1:].tolist() == EXAMPLE_SUMS
    assert t[1, 0].tolist() == [5 * CAP_MAX] * 4                      # nothing bounds the pivot: the cap times the width
    assert t[0].sum(axis=1).tolist() == [1, 10, 6, 11, 12]            # the line counts of `memo mems -m -a` per genome (and the pivot's one)
    assert O.window_table(s, e, a, 0, 20, EDGES4, CAP_MAX, 5, min_len=3)[0].tolist() == EXAMPLE_L3
    cons = G.index_columns("example_cons.parquet", "ref_1")
    assert O.window_table(*cons, 0, 20, EDGES4, CAP_MAX, 5, threshold=5)[0].tolist() == [[3, 3, 3, 3]]   # the 12 matches of `memo mems`
    assert O.window_table(*cons, 0, 20, EDGES4, CAP_MAX, 5, threshold=3)[0].sum() == 13


@pytest.mark.parametrize("index,record,n", (("example_memb.parquet", "ref_1", 5), ("rnd_n8.parquet", "chr1", 8)))
def test_the_starts_are_a_histogram_of_memo_mems_list(index, record, n):
    s, e, a = G.index_columns(index, record)
    last = int(s.max())
    for qs, qe in ((0, min(last, 300)), (7, min(last, 211))):
        for cap, min_len in ((CAP_MAX, 1), (31, 2), (4, 4)):
            for bins in (1, 3, qe - qs):
                edges = np.linspace(qs, qe, bins + 1).astype(np.int64)
                t = O.window_table(s, e, a, qs, qe, edges, cap, n, min_len=min_len)
                for g, starts, _ in mems_oracle.all_matches(s, e, a, qs, qe, cap, n, min_len=min_len):
                    assert np.array_equal(t[0, g], np.histogram(starts, edges)[0].astype(np.uint64)), (index, qs, qe, cap, min_len, bins, g)
                planes = lengths_oracle.planes(s, e, a, qs, qe, cap, n).astype(np.uint64)
                assert np.array_equal(t[1], np.add.reduceat(planes, edges[:-1] - qs, axis=1))


# ---------------------------------------------------------------------------------------
# the text
# ---------------------------------------------------------------------------------------
def test_the_tables_round_trip_through_the_text():
    from memo_amd import features, tracks
    table = np.array(EXAMPLE_STARTS, np.uint64)
    text = tracks.format_tracks(table, 0, EDGES4)
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert lines[0] == ["genome", "0-5", "5-10", "10-15", "15-20"] and [ln[0] for ln in lines[1:]] == ["0", "1", "2", "3", "4"]
    assert np.array_equal(np.array([[int(x) for x in ln[1:]] for ln in lines[1:]], np.uint64), table)
    text = tracks.format_tracks(table[4:], 7, EDGES4, [">=5"])
    assert text == "genome\t7-12\t12-17\t17-22\t22-27\n>=5\t3\t3\t3\t3\n"
    mean = tracks.fractions(np.array(EXAMPLE_SUMS, np.uint64), EDGES4)
    back = [[float(x) for x in ln.split("\t")[1:]] for ln in tracks.format_tracks(mean, 0, EDGES4).splitlines()[1:]]
    assert back == mean.tolist() and back[0] == [2.6, 2.6, 2.8, 2.4]
    bed = features.Bed(["ref_1", "ref_1", "ref_2"], [0, 5, 3], [20, 10, 3], ["a", "b", "."])
    positions = bed.ends - bed.starts
    per = np.array([[12], [3], [0]], np.uint64)
    text = features.format_features(bed, positions, per, True, ["starts"])
    assert text == "chrom\tstart\tend\tname\tpositions\tstarts\nref_1\t0\t20\ta\t20\t12\nref_1\t5\t10\tb\t5\t3\nref_2\t3\t3\t.\t0\t0\n"
    shares = features.format_features(bed, positions, features.shares(per, positions), True, ["starts"]).splitlines()
    assert shares[1].endswith("\t0.6") and shares[2].endswith("\t0.6") and shares[3].endswith("\tnan")


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import breaks_cli
    usage = breaks_cli.USAGE.encode()
    assert usage.startswith(b"\nMEMO breaks - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("breaks", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-a [FILE]", b"-o [FILE]", b"-B [INT]", b"  -m  ", b"-t [INT]", b"-l [INT]",
                 b"-K [INT]", b"  -s  ", b"  -f  ", b"-g [FILE]", b"[500]", b"[2147483647]"):
        assert flag in usage
    assert b"-k" not in usage and b"nothing in the file tells them apart" in usage and b"MEMBERSHIP" in usage
    r = _memo("breaks", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("breaks", "-k", "31")                                   # no -k, as for `memo maxk`
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("breaks", "-b")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- b\n")
    r = _memo("breaks", "-b", "x.parquet", "-r", "ref_1:0-20")
    assert r.returncode == 2 and r.stdout == b"MEMO - breaks\n" and r.stderr == b"memo breaks: -n, -o required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, breaks
    assert memo_amd.region_breaks is breaks.region_breaks and memo_amd.bed_breaks is breaks.bed_breaks
    assert memo_amd.plane_breaks is breaks.plane_breaks and memo_amd.breaks is breaks
    assert {"memo_breaks_dev", "memo_breaks_tile"} <= set(_lib.SYMBOLS)
    assert "memo_debug_breaks_times" in _lib.DEBUG_SYMBOLS and "memo_debug_breaks_times" not in _lib.SYMBOLS
    src = open(EXE).read()
    assert '"breaks"' in src and "memo_amd/breaks_cli.py" in src


def test_refusals_before_the_library_is_touched(tmp_path):
    """exit status 1, one message, nothing written (-b names no file and the library path names none: a refusal that came later
    would be another message)"""
    out = str(tmp_path / "never.tsv")
    good, bad = tmp_path / "good.bed", tmp_path / "bad.bed"
    good.write_text("ref_1\t0\t10\ta\nref_1\t5\t20\tb\n")
    bad.write_text("ref_1\t0\t10\ta\nref_1\t20\t5\tb\n")
    good, bad = str(good), str(bad)
    common = ("-b", str(tmp_path / "no.parquet"), "-n", "5", "-o", out)
    window = ("-r", "ref_1:0-20")
    for extra, env, message in (((), None, b"exactly one of -r"),
                                ((*window, "-a", good), None, b"exactly one of -r"),
                                (("-a", good, "-B", "4"), None, b"-B has no meaning with -a"),
                                ((*window, "-m", "-t", "3"), None, b"-t cannot be combined with -m"),
                                (("-a", good, "-m", "-t", "3"), None, b"-t cannot be combined with -m"),
                                ((*window, "-g", good), None, b"-g needs -m"),
                                ((*window, "-n", "0"), None, b"-n must be an integer in [1, 2048]"),
                                ((*window, "-m", "-n", "2049"), None, b"-n must be an integer in [1, 2048]"),
                                ((*window, "-n", "five"), None, b"-n must be an integer in [1, 2048]"),
                                ((*window, "-t", "0"), None, b"-t must be an integer in [1, 5]"),
                                ((*window, "-t", "6"), None, b"-t must be an integer in [1, 5]"),
                                ((*window, "-K", "0"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-K", "2147483648"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-l", "0"), None, b"-l must be an integer in [1, 2147483647]"),
                                ((*window, "-K", "7", "-l", "8"), None, b"-l must be an integer in [1, 7]"),
                                ((*window, "-B", "0"), None, b"-B must be an integer"),
                                ((*window, "-B", "many"), None, b"-B must be an integer"),
                                ((*window, "-B", "21"), None, b"21 bins for a window of 20 positions"),
                                (("-r", "ref_1:20-0"), None, b"negative dimensions"),
                                (("-r", "ref_1"), None, b"memo breaks: "),
                                (("-a", bad), None, b"line 2"),
                                (("-a", str(tmp_path / "no.bed")), None, b"cannot read the BED file"),
                                ((*window, "-m", "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                                ((*window, "-m", "-g", good), None, b"names 2 genomes, -n says 5"),
                                (window, {"WORLD_SIZE": "2"}, b"sharded launch")):
        r = _memo("breaks", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - breaks\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo breaks: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    r = _memo("breaks", *common, *window, "-m", "-B", "4")
    assert r.returncode == 1 and not os.path.exists(out)
    assert b"Traceback" in r.stderr or b"memo breaks: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.bed", "good.bed"]


def test_the_driver_refuses_before_any_device_call(monkeypatch):
    """in the style of mems._check: the library is never asked for"""
    from memo_amd import _lib, breaks, features

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(breaks, "lib", never)
    bed = features.Bed(["ref_1"], [0], [10], ["a"])
    for kw, message in ((dict(membership=True, threshold=3), "threshold cannot be combined with membership"),
                        (dict(threshold=0), r"threshold must be in \[1, 5\]"), (dict(threshold=6), r"threshold must be in \[1, 5\]"),
                        (dict(min_len=0), "min_len must be in"), (dict(cap=7, min_len=8), r"min_len must be in \[1, 7\]"),
                        (dict(cap=0), "cap must be in"), (dict(cap=2 ** 31), "cap must be in")):
        with pytest.raises(ValueError, match=message):
            breaks.region_breaks("no.parquet", "ref_1:0-20", 5, 4, **kw)
        with pytest.raises(ValueError, match=message):
            breaks.bed_breaks("no.parquet", bed, 5, **kw)
    for n in (0, 2049):
        with pytest.raises(ValueError, match=r"n_docs must be in \[1, 2048\]"):
            breaks.region_breaks("no.parquet", "ref_1:0-20", n, 4, membership=True)
        with pytest.raises(ValueError, match=r"n_docs must be in \[1, 2048\]"):
            breaks.bed_breaks("no.parquet", bed, n)
    with pytest.raises(ValueError, match="21 bins for a window of 20 positions"):
        breaks.region_breaks("no.parquet", "ref_1:0-20", 5, 21)
    with pytest.raises(ValueError, match="0 bins"):
        breaks.region_breaks("no.parquet", "ref_1:5-5", 5, 0)
    with pytest.raises(ValueError, match="negative dimensions"):
        breaks.region_breaks("no.parquet", "ref_1:20-0", 5, 4)
    with pytest.raises(ValueError, match=f"at most {2 ** 31 - 1} positions"):
        breaks.region_breaks("no.parquet", f"ref_1:0-{2 ** 31}", 5, 4)
    with pytest.raises(ValueError, match=f"at most {2 ** 31 - 1} positions"):
        breaks.bed_breaks("no.parquet", features.Bed(["r", "r"], [0, 2 ** 31], [5, 2 ** 31 + 1], ["a", "b"]), 5)
    with pytest.raises(ValueError, match="before position 0"):
        breaks._check_window(-1, 5)
    table, edges, qs = breaks.region_breaks("no.parquet", "ref_1:5-5", 5, 4, membership=True)     # an empty window touches nothing
    assert table.shape == (2, 5, 0) and table.dtype == np.uint64 and edges.tolist() == [0] and qs == 5
    assert breaks.region_breaks("no.parquet", "ref_1:5-5", 5, 4)[0].shape == (2, 1, 0)
    table, positions = breaks.bed_breaks("no.parquet", features.Bed(["r"], [3], [3], ["."]), 5, membership=True)
    assert table.shape == (2, 1, 5) and not table.any() and positions.tolist() == [0]              # a feature of no positions touches no index
