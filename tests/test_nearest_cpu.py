"""`memo nearest` without a GPU: the two forms of the oracle (tests/nearest_oracle.py), the worked example of DESIGN.md 10.17 from the
goldens, the min_len == cap == K identity with `memo tracks`, the text writers, and the refusals of the command line and of the
driver that never reach the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from memo_amd import nearest as _nearest  # noqa: F401  (the oracle's tests too belong to the sub-command: none of them runs without it)
from tests import golden_util as G
from tests import lengths_oracle, tracks_oracle
from tests import nearest_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
EDGES4 = np.array([0, 5, 10, 15, 20], np.int64)            # view.bin_edges(20, 4)

# rows none / 1 / 2 / 3 / 4, then best: ref_1:0-20 of the example, N = 5, -B 4
EXAMPLE = ([[0, 0, 0, 0], [1, 0, 1, 0], [2, 3, 2, 4], [5, 3, 3, 2], [2, 0, 3, 2]], [21, 32, 19, 23])
EXAMPLE_SOLE = [[0, 0, 0, 0], [0, 0, 1, 0], [0, 2, 0, 2], [2, 2, 1, 1], [0, 0, 1, 0]]
EXAMPLE_L4 = [[2, 0, 1, 1], [0, 0, 1, 0], [1, 3, 1, 3], [3, 3, 2, 1], [1, 0, 2, 1]]
EXAMPLE_K3 = ([[0, 0, 0, 0], [3, 2, 3, 2], [4, 5, 3, 4], [5, 5, 5, 5], [4, 5, 4, 5]], [15, 15, 15, 15])
EXAMPLE_S124 = ([[0, 0, 0, 0], [1, 0, 2, 0], [4, 5, 3, 4], [0, 0, 0, 0], [2, 0, 4, 3]], [19, 30, 18, 21])
EXAMPLE_BEST = [6, 5, 4, 3, 3, 8, 7, 6, 6, 5, 4, 3, 4, 4, 4, 6, 5, 4, 3, 5]           # the README's `memo lengths -t 2` line
EXAMPLE_RUNS = [(0, 2, 3), (2, 4, 2), (4, 5, 1), (5, 8, 2), (8, 10, 3), (10, 12, 2), (12, 13, 1), (13, 14, 3), (14, 15, 4), (15, 19, 2), (19, 20, 3)]
EXAMPLE_RUNS_L4 = [(0, 2, 3), (2, 3, 2), (3, 5, 0), (5, 8, 2), (8, 10, 3), (10, 11, 2), (11, 12, 0), (12, 13, 1), (13, 14, 3), (14, 15, 4), (15, 18, 2),
                   (18, 19, 0), (19, 20, 3)]


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def _runs(starts, values, end):
    starts = [int(s) for s in starts]
    return list(zip(starts, starts[1:] + [end], [int(v) for v in values]))


# ---------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------
def test_the_two_forms_of_the_oracle_agree():
    rng = np.random.default_rng(20261021)
    seen = set()
    for planes, L, cap in ((2, 1, 4), (3, 2, 4), (4, 17, 4), (3, 64, 3), (2, 40, 1), (5, 33, CAP_MAX), (9, 21, 4)):
        v = rng.integers(0, min(cap, 6) + 3, (planes, L))                    # (some cells above the cap)
        for first in (0, 7, 2 ** 33):
            for cuts in ([0, L], [0, L // 2, L], sorted([-5, 0, 0, 1, L - 1, L, L + 9]), sorted(rng.integers(0, L + 1, 6).tolist() + [0, L]),
                         list(range(L + 1))):
                edges = np.asarray(cuts, np.int64) + first
                for cand in (None, [planes - 1], list(range(1, planes, 2))):
                    for min_len in sorted({1, 2, min(cap, 6)}):
                        wins, sums = O.table(v, edges, cap, min_len, cand, first)
                        slow = O.naive(v, edges, cap, min_len, cand, first)
                        assert wins.dtype == np.uint64 and wins.shape == (2, planes, len(cuts) - 1) and sums.shape == (len(cuts) - 1,)
                        assert np.array_equal(wins, slow[0]) and np.array_equal(sums, slow[1])
                        assert np.array_equal(O.winners(v, cap, min_len, cand), slow[2])
                        assert (wins[1] <= wins[0]).all() and np.array_equal(wins[0, 0], wins[1, 0])
                        assert int(wins[1].sum()) <= L and int(wins[0, 0].sum() + wins[0, 1:].sum()) >= L
                        outside = [g for g in range(1, planes) if cand is not None and g not in cand]
                        assert not wins[:, outside].any()
                        seen.add((bool(wins[0, 0].any()), bool((wins[1, 1:] < wins[0, 1:]).any())))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert _runs(*O.run_code(np.array([3, 3, 0, 0, 0, 1], np.uint16)), 6) == [(0, 2, 3), (2, 5, 0), (5, 6, 1)]
    assert O.run_code(np.zeros(0, np.uint16))[0].shape == (0,)


def test_the_definition_by_hand():
    """cap = 4, three candidates: a sole winner, a tie, a tie at the cap (a cell above it counts as the cap), nothing at all"""
    v = [[9, 9, 9, 9, 9], [3, 2, 4, 0, 1], [1, 2, 9, 0, 0], [0, 1, 4, 0, 1]]
    wins, sums = O.table(v, [0, 5], 4)
    assert wins[0, :, 0].tolist() == [1, 4, 2, 2] and wins[1, :, 0].tolist() == [1, 1, 0, 0] and sums.tolist() == [3 + 2 + 4 + 0 + 1]
    assert O.winners(v, 4).tolist() == [1, 1, 1, 0, 1]
    assert O.table(v, [0, 5], 4, min_len=2)[0][0, :, 0].tolist() == [2, 3, 2, 1] and O.winners(v, 4, 2).tolist() == [1, 1, 1, 0, 0]
    assert O.winners(v, 4, 1, [2, 3]).tolist() == [2, 2, 2, 0, 3] and O.table(v, [0, 5], 4, 1, [2, 3])[1].tolist() == [1 + 2 + 4 + 0 + 1]
    assert O.table(v, [0, 5], 4, 1, [2, 3])[0][:, 1, 0].tolist() == [0, 0]                 # outside the set: an empty row


def test_the_worked_example_from_the_goldens():
    """ref_1:0-20 of the example pair, N = 5, -B 4: every table of the README and of DESIGN.md 10.17"""
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    table = lambda **kw: O.window_table(s, e, a, 0, 20, EDGES4, kw.pop("cap", CAP_MAX), 5, **kw)      # noqa: E731
    wins, sums = table()
    assert wins[0].tolist() == EXAMPLE[0] and sums.tolist() == EXAMPLE[1] and wins[1].tolist() == EXAMPLE_SOLE
    wins, sums = table(min_len=4)
    assert wins[0].tolist() == EXAMPLE_L4 and sums.tolist() == EXAMPLE[1]
    assert wins[1].tolist() == [EXAMPLE_L4[0]] + EXAMPLE_SOLE[1:]                                        # -l 4 -u
    wins, sums = table(min_len=3, cap=3)
    assert wins[0].tolist() == EXAMPLE_K3[0] and sums.tolist() == EXAMPLE_K3[1] and not wins[1, 1:].any()
    wins, sums = table(candidates=[1, 2, 4])
    assert wins[0].tolist() == EXAMPLE_S124[0] and sums.tolist() == EXAMPLE_S124[1]
    per = O.window_table(s, e, a, 0, 20, np.arange(21), CAP_MAX, 5)[1]
    assert per.tolist() == EXAMPLE_BEST
    assert np.array_equal(per, lengths_oracle.kth(s, e, a, 0, 20, CAP_MAX, 5, 2))                       # the pivot's plane is the cap: T = 2
    assert not (a == 0).any()
    assert _runs(*O.window_winners(s, e, a, 0, 20, CAP_MAX, 5), 20) == EXAMPLE_RUNS
    assert _runs(*O.window_winners(s, e, a, 0, 20, CAP_MAX, 5, min_len=4), 20) == EXAMPLE_RUNS_L4


def test_min_len_equal_to_the_cap_is_memo_tracks():
    """MINLEN = CAP = K: a genome attains exactly where its length is at least K, which is its bit of `memo query -m -k K`"""
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "rnd_n40_memb_k31_c0w1")
    rec, qs, qe = G.region(c)
    s, e, a = G.index_columns(c["index"], rec)
    assert (e >= s).all()
    B = G.expected_matrix(c, G.load(c))
    assert B.shape == (qe - qs, c["n"]) and B[:, 1:].any() and not B[:, 1:].all()
    for bins in (1, 7, qe - qs):
        edges = np.linspace(qs, qe, bins + 1).astype(np.int64)
        wins, sums = O.window_table(s, e, a, qs, qe, edges, c["k"], c["n"], min_len=c["k"])
        want = tracks_oracle.tracks(B, edges, qs)
        assert np.array_equal(wins[0, 1:], want[1:].astype(np.uint64)), bins
        assert np.array_equal(wins[0, 0], (np.diff(edges) - tracks_oracle.tracks(B[:, 1:].any(axis=1, keepdims=True), edges, qs)[0]).astype(np.uint64))


# ---------------------------------------------------------------------------------------
# the text
# ---------------------------------------------------------------------------------------
def test_the_table_and_the_intervals_round_trip_through_the_text():
    from memo_amd import nearest, tracks
    wins, sums = np.array(EXAMPLE[0], np.uint64), np.array(EXAMPLE[1], np.uint64)
    text = nearest.format_nearest(wins, sums, 0, EDGES4)
    assert text == ("genome\t0-5\t5-10\t10-15\t15-20\nnone\t0\t0\t0\t0\n1\t1\t0\t1\t0\n2\t2\t3\t2\t4\n3\t5\t3\t3\t2\n4\t2\t0\t3\t2\n"
                    "best\t21\t32\t19\t23\n")
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert np.array_equal(np.array([[int(x) for x in ln[1:]] for ln in lines[1:-1]], np.uint64), wins)
    assert [int(x) for x in lines[-1][1:]] == EXAMPLE[1]
    labelled = nearest.format_nearest(wins, sums, 7, EDGES4, ["pivot", "g1", "g2", "g3", "g4"]).splitlines()
    assert [ln.split("\t")[0] for ln in labelled] == ["genome", "none", "g1", "g2", "g3", "g4", "best"] and labelled[0].endswith("\t22-27")
    shares = nearest.format_nearest(tracks.fractions(wins, EDGES4), tracks.fractions(sums[None, :], EDGES4)[0], 0, EDGES4).splitlines()
    assert shares[4] == "3\t1.0\t0.6\t0.6\t0.4" and shares[-1] == "best\t4.2\t6.4\t3.8\t4.6"
    with pytest.raises(ValueError):
        nearest.format_nearest(wins, sums[:3], 0, EDGES4)
    with pytest.raises(ValueError):
        nearest.format_nearest(wins, sums, 0, EDGES4, ["a", "b"])
    starts, values = [r[0] for r in EXAMPLE_RUNS_L4], [r[2] for r in EXAMPLE_RUNS_L4]
    text = nearest.format_intervals("ref_1", 0, 20, starts, values)
    assert text.count("\n") == 13 and text.startswith("ref_1\t0\t2\t3\nref_1\t2\t3\t2\nref_1\t3\t5\t.\n") and text.endswith("ref_1\t19\t20\t3\n")
    back = [(int(f[1]), int(f[2]), 0 if f[3] == "." else int(f[3])) for f in (ln.split("\t") for ln in text.splitlines())]
    assert back == EXAMPLE_RUNS_L4
    assert nearest.format_intervals("c", 100, 109, [0, 4], [2, 0], ["p", "a", "b"]) == "c\t100\t104\tb\nc\t104\t109\t.\n"
    assert nearest.format_intervals("c", 5, 5, [], []) == ""


def test_candidate_words():
    from memo_amd import nearest
    w = nearest.candidate_words(None, 5)
    assert w.dtype == np.uint32 and w.shape == (64,) and w[0] == 0b11110 and not w[1:].any()
    w = nearest.candidate_words("31-33,2047", 2048)
    assert w[0] == 1 << 31 and w[1] == 0b11 and w[63] == 1 << 31 and not w[2:63].any()
    assert nearest.candidate_words([1, 64], 65)[2] == 1
    raw = np.arange(64, dtype=np.uint32)
    assert nearest.candidate_words(raw, 5) is raw or np.array_equal(nearest.candidate_words(raw, 5), raw)
    for bad in ("0", "5", "1,1", "x", "3-1", ""):
        with pytest.raises(ValueError):
            nearest.candidate_words(bad, 5)


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import nearest_cli
    usage = nearest_cli.USAGE.encode()
    assert usage.startswith(b"\nMEMO nearest - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("nearest", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-B [INT]", b"-l [INT]", b"-K [INT]", b"-s [LIST]", b"  -u  ",
                 b"  -f  ", b"-g [FILE]", b"  -i  ", b"[500]", b"[2147483647]"):
        assert flag in usage
    assert b"-k" not in usage and b"-m " not in usage and b"nothing in the file can tell" in usage and b"MEMBERSHIP" in usage
    for flag, said in (("-x", b"illegal option -- x"), ("-k", b"illegal option -- k"), ("-m", b"illegal option -- m"), ("-a", b"illegal option -- a")):
        r = _memo("nearest", flag, "31")
        assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": " + said + b"\n")
    r = _memo("nearest", "-b")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- b\n")
    r = _memo("nearest", "-b", "x.parquet", "-r", "ref_1:0-20")
    assert r.returncode == 2 and r.stdout == b"MEMO - nearest\n" and r.stderr == b"memo nearest: -n, -o required\n"
    r = _memo("nearest", "-b", "x.parquet", "-n", "5", "-o", "x.tsv")
    assert r.returncode == 2 and r.stderr == b"memo nearest: -r required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, nearest
    assert memo_amd.region_nearest is nearest.region_nearest and memo_amd.region_winners is nearest.region_winners
    assert memo_amd.plane_nearest is nearest.plane_nearest and memo_amd.nearest is nearest
    assert {"region_nearest", "region_winners", "plane_nearest"} <= set(dir(memo_amd))
    assert {"memo_nearest_dev", "memo_nearest_tile"} <= set(_lib.SYMBOLS)
    assert "memo_debug_nearest_times" in _lib.DEBUG_SYMBOLS and "memo_debug_nearest_times" not in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["memo_nearest_dev"][1]) == 15
    src = open(EXE).read()
    assert '"nearest"' in src and "memo_amd/nearest_cli.py" in src
    for name, text in (("include/memo_amd_dap.h", "int memo_nearest_dev("), ("include/memo_amd_dap.h", "int32_t memo_nearest_tile(int32_t planes);"),
                       ("include/memo_amd_debug.h", "int memo_debug_nearest_times("), ("memo_amd/csrc/Makefile", "memo_nearest.o")):
        assert text in open(os.path.join(ROOT, name)).read(), (name, text)


def test_refusals_before_the_library_is_touched(tmp_path):
    """exit status 1, one message, nothing written (-b names no file and the library path names none: a refusal that came later
    would be another message)"""
    out = str(tmp_path / "never.tsv")
    two = tmp_path / "two.txt"
    two.write_text("pivot.fa\ng1.fa\n")
    common = ("-b", str(tmp_path / "no.parquet"), "-n", "5", "-o", out)
    window = ("-r", "ref_1:0-20")
    for extra, env, message in (((*window, "-B", "21"), None, b"21 bins for a window of 20 positions"),
                                (window, None, b"500 bins for a window of 20 positions"),
                                ((*window, "-B", "0"), None, b"-B must be an integer"),
                                ((*window, "-B", "many"), None, b"-B must be an integer"),
                                ((*window, "-K", "7", "-l", "8"), None, b"-l must be an integer in [1, 7]"),
                                ((*window, "-l", "0"), None, b"-l must be an integer in [1, 2147483647]"),
                                ((*window, "-K", "0"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-K", "2147483648"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-s", "1,,2"), None, b"does not parse"),
                                ((*window, "-s", "one"), None, b"does not parse"),
                                ((*window, "-s", "3-1"), None, b"a range runs upwards"),
                                ((*window, "-s", "0,1"), None, b"names annot 0, outside [1, 4]"),
                                ((*window, "-s", "1-5"), None, b"names annot 5, outside [1, 4]"),
                                ((*window, "-s", "2,2"), None, b"names annot 2 twice"),
                                ((*window, "-n", "1"), None, b"-n must be an integer in [2, 2048]"),
                                ((*window, "-n", "2049"), None, b"-n must be an integer in [2, 2048]"),
                                ((*window, "-n", "five"), None, b"-n must be an integer in [2, 2048]"),
                                ((*window, "-i", "-B", "4"), None, b"-B has no meaning with -i"),
                                ((*window, "-i", "-u"), None, b"-u has no meaning with -i"),
                                ((*window, "-i", "-f"), None, b"-f has no meaning with -i"),
                                (("-r", "ref_1:20-0"), None, b"negative dimensions"),
                                (("-r", "ref_1:20-0", "-i"), None, b"negative dimensions"),
                                (("-r", "ref_1"), None, b"memo nearest: "),
                                ((*window, "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                                ((*window, "-g", str(two)), None, b"names 2 genomes, -n says 5"),
                                (window, {"WORLD_SIZE": "2"}, b"sharded launch"),
                                ((*window, "-i"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch")):
        r = _memo("nearest", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - nearest\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo nearest: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same commands with nothing to refuse do reach the library, which is not there
    for extra in ((*window, "-B", "4"), (*window, "-i")):
        r = _memo("nearest", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo nearest: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["two.txt"]


def test_the_driver_refuses_before_any_device_call(monkeypatch):
    """in the style of breaks._check: the library is never asked for"""
    from memo_amd import _device, _lib, nearest

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(nearest, "lib", never)
    monkeypatch.setattr(_device, "lib", never)
    both = (lambda **kw: nearest.region_nearest("no.parquet", "ref_1:0-20", 5, 4, **kw), lambda **kw: nearest.region_winners("no.parquet", "ref_1:0-20", 5, **kw))
    for kw, message in ((dict(min_len=0), "min_len must be in"), (dict(cap=7, min_len=8), r"min_len must be in \[1, 7\]"), (dict(cap=0), "cap must be in"),
                        (dict(cap=2 ** 31), "cap must be in"), (dict(candidates="0"), r"names annot 0, outside \[1, 4\]"),
                        (dict(candidates=[5]), r"names annot 5, outside \[1, 4\]"), (dict(candidates="1,x"), "does not parse"),
                        (dict(candidates=[2, 2]), "names annot 2 twice")):
        for call in both:
            with pytest.raises(ValueError, match=message):
                call(**kw)
    for n in (0, 1, 2049):
        with pytest.raises(ValueError, match=r"n_docs must be in \[2, 2048\]"):
            nearest.region_nearest("no.parquet", "ref_1:0-20", n, 4)
        with pytest.raises(ValueError, match=r"n_docs must be in \[2, 2048\]"):
            nearest.region_winners("no.parquet", "ref_1:0-20", n)
    with pytest.raises(ValueError, match="21 bins for a window of 20 positions"):
        nearest.region_nearest("no.parquet", "ref_1:0-20", 5, 21)
    with pytest.raises(ValueError, match="0 bins"):
        nearest.region_nearest("no.parquet", "ref_1:5-5", 5, 0)
    for call in (lambda r: nearest.region_nearest("no.parquet", r, 5, 4), lambda r: nearest.region_winners("no.parquet", r, 5)):
        with pytest.raises(ValueError, match="negative dimensions"):
            call("ref_1:20-0")
        with pytest.raises(ValueError, match=f"at most {2 ** 31 - 1} positions"):
            call(f"ref_1:0-{2 ** 31}")
    with pytest.raises(ValueError, match=r"cells must be \[planes, L\]"):
        nearest.plane_nearest(np.zeros(5, np.uint32), [0, 5], cap=4)
    with pytest.raises(ValueError, match="wins must be"):
        nearest.plane_nearest(np.zeros((3, 5), np.uint32), [0, 5], cap=4, wins=np.zeros((2, 3, 2), np.uint64))
    with pytest.raises(ValueError, match="sums must be"):
        nearest.plane_nearest(np.zeros((3, 5), np.uint32), [0, 5], cap=4, sums=np.zeros(2, np.uint64))
    with pytest.raises(ValueError, match="outside"):
        nearest.plane_nearest(np.zeros((3, 5), np.uint32), [0, 5], cap=4, candidates=[3])
    wins, sums, edges, qs = nearest.region_nearest("no.parquet", "ref_1:5-5", 5, 4)                 # an empty window touches nothing
    assert wins.shape == (2, 5, 0) and wins.dtype == np.uint64 and sums.shape == (0,) and edges.tolist() == [0] and qs == 5
    starts, winners, qs, qe = nearest.region_winners("no.parquet", "ref_1:5-5", 5)
    assert starts.shape == (0,) and starts.dtype == np.int64 and winners.dtype == np.uint16 and (qs, qe) == (5, 5)
