"""`memo mosaic` without a GPU: the oracle (tests/mosaic_oracle.py) against every line of the worked examples of DESIGN.md 10.18 from
the goldens, the greedy count against the dynamic programme, the host binning against one base at a time, the text writers, and the
refusals of the command line and of the driver that never reach the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from memo_amd import mosaic as _mosaic  # noqa: F401  (the oracle's tests too belong to the sub-command: none of them runs without it)
from tests import golden_util as G
from tests import mosaic_oracle as M
from tests import nearest_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
EDGES4 = np.array([0, 5, 10, 15, 20], np.int64)            # view.bin_edges(20, 4)
PANEL = [2, 3, 4, 5, 6, 7, 8, 9, 30]                        # -s 2-9,30

# ref_1:0-20 of the example, N = 5: (flags of region_mosaic, the lines as (START, END, GENOME))
EXAMPLE = [(dict(), [(0, 6, 3), (6, 13, 2), (13, 17, 3), (17, 20, 2)]),
           (dict(min_len=4), [(0, 6, 3), (6, 13, 2), (13, 17, 3), (17, 20, 2)]),
           (dict(min_len=5), [(0, 6, 3), (6, 13, 2), (13, 15, 0), (15, 20, 2)]),
           (dict(candidates=[1, 2, 4]), [(0, 5, 2), (5, 13, 2), (13, 16, 1), (16, 20, 2)]),
           (dict(candidates=[1]), [(a, b, 1) for a, b in zip([0, 3, 5, 7, 11, 13, 16, 18], [3, 5, 7, 11, 13, 16, 18, 20])]),
           (dict(candidates=[4]), [(a, b, 4) for a, b in zip([0, 3, 6, 9, 12, 14, 18], [3, 6, 9, 12, 14, 18, 20])]),
           (dict(min_len=3, cap=3), [(0, 3, 1), (3, 6, 2), (6, 9, 2), (9, 12, 2), (12, 15, 1), (15, 18, 1), (18, 20, 2)])]
EXAMPLE_3_17 = [(3, 6, 2), (6, 13, 2), (13, 17, 3)]
EXAMPLE_B4 = ([[0, 0, 0, 0], [0, 0, 0, 0], [0, 4, 3, 3], [5, 1, 2, 2], [0, 0, 0, 0]], [1, 1, 1, 1])     # rows none / 1 / 2 / 3 / 4, then phrases
# chr1 of rnd_n40.parquet, N = 40: (window, flags, lines)
RND40 = [((0, 2100), dict(), 28), ((0, 2100), dict(cap=8), 263), ((0, 2100), dict(cap=31, min_len=31), 68), ((0, 2100), dict(min_len=90), 28),
         ((0, 2100), dict(candidates=PANEL), 36), ((150, 450), dict(), 4), ((150, 450), dict(candidates=PANEL), 6)]


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def closed(rng, L, mean):
    """lengths as an index leaves them, len[p + 1] >= len[p] - 1: falling ramps between random breaks, zeros where a ramp has run out"""
    at = np.flatnonzero(rng.random(L) < 1.0 / mean)
    at = np.concatenate([[0], at[at > 0], [L]])
    reach = np.maximum.accumulate(at[:-1] + rng.integers(0, 2 * mean, len(at) - 1))    # (a match ends no earlier than the one before it)
    return np.maximum(np.repeat(reach, np.diff(at)) - np.arange(L), 0).astype(np.uint32)


@pytest.fixture(scope="module")
def planes():
    """the two goldens' windows, every genome's plane, computed once"""
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    out = {"example": O.window_planes(s, e, a, 0, 20, CAP_MAX, 5)}
    s, e, a = G.index_columns("rnd_n40.parquet", "chr1")
    out["rnd40"] = O.window_planes(s, e, a, 0, 2100, CAP_MAX, 40)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------
def test_the_worked_example_from_the_goldens(planes):
    v = planes["example"]
    for kw, want in EXAMPLE:
        kw = dict(kw)
        cap = kw.pop("cap", CAP_MAX)
        assert M.intervals(*M.greedy(*M.steps(v, cap, **kw)), 20) == want, kw
    # the parse depends on where the window starts: cells [3, 17) of the same planes, their values cut at the window's end by the walk
    assert M.intervals(*M.greedy(*M.steps(v[:, 3:17], CAP_MAX)), 17, 3) == EXAMPLE_3_17
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    assert M.intervals(*M.window_lines(s, e, a, 3, 17, CAP_MAX, 5), 17, 3) == EXAMPLE_3_17
    starts, genomes = M.greedy(*M.steps(v, CAP_MAX))
    bases, lines = M.bin_naive(starts, genomes, 20, EDGES4, 5)
    assert bases.tolist() == EXAMPLE_B4[0] and lines.tolist() == EXAMPLE_B4[1]
    # `memo nearest -i` on the same window: 11 runs where the parse has 4 lines
    assert len(O.run_code(O.winners(v, CAP_MAX))[0]) == 11


def test_the_counts_on_rnd_n40(planes):
    whole = planes["rnd40"]
    for (qs, qe), kw, count in RND40:
        kw = dict(kw)
        cap = kw.pop("cap", CAP_MAX)
        # (a window that ends before the planes' end: lengths.py's formula cuts nothing at the window's end, the walk does)
        step, winner = M.steps(whole[:, qs:qe], cap, **kw)
        starts, genomes = M.greedy(step, winner)
        assert len(starts) == count, ((qs, qe), kw)
        if kw.get("min_len") == 90:
            assert int((genomes == 0).sum()) == 13 and len(M.reached(step)) == 710 and int((winner == 0).sum()) == 1789
        else:
            assert genomes.all() and len(M.reached(step)) == count


def test_greedy_is_fewest_at_min_len_one(planes):
    """len[p + 1] >= len[p] - 1 makes p + best[p] non-decreasing, and the greedy parse then has the fewest pieces of any cover"""
    for v in (planes["example"], planes["rnd40"][:, :700], planes["rnd40"][:, 150:450]):
        for cand in (None, [1], [2, 3]):
            best = O.per_position(v, CAP_MAX, 1, cand)[0]
            assert (np.diff(best) >= -1).all()
            assert len(M.greedy(*M.steps(v, CAP_MAX, 1, cand))[0]) == M.fewest(best)
    rng = np.random.default_rng(20261021)
    for i in range(200):
        L, planes_ = int(rng.integers(1, 120)), int(rng.integers(2, 6))
        v = np.stack([closed(rng, L, int(rng.integers(2, 30))) for _ in range(planes_)])
        cap = int(rng.choice([3, 7, CAP_MAX]))
        best = O.per_position(v, cap)[0]
        assert (np.diff(best) >= -1).all(), i                     # the cap and the maximum keep the inequality
        starts, genomes = M.greedy(*M.steps(v, cap))
        assert len(M.reached(M.steps(v, cap)[0])) == M.fewest(best), i     # the phrases; the lines are fewer where none-phrases merge
        assert len(starts) <= M.fewest(best) and (len(starts) == M.fewest(best) or not genomes.all()), i
    # not promised where the lengths are not an index's: a long piece hidden behind a short one
    assert len(M.reached([2, 1, 9, 1, 1, 1, 1, 1, 1, 1, 1])) == 2 and M.fewest([2, 1, 9, 1, 1, 1, 1, 1, 1, 1, 1]) == 2
    assert len(M.reached([3, 9, 1, 1, 1, 1, 1, 1, 1, 1])) == 8 and M.fewest([3, 9, 1, 1, 1, 1, 1, 1, 1, 1]) == 2


def test_the_merging_rule_by_hand():
    #        0  1  2  3  4  5  6  7  8  9
    step = [2, 1, 1, 1, 3, 1, 1, 0, 1, 5]
    win_ = [1, 0, 0, 0, 2, 0, 0, 0, 2, 2]
    assert M.reached(step) == [0, 2, 3, 4, 7, 8, 9]                                          # a step of 0 counts as 1
    assert M.intervals(*M.greedy(step, win_), 10) == [(0, 2, 1), (2, 4, 0), (4, 7, 2), (7, 8, 0), (8, 9, 2), (9, 10, 2)]
    # a copy that ends inside a run of none: position 5 is none but not reached, so 6 begins a new `.` line only through its phrase
    assert M.intervals(*M.greedy([6, 1, 1, 1, 1, 1, 1, 1], [3, 0, 0, 0, 0, 0, 0, 0]), 8) == [(0, 6, 3), (6, 8, 0)]
    assert M.intervals(*M.greedy([1, 1, 1], [0, 0, 0]), 3) == [(0, 3, 0)]
    assert M.greedy([], [])[0].shape == (0,) and M.greedy([], [])[1].dtype == np.uint16
    s, w = M.steps([[9, 9, 9], [0, 4, 2], [0, 4, 7]], 5, 2)
    assert s.tolist() == [1, 4, 5] and w.tolist() == [0, 1, 2] and s.dtype == np.uint32 and w.dtype == np.uint16


# ---------------------------------------------------------------------------------------
# the host binning and the text
# ---------------------------------------------------------------------------------------
def test_bin_phrases_against_one_base_at_a_time():
    from memo_amd import mosaic, tracks
    rng = np.random.default_rng(3)
    seen = set()
    for L, n in ((1, 2), (20, 5), (97, 7), (400, 40)):
        for mean in (1, 3, 40):
            cut = np.flatnonzero(rng.random(L) < 1.0 / mean)
            starts = np.unique(np.concatenate([[0], cut])).astype(np.int64)
            genomes = rng.integers(0, n, len(starts)).astype(np.uint16)
            choices = [[0, L], list(range(L + 1)), tracks.region_edges(L, min(L, 7)).tolist(), sorted(rng.integers(0, L + 1, 5).tolist() + [0, L]),
                       [0, 0, L // 2, L // 2, L, L]]                            # one bin, one bin a position, view's, random, empty bins
            if len(starts) > 1:
                choices.append(sorted({0, int(starts[1]), L}))                  # a line that ends on an edge
            for edges in choices:
                bases, lines = mosaic.bin_phrases(starts, genomes, L, edges, n)
                want = M.bin_naive(starts, genomes, L, edges, n)
                assert bases.dtype == np.uint64 and lines.dtype == np.uint64 and bases.shape == (n, len(edges) - 1)
                assert np.array_equal(bases, want[0]) and np.array_equal(lines, want[1]), (L, mean, edges[:8])
                assert np.array_equal(bases.sum(axis=0), np.diff(edges).astype(np.uint64)) and int(lines.sum()) == len(starts)
                spans = np.searchsorted(edges, np.append(starts[1:], L), "left") - np.searchsorted(edges, starts, "right")
                seen.add(("spans", bool((spans >= 2).any())))
                seen.add(("empty", bool((np.diff(edges) == 0).any())))
    assert seen == {("spans", True), ("spans", False), ("empty", True), ("empty", False)}
    bases, lines = mosaic.bin_phrases([0, 6, 13, 17], [3, 2, 3, 2], 20, EDGES4, 5)
    assert bases.tolist() == EXAMPLE_B4[0] and lines.tolist() == EXAMPLE_B4[1]
    bases, lines = mosaic.bin_phrases([], [], 0, [0], 5)
    assert bases.shape == (5, 0) and lines.shape == (0,)
    for bad in (dict(edges=[1, 20]), dict(edges=[0, 19]), dict(edges=[0, 12, 10, 20]), dict(genomes=[3, 2, 3, 5]), dict(genomes=[3, 2, 3])):
        kw = dict(dict(starts=[0, 6, 13, 17], genomes=[3, 2, 3, 2], L=20, edges=EDGES4, n_docs=5), **bad)
        with pytest.raises(ValueError):
            mosaic.bin_phrases(**kw)


def test_the_table_and_the_intervals_as_text():
    from memo_amd import mosaic, nearest, tracks
    bases, lines = np.array(EXAMPLE_B4[0], np.uint64), np.array(EXAMPLE_B4[1], np.uint64)
    text = mosaic.format_mosaic(bases, lines, 0, EDGES4)
    assert text == "genome\t0-5\t5-10\t10-15\t15-20\nnone\t0\t0\t0\t0\n1\t0\t0\t0\t0\n2\t0\t4\t3\t3\n3\t5\t1\t2\t2\n4\t0\t0\t0\t0\nphrases\t1\t1\t1\t1\n"
    labelled = mosaic.format_mosaic(bases, lines, 7, EDGES4, ["pivot", "g1", "g2", "g3", "g4"]).splitlines()
    assert [ln.split("\t")[0] for ln in labelled] == ["genome", "none", "g1", "g2", "g3", "g4", "phrases"] and labelled[0].endswith("\t22-27")
    shares = mosaic.format_mosaic(tracks.fractions(bases, EDGES4), tracks.fractions(lines[None, :], EDGES4)[0], 0, EDGES4).splitlines()
    assert shares[3] == "2\t0.0\t0.8\t0.6\t0.6" and shares[-1] == "phrases\t0.2\t0.2\t0.2\t0.2"
    with pytest.raises(ValueError):
        mosaic.format_mosaic(bases, lines[:3], 0, EDGES4)
    with pytest.raises(ValueError):
        mosaic.format_mosaic(bases, lines, 0, EDGES4, ["a", "b"])
    starts, genomes = [r[0] for r in EXAMPLE[2][1]], [r[2] for r in EXAMPLE[2][1]]
    assert nearest.format_intervals("ref_1", 0, 20, starts, genomes) == "ref_1\t0\t6\t3\nref_1\t6\t13\t2\nref_1\t13\t15\t.\nref_1\t15\t20\t2\n"
    assert nearest.format_intervals("ref_1", 3, 17, [0, 3, 10], [2, 2, 3], ["p", "a", "b", "c", "d"]) == "ref_1\t3\t6\tb\nref_1\t6\t13\tb\nref_1\t13\t17\tc\n"


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import mosaic_cli
    usage = mosaic_cli.USAGE.encode()
    assert usage.startswith(b"\nMEMO mosaic - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("mosaic", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-B [INT]", b"-l [INT]", b"-K [INT]", b"-s [LIST]", b"  -f  ",
                 b"-g [FILE]", b"[2147483647]"):
        assert flag in usage
    assert b"-k" not in usage and b"-m " not in usage and b"nothing in the file can tell" in usage and b"MEMBERSHIP" in usage
    for flag, said in (("-x", b"illegal option -- x"), ("-k", b"illegal option -- k"), ("-m", b"illegal option -- m"), ("-i", b"illegal option -- i"),
                       ("-u", b"illegal option -- u")):
        r = _memo("mosaic", flag, "31")
        assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": " + said + b"\n")
    r = _memo("mosaic", "-b")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- b\n")
    r = _memo("mosaic", "-b", "x.parquet", "-r", "ref_1:0-20")
    assert r.returncode == 2 and r.stdout == b"MEMO - mosaic\n" and r.stderr == b"memo mosaic: -n, -o required\n"
    r = _memo("mosaic", "-b", "x.parquet", "-n", "5", "-o", "x.tsv")
    assert r.returncode == 2 and r.stderr == b"memo mosaic: -r required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, mosaic
    assert memo_amd.region_mosaic is mosaic.region_mosaic and memo_amd.plane_mosaic is mosaic.plane_mosaic
    assert memo_amd.bin_phrases is mosaic.bin_phrases and memo_amd.mosaic is mosaic
    assert {"region_mosaic", "plane_mosaic", "bin_phrases"} <= set(dir(memo_amd))
    assert {"memo_mosaic_fold_dev", "memo_mosaic_parse_dev", "memo_mosaic_tile"} <= set(_lib.SYMBOLS)
    for name in ("memo_debug_mosaic_times", "memo_debug_mosaic_shape"):
        assert name in _lib.DEBUG_SYMBOLS and name not in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["memo_mosaic_fold_dev"][1]) == 11 and len(_lib.SYMBOLS["memo_mosaic_parse_dev"][1]) == 8
    src = open(EXE).read()
    assert '"mosaic"' in src and "memo_amd/mosaic_cli.py" in src
    for name, text in (("include/memo_amd_dap.h", "int memo_mosaic_fold_dev("), ("include/memo_amd_dap.h", "int memo_mosaic_parse_dev("),
                       ("include/memo_amd_dap.h", "int32_t memo_mosaic_tile(void);"), ("include/memo_amd_debug.h", "int memo_debug_mosaic_times("),
                       ("memo_amd/csrc/Makefile", "memo_mosaic.o")):
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
                                ((*window, "-B", "500"), None, b"500 bins for a window of 20 positions"),
                                ((*window, "-B", "0"), None, b"-B must be an integer"),
                                ((*window, "-B", "many"), None, b"-B must be an integer"),
                                ((*window, "-f"), None, b"-f has no meaning without -B"),
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
                                (("-r", "ref_1:20-0"), None, b"negative dimensions"),
                                (("-r", "ref_1:20-0", "-B", "4"), None, b"negative dimensions"),
                                (("-r", "ref_1"), None, b"memo mosaic: "),
                                (("-r", f"ref_1:0-{2 ** 31}"), None, f"at most {2 ** 31 - 1} positions".encode()),
                                ((*window, "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                                ((*window, "-g", str(two)), None, b"names 2 genomes, -n says 5"),
                                (window, {"WORLD_SIZE": "2"}, b"sharded launch"),
                                ((*window, "-B", "4"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch")):
        r = _memo("mosaic", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - mosaic\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo mosaic: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same commands with nothing to refuse do reach the library, which is not there
    for extra in ((*window, "-B", "4"), window):
        r = _memo("mosaic", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo mosaic: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["two.txt"]


def test_the_driver_refuses_before_any_device_call(monkeypatch):
    """in the style of nearest._check: the library is never asked for"""
    from memo_amd import _device, _lib, mosaic

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(mosaic, "lib", never)
    monkeypatch.setattr(_device, "lib", never)
    call = lambda **kw: mosaic.region_mosaic("no.parquet", "ref_1:0-20", 5, **kw)              # noqa: E731
    for kw, message in ((dict(min_len=0), "min_len must be in"), (dict(cap=7, min_len=8), r"min_len must be in \[1, 7\]"), (dict(cap=0), "cap must be in"),
                        (dict(cap=2 ** 31), "cap must be in"), (dict(candidates="0"), r"names annot 0, outside \[1, 4\]"),
                        (dict(candidates=[5]), r"names annot 5, outside \[1, 4\]"), (dict(candidates="1,x"), "does not parse"),
                        (dict(candidates=[2, 2]), "names annot 2 twice")):
        with pytest.raises(ValueError, match=message):
            call(**kw)
    for n in (0, 1, 2049):
        with pytest.raises(ValueError, match=r"n_docs must be in \[2, 2048\]"):
            mosaic.region_mosaic("no.parquet", "ref_1:0-20", n)
    with pytest.raises(ValueError, match="negative dimensions"):
        mosaic.region_mosaic("no.parquet", "ref_1:20-0", 5)
    with pytest.raises(ValueError, match=f"at most {2 ** 31 - 1} positions"):
        mosaic.region_mosaic("no.parquet", f"ref_1:0-{2 ** 31}", 5)
    with pytest.raises(ValueError, match=r"cells must be \[planes, L\]"):
        mosaic.plane_mosaic(np.zeros(5, np.uint32), cap=4)
    with pytest.raises(ValueError, match="outside"):
        mosaic.plane_mosaic(np.zeros((3, 5), np.uint32), cap=4, candidates=[3])
    with pytest.raises(ValueError, match="vectors of one length"):
        mosaic.parse(np.ones(5, np.uint32), np.ones(4, np.uint16))
    starts, genomes, qs, qe = mosaic.region_mosaic("no.parquet", "ref_1:5-5", 5)                # an empty window touches nothing
    assert starts.shape == (0,) and starts.dtype == np.int64 and genomes.dtype == np.uint16 and (qs, qe) == (5, 5)
