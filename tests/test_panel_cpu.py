"""`memo panel` without a GPU: the oracle (tests/panel_oracle.py) against every row of the worked tables (tests/panel_tables.py)
from the goldens and against the oracle of `memo collect` on its own order, ties on hand-made bits, the host's lazy choice against
the eager one, the text against literals, the command line as far as it goes without the library, and the new symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from memo_amd import panel as _panel  # noqa: F401  (the oracle's tests too belong to the sub-command: none of them runs without it)
from tests import collect_oracle
from tests import golden_util as G
from tests import panel_oracle as P
from tests import panel_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def golden_bits(index, record, qs, qe, k, n):
    """B uint8 [L, N] of a window of a golden index, by the CPU oracle of `memo query -m`"""
    from oracle import memo_oracle
    s, e, o = G.index_columns(index, record)
    bits = memo_oracle.np_membership(*memo_oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n)
    return collect_oracle.unpack(bits, n)


def oracle_kw(kw):
    """region_panel's flags as the oracle takes them"""
    from memo_amd.merge import parse_selection
    out = {}
    if "objective" in kw:
        out["objective"] = kw["objective"]
    if "candidates" in kw:
        out["candidates"] = parse_selection(kw["candidates"], 10 ** 6)
    if "seeds" in kw:
        out["seeds"] = parse_selection(kw["seeds"], 10 ** 6)
    if "max_genomes" in kw:
        out["most"] = kw["max_genomes"]
    if "fraction" in kw:
        out["fraction"] = kw["fraction"]
    return out


@pytest.fixture(scope="module")
def bits():
    """the goldens' windows at every k of the tables, computed once"""
    out = {("example", k): golden_bits("example_memb.parquet", "ref_1", 0, 20, k, 5) for k in (3, 4, 5)}
    for k in (31, 12, 8):
        out[("rnd40", k)] = golden_bits("rnd_n40.parquet", "chr1", 0, 2100, k, 40)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------
def test_the_example_tables(bits):
    for k, kw, want in T.EXAMPLE:
        assert P.rows(P.greedy(bits[("example", k)], **oracle_kw(kw))) == want, (k, kw)
    B = bits[("example", 4)]
    assert int(B[:, 2].sum()) == 12 and int(B[:, 3].sum()) == 12                   # the tie of the k = 4 rows


def test_the_rnd_n40_tables(bits):
    for k, kw, begins, first, last in T.RND40:
        got = P.rows(P.greedy(bits[("rnd40", k)], **oracle_kw(kw)))
        assert len(got) == 39 and [r[0] for r in got[:12]] == begins and got[:len(first)] == first and got[-1] == last, (k, kw)
    for (qs, qe), k, kw, want in T.RND40_STOPS:
        B = bits[("rnd40", k)][qs:qe] if (qs, qe) == (0, 2100) else golden_bits("rnd_n40.parquet", "chr1", qs, qe, k, 40)
        got = P.rows(P.greedy(B, **oracle_kw(kw)))
        assert (len(got) == want) if isinstance(want, int) else (got == want), ((qs, qe), k, kw)


def test_the_oracle_against_collects_on_its_own_order(bits):
    for (name, k), B in bits.items():
        for kw in (dict(), dict(objective="core"), dict(seeds=[2, 1]), dict(most=3), dict(fraction="0.5")):
            order, core, covered = P.greedy(B, **kw)
            assert len(set(order)) == len(order) and 0 not in order
            want = collect_oracle.curves(B, [order])
            assert core == want[0][0].tolist() and covered == want[1][0].tolist(), (name, k, kw)
            assert all(a >= b for a, b in zip(core, core[1:])) and all(a <= b for a, b in zip(covered, covered[1:]))


def test_ties_on_hand_made_bits():
    #             p  1  2  3  4  5
    B = np.array([[1, 1, 1, 0, 1, 0],
                  [1, 1, 1, 0, 1, 0],
                  [1, 0, 0, 0, 1, 0],
                  [1, 0, 0, 0, 0, 0]], np.uint8)
    # 4 covers most; 1 and 2 are duplicate columns: the lower annot first; 3 and 5 are all-zero columns: last, the lower annot first
    assert P.rows(P.greedy(B)) == [(4, 3, 3), (1, 2, 3), (2, 2, 3), (3, 0, 3), (5, 0, 3)]
    assert P.rows(P.greedy(B, "core")) == [(4, 3, 3), (1, 2, 3), (2, 2, 3), (3, 0, 3), (5, 0, 3)]
    assert P.rows(P.greedy(B, candidates=[2, 1])) == [(1, 2, 2), (2, 2, 2)]                       # not the order written: the annot
    assert P.rows(P.greedy(B, candidates=[5, 3])) == [(3, 0, 0), (5, 0, 0)]
    assert P.rows(P.greedy(B, candidates=[2])) == [(2, 2, 2)]                                     # a lone candidate
    assert P.rows(P.greedy(B, candidates=[5])) == [(5, 0, 0)]
    assert P.rows(P.greedy(B, seeds=[5, 2])) == [(5, 0, 0), (2, 0, 2), (4, 0, 3), (1, 0, 3), (3, 0, 3)]     # seeds in the order written
    assert P.rows(P.greedy(B, seeds=[2], candidates=[2, 4])) == [(2, 2, 2), (4, 2, 3)]            # a seed leaves the candidates
    assert P.rows(P.greedy(B, seeds=[2], candidates=[1])) == [(2, 2, 2), (1, 2, 2)]               # ... and need not be one
    assert P.rows(P.greedy(B, fraction=0)) == [] and P.rows(P.greedy(B, seeds=[3], fraction=0)) == [(3, 0, 0)]
    assert P.rows(P.greedy(B, fraction="0.75")) == [(4, 3, 3)] and len(P.rows(P.greedy(B, fraction=1))) == 5
    assert P.rows(P.greedy(B, most=0)) == [] and P.rows(P.greedy(B, seeds=[1], most=1)) == [(1, 2, 2)]
    # the objectives part where covering more costs the core: 1 holds three of four positions, 2 a fourth one only
    B = np.array([[1, 1, 0, 1], [1, 1, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0]], np.uint8)
    assert P.rows(P.greedy(B)) == [(1, 3, 3), (2, 0, 4), (3, 0, 4)]
    assert P.rows(P.greedy(B, "core")) == [(1, 3, 3), (3, 2, 3), (2, 0, 4)]
    assert P.greedy(np.zeros((0, 3), np.uint8)) == ([1, 2], [0, 0], [0, 0])


# ---------------------------------------------------------------------------------------
# the host's choice
# ---------------------------------------------------------------------------------------
def numpy_state(B):
    """score and take of panel.greedy on NumPy masks, and the lists every call of score was made with"""
    B = np.asarray(B).astype(bool)
    state = {"core": np.ones(len(B), bool), "covered": np.zeros(len(B), bool), "calls": []}

    def score(genomes):
        state["calls"].append(list(genomes))
        return [[int((B[:, g] & ~state["covered"]).sum()), int((B[:, g] & state["core"]).sum())] for g in genomes]

    def take(g):
        state["core"], state["covered"] = state["core"] & B[:, g], state["covered"] | B[:, g]
        return int(state["core"].sum()), int(state["covered"].sum())
    return score, take, state


def test_lazy_equals_eager_and_the_oracle_on_random_bits():
    from memo_amd import panel
    rng = np.random.default_rng(20261021)
    spared = 0
    for i in range(120):
        L, N = int(rng.integers(1, 300)), int(rng.integers(2, 40))
        density = rng.choice([0.05, 0.5, 0.95])
        B = (rng.random((L, N)) < density).astype(np.uint8)
        if i % 3 == 0:
            B[:, rng.integers(1, N, 3)] = B[:, [1]]                                # duplicate columns: ties
        if i % 4 == 0:
            B[:, rng.integers(1, N)] = 0
        B[:, 0] = 1
        objective = ("covered", "core")[i % 2]
        everyone = list(range(1, N))
        seeds = [int(g) for g in rng.permutation(everyone)[:int(rng.integers(0, 3))]] if i % 5 == 0 else []
        cand = [int(g) for g in rng.permutation(everyone)[:int(rng.integers(1, N))]] if i % 7 == 0 else everyone
        cand = [g for g in cand if g not in seeds]
        most = None if i % 6 else len(seeds) + int(rng.integers(0, 4))
        fraction = None if i % 9 else "0.9"
        want = P.greedy(B, objective, cand, seeds, most, fraction)
        stop_at = panel.threshold(fraction, L)
        got = {}
        for lazy in (True, False):
            score, take, state = numpy_state(B)
            got[lazy] = panel.greedy(score, take, L, cand, seeds, objective, most, stop_at, lazy=lazy)
            got[lazy, "scored"] = panel.planes_scored()
            assert got[lazy, "scored"] == sum(len(c) for c in state["calls"])
        assert got[True] == got[False] == want, i
        steps = len(want[0]) - len(seeds[:len(want[0])])
        assert got[False, "scored"] == sum(len(cand) - j for j in range(steps))      # eager: every remaining candidate, every step
        assert got[True, "scored"] <= got[False, "scored"] <= len(cand) * (len(cand) + 1) // 2
        spared += got[False, "scored"] - got[True, "scored"]
    assert spared > 0


def test_a_lazy_step_stops_at_the_first_bound_it_beats():
    from memo_amd import panel
    # genome 1 covers everything: after it every `new` is 0 and the bounds by `kept` decide; 24 candidates in batches of 8
    L, N = 64, 25
    B = np.zeros((L, N), np.uint8)
    B[:, 0] = B[:, 1] = 1
    for g in range(2, N):
        B[:g, g] = 1                                                               # nested: kept never changes once 1 and 2 are taken
    score, take, state = numpy_state(B)
    order, core, covered = panel.greedy(score, take, L, list(range(1, N)))
    assert (order, core, covered) == P.greedy(B)
    assert order == [1] + list(range(N - 1, 1, -1))
    assert state["calls"][0] == list(range(1, 9))              # step 1 stops after one batch: genome 1's fresh key is at least every bound left
    assert len(state["calls"]) <= 2 * len(order) and len(state["calls"][1]) == panel.LAZY_BATCH       # a step is two calls at the most
    assert panel.planes_scored() == sum(len(c) for c in state["calls"]) <= 0.6 * ((N - 1) * N // 2)        # of what rescoring everyone reads


def test_plan_and_threshold_refuse_without_the_library(monkeypatch):
    from memo_amd import _device, _lib, panel

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(panel, "lib", never)
    monkeypatch.setattr(_device, "lib", never)
    assert panel.plan(5) == ([1, 2, 3, 4], [], 4)
    assert panel.plan(5, "core", "4,1-2", "3,1", 3) == ([4, 2], [3, 1], 3)
    assert panel.plan(5, seeds=[2], candidates=[1]) == ([1], [2], 2)
    for args, message in (((1,), r"n_docs must be in \[2, 2048\]"), ((2049,), "n_docs must be in"), ((5, "both"), "objective must be one of covered, core"),
                          ((5, "core", "0"), r"names annot 0, outside \[1, 4\]"), ((5, "core", "1,1"), "names annot 1 twice"),
                          ((5, "core", None, "2,2"), "names annot 2 twice"), ((5, "core", None, "x"), "does not parse"),
                          ((5, "core", None, "1,2", 1), "max_genomes = 1 is below the 2 seeds")):
        with pytest.raises(ValueError, match=message):
            panel.plan(*args)
    assert [panel.threshold(f, 20) for f in ("0.7", 0.7, "0", 1, "1", "0.71", None)] == [14, 14, 0, 20, 20, 15, None]
    assert panel.threshold("0.95", 2100) == 1995 and panel.threshold(1 / 3, 3) == 1
    for bad in ("-0.1", "1.01", "half", "nan", 2):
        with pytest.raises(ValueError):
            panel.threshold(bad, 20)
    for kw in (dict(slice_positions=0), dict(slice_positions=33), dict(slice_positions=16)):
        with pytest.raises(ValueError, match="multiple of 32"):
            panel.region_panel("no.parquet", "ref_1:0-20", 3, 5, **kw)
    with pytest.raises(ValueError, match="negative dimensions"):
        panel.region_panel("no.parquet", "ref_1:20-0", 3, 5)
    order, core, covered, L = panel.region_panel("no.parquet", "ref_1:5-5", 3, 5)             # an empty window touches nothing
    assert (order.shape, core.shape, covered.shape, L) == ((0,), (0,), (0,), 0) and order.dtype == np.uint16 and core.dtype == np.uint64
    assert panel.planes_scored() == 0


# ---------------------------------------------------------------------------------------
# the text
# ---------------------------------------------------------------------------------------
def test_format_against_literals():
    from memo_amd import collect, panel
    k, kw, rows = T.EXAMPLE[0]
    order, core, covered = (list(c) for c in zip(*rows))
    text = panel.format_panel(20, order, core, covered)
    assert text == T.README_EXAMPLE
    assert text == collect.format_curves(20, np.array([core]), np.array([covered]), "curve", np.array([order]), ["0", "1", "2", "3", "4"])
    named = panel.format_panel(20, np.array(order, np.uint16), np.array(core, np.uint64), np.array(covered, np.uint64), ["pivot", "g1", "g2", "g3", "g4"])
    assert named == "genomes\tcore\tcovered\tadded\n1\t20\t0\tpivot\n2\t20\t20\tg3\n3\t18\t20\tg4\n4\t16\t20\tg2\n5\t8\t20\tg1\n"
    assert panel.format_panel(20, [], [], []) == "genomes\tcore\tcovered\tadded\n1\t20\t0\t0\n"         # -f 0 without seeds: the pivot alone
    assert panel.format_panel(2 ** 33, [7], [2 ** 32 + 1], [2 ** 32 + 5]) == f"genomes\tcore\tcovered\tadded\n1\t{2 ** 33}\t0\t0\n2\t{2 ** 32 + 1}\t{2 ** 32 + 5}\t7\n"
    assert panel.format_panel(0, [], [], []) == "" and panel.format_panel(0, [], [], [], ["p", "a"]) == ""    # an empty window: an empty file


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import panel_cli
    usage = panel_cli.USAGE.encode()
    assert usage == open(os.path.join(G.GOLD, "cli", "memo_panel_usage.txt"), "rb").read()
    assert usage.startswith(b"\nMEMO panel - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("panel", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-k [INT]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-O [covered|core]", b"-s [LIST]", b"-i [LIST]", b"-m [INT]",
                 b"-f [FRACTION]", b"-g [FILE]", b"[31]"):
        assert flag in usage
    assert b"MEMBERSHIP" in usage and b"nothing can tell" in usage
    r = _memo("panel", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("panel", "-n", "5", "-O")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- O\n")
    r = _memo("panel", "-b", "x.parquet", "-k", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - panel\n" and r.stderr == b"memo panel: -r, -n, -o required\n"
    r = _memo("panel", "-r", "ref_1:0-20", "-n", "5", "-o", "x")
    assert r.returncode == 2 and r.stderr == b"memo panel: -b required\n"
    for argv, fixture in (([], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):            # the reference's texts stay the reference's
        assert _memo(*argv).stdout == open(os.path.join(G.GOLD, "cli", fixture), "rb").read()


def test_refusals_before_the_library_is_touched(tmp_path):
    """exit status 1, one message, nothing written (-b names no file and the library path names none: a refusal that came later
    would be another message)"""
    out = str(tmp_path / "never.tsv")
    four = tmp_path / "four.txt"
    four.write_text("pivot.fa\ng1.fa\ng2.fa\ng3.fa\n")
    common = ("-b", str(tmp_path / "no.parquet"), "-k", "3", "-o", out)
    window = ("-r", "ref_1:0-20", "-n", "5")
    for extra, env, message in ((window, {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (window, {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-r", "ref_1:0-20", "-n", "five"), None, b"-n must be an integer in [2, 2048]"),
                                (("-r", "ref_1:0-20", "-n", "1"), None, b"-n must be an integer in [2, 2048]"),
                                (("-r", "ref_1:0-20", "-n", "2049"), None, b"-n must be an integer in [2, 2048]"),
                                ((*window, "-k", "3.5"), None, b"invalid literal for int()"),
                                ((*window, "-O", "both"), None, b"-O must be one of covered, core"),
                                ((*window, "-O", ""), None, b"-O must be one of covered, core"),
                                ((*window, "-s", "1,,2"), None, b"does not parse"),
                                ((*window, "-s", "3-1"), None, b"a range runs upwards"),
                                ((*window, "-s", "0,1"), None, b"names annot 0, outside [1, 4]"),
                                ((*window, "-s", "1-5"), None, b"names annot 5, outside [1, 4]"),
                                ((*window, "-s", "2,2"), None, b"names annot 2 twice"),
                                ((*window, "-i", "one"), None, b"does not parse"),
                                ((*window, "-i", "0"), None, b"names annot 0, outside [1, 4]"),
                                ((*window, "-i", "3,1,3"), None, b"names annot 3 twice"),
                                ((*window, "-i", "1,2", "-m", "1"), None, b"-m 1 is below the 2 seeds"),
                                ((*window, "-m", "-1"), None, b"-m must be an integer in [0, 2048]"),
                                ((*window, "-m", "few"), None, b"-m must be an integer in [0, 2048]"),
                                ((*window, "-f", "1.5"), None, b"-f must lie in [0, 1]"),
                                ((*window, "-f", "-0.1"), None, b"-f must lie in [0, 1]"),
                                ((*window, "-f", "most"), None, b"-f 'most' is not a number"),
                                (("-n", "5", "-r", "ref_1:20-0"), None, b"negative dimensions"),
                                (("-n", "5", "-r", "ref_1"), None, b"memo panel: "),
                                ((*window, "-g", str(four)), None, b"names 4 genomes, -n says 5"),
                                ((*window, "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list")):
        r = _memo("panel", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - panel\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo panel: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same commands with nothing to refuse do reach the library, which is not there
    for extra in (("-r", "ref_1:0-20", "-n", "4", "-g", str(four)), (*window, "-i", "1,2", "-m", "2", "-f", "0.5", "-s", "3-4", "-O", "core")):
        r = _memo("panel", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo panel: " in r.stderr
    # an empty window needs no library: an empty file
    r = _memo("panel", *common, "-r", "ref_1:7-7", "-n", "5")
    assert (r.returncode, r.stderr) == (0, b"") and open(out, "rb").read() == b""
    assert sorted(os.listdir(tmp_path)) == ["four.txt", "never.tsv"]


# ---------------------------------------------------------------------------------------
# the names
# ---------------------------------------------------------------------------------------
NEW = ("memo_panel_planes_dev", "memo_panel_begin_dev", "memo_panel_score_dev", "memo_panel_take_dev", "memo_panel_tile", "memo_panel_pass_words")


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, panel
    assert memo_amd.region_panel is panel.region_panel and memo_amd.panel is panel and "region_panel" in dir(memo_amd)
    assert set(NEW) <= set(_lib.SYMBOLS) and "memo_debug_panel_times" in _lib.DEBUG_SYMBOLS and "memo_debug_panel_times" not in _lib.SYMBOLS
    src = open(EXE).read()
    assert '"panel"' in src and "memo_amd/panel_cli.py" in src
    assert "memo_panel.o" in open(os.path.join(ROOT, "memo_amd", "csrc", "Makefile")).read()


def test_the_new_symbols_of_the_libraries_against_the_headers():
    """nm -D: the product library exports the six names the header declares beside memo_collect_dev, with the argument counts the
    binding gives them; the switch lives in the A/B library alone"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()

    def exported(path):
        txt = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in txt.splitlines() if "memo_" in ln and "panel" in ln}

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return {name: args for name, args in re.findall(r"\b(memo_[a-z_0-9]*panel[a-z_0-9]*)\s*\(([^)]*)\)", src)}
    product, debug = declared("memo_amd_dap.h"), declared("memo_amd_debug.h")
    assert set(product) == set(NEW) and set(debug) == {"memo_debug_panel_times"}
    assert exported(_lib.SO_PATH) == set(NEW)
    assert exported(_lib.AB_SO_PATH) == set(NEW) | {"memo_debug_panel_times"}
    for name, args in {**product, **debug}.items():
        count = 0 if args.strip() == "void" else args.count(",") + 1
        assert count == len({**_lib.SYMBOLS, **_lib.DEBUG_SYMBOLS}[name][1]), name
    text = open(os.path.join(ROOT, "include", "memo_amd_dap.h")).read()
    assert text.index("int memo_collect_dev(") < text.index("int memo_panel_planes_dev(") < text.index("int memo_tracks_dev(")
