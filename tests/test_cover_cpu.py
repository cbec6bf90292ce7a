"""`memo cover` without a GPU: the oracle (tests/cover_oracle.py) against every row of the worked tables (tests/cover_tables.py) from
the goldens, against the oracle of `memo panel` at kmin = kmax = k and against the bit form summed over k, the host's lazy choice
against the eager one on NumPy weights, the text against literals, the command line as far as it goes without the library, and the
new symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from memo_amd import cover as _cover  # noqa: F401  (the oracle's tests too belong to the sub-command: none of them runs without it)
from tests import cover_oracle as C
from tests import cover_tables as T
from tests import golden_util as G
from tests import lengths_oracle
from tests import panel_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
GOLDENS = {"example": ("example_memb.parquet", "ref_1", 0, 20, 5), "rnd40": ("rnd_n40.parquet", "chr1", 0, 2100, 40)}


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def oracle_kw(kw):
    """region_cover's flags as the oracle takes them"""
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


def span_of(kw):
    kmin, kmax = kw.get("kmin", 1), kw.get("kmax", CAP_MAX)
    return kmin, kmax, kmax - kmin + 1


@pytest.fixture(scope="module")
def lengths():
    """the goldens' match lengths uncapped (a cap commutes with the weights' own), computed once"""
    out = {}
    for name, (index, record, qs, qe, n) in GOLDENS.items():
        out[name] = lengths_oracle.planes(*G.index_columns(index, record), qs, qe, CAP_MAX, n)
        out[name].setflags(write=False)
    return out


def golden_rows(lengths, name, kw):
    kmin, kmax, span = span_of(kw)
    return C.rows(C.greedy(C.weights(lengths[name], kmin, kmax), span, **oracle_kw(kw)))


# ---------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------
def test_the_example_tables(lengths):
    for kw, total, want in T.EXAMPLE:
        assert golden_rows(lengths, "example", kw) == want and total == 20 * span_of(kw)[2], kw
    W = C.weights(lengths["example"], 1, 8)
    assert {g: int(W[g].sum()) for g in T.EXAMPLE_DIAGONAL} == T.EXAMPLE_DIAGONAL
    assert int(W[0].sum()) == 160                                                    # nothing bounds the pivot: the cap everywhere


def test_the_rnd_n40_tables(lengths):
    for kw, begins, first, last in T.RND40:
        got = golden_rows(lengths, "rnd40", kw)
        assert len(got) == 39 and [r[0] for r in got[:12]] == begins and got[:len(first)] == first and got[-1] == last, kw
    for kw, want in T.RND40_STOPS:
        assert len(golden_rows(lengths, "rnd40", kw)) == want, kw
    assert 2100 * 64 == 134400


def test_one_k_is_the_panel_oracle_on_the_membership_bits(lengths):
    """kmin = kmax = k: the weights are `memo query -m -k k`'s bits, and every row of the greedy is panel's"""
    from oracle import memo_oracle
    from tests import collect_oracle
    for name, (index, record, qs, qe, n) in GOLDENS.items():
        s, e, o = G.index_columns(index, record)
        for k in (3, 4, 5, 8, 12, 31):
            B = collect_oracle.unpack(memo_oracle.np_membership(*memo_oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n), n)
            W = C.weights(lengths[name], k, k)
            assert np.array_equal(W[1:].T, B[:, 1:].astype(np.int64)), (name, k)
            for kw in (dict(), dict(objective="core"), dict(seeds=[2, 1]), dict(most=3), dict(fraction="0.5")):
                assert C.greedy(W, 1, **kw) == panel_oracle.greedy(B, **kw), (name, k, kw)


def test_scores_are_the_bit_form_summed_over_k():
    """on seeded random lengths and any state the greedy can reach, new and kept are panel's new and kept at every k of
    [kmin, kmax], added up; so are the sums of core and covered"""
    rng = np.random.default_rng(20261021)
    for i in range(40):
        N, L = int(rng.integers(2, 9)), int(rng.integers(1, 60))
        kmin = int(rng.integers(1, 8))
        kmax = kmin + int(rng.integers(0, 12))
        span = kmax - kmin + 1
        lens = rng.integers(0, kmax + 6, (N, L))
        W = C.weights(lens, kmin, kmax)
        taken = [int(g) for g in rng.permutation(N)[:int(rng.integers(0, N))]]
        core, covered = np.full(L, span, np.int64), np.zeros(L, np.int64)
        for g in taken:
            core, covered = np.minimum(core, W[g]), np.maximum(covered, W[g])
        bits = {k: lens >= k for k in range(kmin, kmax + 1)}                      # bit g of `memo query -m -k k`
        core_k = {k: np.all(bits[k][taken], axis=0) for k in bits}
        covered_k = {k: np.any(bits[k][taken], axis=0) for k in bits}
        assert int(core.sum()) == sum(int(v.sum()) for v in core_k.values()) and int(covered.sum()) == sum(int(v.sum()) for v in covered_k.values())
        for g in range(N):
            new = sum(int((bits[k][g] & ~covered_k[k]).sum()) for k in bits)
            kept = sum(int((bits[k][g] & core_k[k]).sum()) for k in bits)
            assert C.scores(W[g], core, covered) == (new, kept), (i, g)


# ---------------------------------------------------------------------------------------
# the host's choice
# ---------------------------------------------------------------------------------------
def numpy_state(W, span):
    """score and take of panel.greedy on NumPy vectors, and the lists every call of score was made with"""
    W = np.asarray(W, np.int64)
    state = {"core": np.full(W.shape[1], span, np.int64), "covered": np.zeros(W.shape[1], np.int64), "calls": []}

    def score(genomes):
        state["calls"].append(list(genomes))
        return [list(C.scores(W[g], state["core"], state["covered"])) for g in genomes]

    def take(g):
        state["core"], state["covered"] = np.minimum(state["core"], W[g]), np.maximum(state["covered"], W[g])
        return int(state["core"].sum()), int(state["covered"].sum())
    return score, take, state


def test_lazy_equals_eager_and_the_oracle_on_random_weights():
    from memo_amd import panel
    rng = np.random.default_rng(20261022)
    spared = 0
    for i in range(100):
        L, N = int(rng.integers(1, 200)), int(rng.integers(2, 30))
        span = int(rng.choice([1, 7, 64, 65535, 65536, CAP_MAX]))
        W = rng.integers(0, span + 1, (N, L))
        if i % 3 == 0:
            W[rng.integers(1, N, 3)] = W[1]                                            # duplicate planes: ties
        if i % 4 == 0:
            W[rng.integers(1, N)] = 0                                                  # an all-zero plane
        W[0] = span
        objective = ("covered", "core")[i % 2]
        everyone = list(range(1, N))
        seeds = [int(g) for g in rng.permutation(everyone)[:int(rng.integers(0, 3))]] if i % 5 == 0 else []
        cand = [int(g) for g in rng.permutation(everyone)[:int(rng.integers(1, N))]] if i % 7 == 0 else everyone
        if i % 10 == 9:
            cand = [int(rng.integers(1, N))]                                           # a lone candidate
        cand = [g for g in cand if g not in seeds]
        most = None if i % 6 else len(seeds) + int(rng.integers(0, 4))
        fraction = None if i % 9 else "0.9"
        want = C.greedy(W, span, objective, cand, seeds, most, fraction)
        stop_at = panel.threshold(fraction, L * span)
        got = {}
        for lazy in (True, False):
            score, take, state = numpy_state(W, span)
            got[lazy] = panel.greedy(score, take, L * span, cand, seeds, objective, most, stop_at, lazy=lazy)
            got[lazy, "scored"] = panel.planes_scored()
            assert got[lazy, "scored"] == sum(len(c) for c in state["calls"])
        assert got[True] == got[False] == want, i
        assert got[True, "scored"] <= got[False, "scored"] <= len(cand) * (len(cand) + 1) // 2
        spared += got[False, "scored"] - got[True, "scored"]
    assert spared > 0


def test_refusals_that_need_no_library(monkeypatch):
    from memo_amd import _device, _lib, cover

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(cover, "lib", never)
    monkeypatch.setattr(_device, "lib", never)
    assert cover.span_of() == (1, CAP_MAX, CAP_MAX) and cover.span_of(3, 8) == (3, 8, 6) and cover.span_of(5, 5) == (5, 5, 1)
    for args in ((0, 8), (9, 8), (1, 0), (1, 2 ** 31)):
        with pytest.raises(ValueError, match="must be in"):
            cover.span_of(*args)
    assert [cover.cell_bytes_of(s) for s in (1, 65535, 65536, CAP_MAX)] == [2, 2, 4, 4]
    assert cover.slice_step(5, 8) == 8 and cover.slice_step(5, 2104) == 2104 and cover.slice_step(40) % 8 == 0 and cover.slice_step(2048) >= 8
    for bad in (12, 0, -8, 7, 2101):
        with pytest.raises(ValueError, match="multiple of 8"):
            cover.region_cover("no.parquet", "ref_1:0-20", 5, slice_positions=bad)
    for kw, message in ((dict(kmin=0), "kmin must be in"), (dict(kmin=9, kmax=8), "kmin must be in"), (dict(kmax=2 ** 31), "kmax must be in"),
                        (dict(objective="both"), "objective must be one of"), (dict(candidates="0"), "names annot 0"), (dict(seeds="2,2"), "names annot 2 twice"),
                        (dict(seeds="1,2", max_genomes=1), "below the 2 seeds"), (dict(fraction="1.5", kmax=8), r"must lie in \[0, 1\]")):
        with pytest.raises(ValueError, match=message):
            cover.region_cover("no.parquet", "ref_1:0-20", 5, **kw)
    with pytest.raises(ValueError, match="n_docs must be in"):
        cover.region_cover("no.parquet", "ref_1:0-20", 1)
    with pytest.raises(ValueError, match="negative dimensions"):
        cover.region_cover("no.parquet", "ref_1:20-0", 5)
    with pytest.raises(ValueError, match="at most 2147483647 positions"):
        cover.region_cover("no.parquet", "ref_1:0-2147483648", 5)
    order, core, covered, L, span = cover.region_cover("no.parquet", "ref_1:5-5", 5, kmin=3, kmax=8)          # an empty window touches nothing
    assert (order.shape, core.shape, covered.shape, L, span) == ((0,), (0,), (0,), 0, 6) and order.dtype == np.uint16 and core.dtype == np.uint64
    assert cover.planes_scored() == 0


# ---------------------------------------------------------------------------------------
# the text
# ---------------------------------------------------------------------------------------
def test_format_against_literals():
    from memo_amd import collect, cover
    order, core, covered = (list(c) for c in zip(*T.EXAMPLE[2][2]))
    text = cover.format_cover(20, 8, order, core, covered)
    assert text == T.README_EXAMPLE
    assert text == collect.format_curves(160, np.array([core]), np.array([covered]), "curve", np.array([order]), ["0", "1", "2", "3", "4"])
    named = cover.format_cover(20, 8, np.array(order, np.uint16), np.array(core, np.uint64), np.array(covered, np.uint64), ["pivot", "g1", "g2", "g3", "g4"])
    assert named == "genomes\tcore\tcovered\tadded\n1\t160\t0\tpivot\n2\t83\t83\tg3\n3\t72\t93\tg2\n4\t59\t94\tg4\n5\t49\t95\tg1\n"
    assert cover.format_cover(20, CAP_MAX, order, core, covered).splitlines()[1] == "1\t42949672940\t0\t0"      # the default cap's pivot row
    assert cover.format_cover(20, 8, [], [], []) == "genomes\tcore\tcovered\tadded\n1\t160\t0\t0\n"             # -f 0 without seeds: the pivot alone
    big = (2 ** 31 - 1) ** 2
    assert cover.format_cover(CAP_MAX, CAP_MAX, [7], [big - 1], [big]) == f"genomes\tcore\tcovered\tadded\n1\t{big}\t0\t0\n2\t{big - 1}\t{big}\t7\n"
    assert cover.format_cover(0, 8, [], [], []) == "" and cover.format_cover(0, 8, [], [], [], ["p", "a"]) == ""    # an empty window: an empty file


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import cover_cli
    usage = cover_cli.USAGE.encode()
    assert usage == open(os.path.join(G.GOLD, "cli", "memo_cover_usage.txt"), "rb").read()
    assert usage.startswith(b"\nMEMO cover - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("cover", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-l [INT]", b"-K [INT]", b"-O [covered|core]", b"-s [LIST]", b"-i [LIST]",
                 b"-m [INT]", b"-f [FRACTION]", b"-g [FILE]", b"[2147483647]", b"[1]"):
        assert flag in usage
    assert b"-k [INT]" not in usage and b"MEMBERSHIP" in usage and b"nothing can tell" in usage
    r = _memo("cover", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("cover", "-n", "5", "-K")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- K\n")
    r = _memo("cover", "-b", "x.parquet", "-K", "8")
    assert r.returncode == 2 and r.stdout == b"MEMO - cover\n" and r.stderr == b"memo cover: -r, -n, -o required\n"
    r = _memo("cover", "-r", "ref_1:0-20", "-n", "5", "-o", "x")
    assert r.returncode == 2 and r.stderr == b"memo cover: -b required\n"
    for argv, fixture in (([], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):            # the reference's texts stay the reference's
        assert _memo(*argv).stdout == open(os.path.join(G.GOLD, "cli", fixture), "rb").read()


def test_refusals_before_the_library_is_touched(tmp_path):
    """exit status 1, one message, nothing written (-b names no file and the library path names none: a refusal that came later
    would be another message)"""
    out = str(tmp_path / "never.tsv")
    four = tmp_path / "four.txt"
    four.write_text("pivot.fa\ng1.fa\ng2.fa\ng3.fa\n")
    common = ("-b", str(tmp_path / "no.parquet"), "-o", out)
    window = ("-r", "ref_1:0-20", "-n", "5")
    for extra, env, message in ((window, {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (window, {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                ((*window, "-k", "31"), None, b"there is no -k"),
                                (("-r", "ref_1:0-20", "-n", "five"), None, b"-n must be an integer in [2, 2048]"),
                                (("-r", "ref_1:0-20", "-n", "1"), None, b"-n must be an integer in [2, 2048]"),
                                (("-r", "ref_1:0-20", "-n", "2049"), None, b"-n must be an integer in [2, 2048]"),
                                ((*window, "-K", "0"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-K", "2147483648"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-K", "many"), None, b"-K must be an integer in [1, 2147483647]"),
                                ((*window, "-l", "0"), None, b"-l must be an integer in [1, 2147483647]"),
                                ((*window, "-l", "9", "-K", "8"), None, b"-l must be an integer in [1, 8]"),
                                ((*window, "-f", "0.5"), None, b"-f needs -K"),
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
                                ((*window, "-K", "8", "-f", "1.5"), None, b"-f must lie in [0, 1]"),
                                ((*window, "-K", "8", "-f", "-0.1"), None, b"-f must lie in [0, 1]"),
                                ((*window, "-K", "8", "-f", "most"), None, b"-f 'most' is not a number"),
                                (("-n", "5", "-r", "ref_1:20-0"), None, b"negative dimensions"),
                                (("-n", "5", "-r", "ref_1"), None, b"memo cover: "),
                                ((*window, "-g", str(four)), None, b"names 4 genomes, -n says 5"),
                                ((*window, "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list")):
        r = _memo("cover", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - cover\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo cover: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    r = _memo("cover", *common, *window, "-k", "31")
    assert b"-l" in r.stderr and b"-K" in r.stderr                                   # the refusal of -k names what takes its place
    # the same commands with nothing to refuse do reach the library, which is not there
    for extra in (("-r", "ref_1:0-20", "-n", "4", "-g", str(four)), (*window, "-i", "1,2", "-m", "2", "-K", "8", "-f", "0.5", "-s", "3-4", "-O", "core", "-l", "3")):
        r = _memo("cover", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo cover: " in r.stderr
    # an empty window needs no library: an empty file
    r = _memo("cover", *common, "-r", "ref_1:7-7", "-n", "5")
    assert (r.returncode, r.stderr) == (0, b"") and open(out, "rb").read() == b""
    assert sorted(os.listdir(tmp_path)) == ["four.txt", "never.tsv"]


# ---------------------------------------------------------------------------------------
# the names
# ---------------------------------------------------------------------------------------
NEW = ("memo_cover_weights_dev", "memo_cover_begin_dev", "memo_cover_score_dev", "memo_cover_take_dev", "memo_cover_pass_cells")


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, cover
    assert memo_amd.region_cover is cover.region_cover and memo_amd.cover is cover and "region_cover" in dir(memo_amd)
    assert set(NEW) <= set(_lib.SYMBOLS) and "memo_debug_cover_times" in _lib.DEBUG_SYMBOLS and "memo_debug_cover_times" not in _lib.SYMBOLS
    src = open(EXE).read()
    assert '"cover"' in src and "memo_amd/cover_cli.py" in src
    assert "memo_cover.o" in open(os.path.join(ROOT, "memo_amd", "csrc", "Makefile")).read()


def test_the_new_symbols_of_the_libraries_against_the_headers():
    """nm -D: the product library exports the five names the header declares beside memo_panel_*, with the argument counts the
    binding gives them; the switch lives in the A/B library alone"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()

    def exported(path):
        txt = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in txt.splitlines() if "memo_" in ln and "cover" in ln}

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return {name: args for name, args in re.findall(r"\b(memo_[a-z_0-9]*cover[a-z_0-9]*)\s*\(([^)]*)\)", src)}
    product, debug = declared("memo_amd_dap.h"), declared("memo_amd_debug.h")
    assert set(product) == set(NEW) and set(debug) == {"memo_debug_cover_times"}
    assert exported(_lib.SO_PATH) == set(NEW)
    assert exported(_lib.AB_SO_PATH) == set(NEW) | {"memo_debug_cover_times"}
    for name, args in {**product, **debug}.items():
        count = 0 if args.strip() == "void" else args.count(",") + 1
        assert count == len({**_lib.SYMBOLS, **_lib.DEBUG_SYMBOLS}[name][1]), name
    text = open(os.path.join(ROOT, "include", "memo_amd_dap.h")).read()
    assert text.index("int memo_panel_take_dev(") < text.index("int memo_cover_weights_dev(") < text.index("int memo_tracks_dev(")
