"""`memo spectrum` without a GPU: the definition itself (tests/spectrum_oracle.py) against the restated reference
(oracle.memo_oracle.np_conservation / np_membership) on the golden windows whose rows have end >= start, the README example's numbers,
the cumulative form against lengths_oracle.kth, and the command line (usage bytes, getopts handling, every refusal before the library
is even loaded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import lengths_oracle, spectrum_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")

KS = tuple(range(1, 40)) + (64, 65, 101, 257, 299)
KMAX = 300
LEGAL = sorted({c["index"] for c in G.cases(raises=False)} - {"rnd_negoverlap.parquet"})          # every row has end >= start


def windows_of(index, membership):
    return sorted({(c["region"], c["n"]) for c in G.cases(raises=False, membership=membership) if c["index"] == index})


def test_the_golden_windows_the_promise_is_checked_on():
    """the 164 windows that do not raise on the golden indexes whose rows all have end >= start, each taken in the
    mode of its index: 83 on conservation indexes, and the 81 on membership indexes that 10.7 uses"""
    assert sum(len(windows_of(i, False)) for i in LEGAL) == 83
    assert sum(len(windows_of(i, True)) for i in LEGAL) == 81
    assert len({(c["index"], c["region"], c["n"], c["membership"]) for c in G.cases(raises=False) if c["index"] in LEGAL}) == 164


@pytest.mark.parametrize("index", LEGAL)
def test_exact_is_the_bincount_of_the_query_at_every_k(index):
    from oracle import memo_oracle as O
    for membership in (False, True):
        for region, n in windows_of(index, membership):
            rec, se = region.split(":")
            qs, qe = map(int, se.split("-"))
            s, e, a = G.index_columns(index, rec)
            got = spectrum_oracle.exact(s, e, a, qs, qe, n, KMAX, membership)
            assert got.shape == (KMAX, n + 1) and (got.sum(axis=1) == qe - qs).all()
            for k in KS:
                f = (s > qs) & (s < qe + k)                          # the reference's own filter (memo_query.py:25-27 with main's + k)
                if membership:
                    held = O.bits_to_matrix(O.np_membership(s[f], e[f], a[f], qs, qe, k, n), n).astype(np.int64).sum(axis=1)
                else:
                    held = O.np_conservation(s[f], e[f], a[f], qs, qe, k, n).astype(np.int64)
                want = np.bincount(held, minlength=n + 1)
                assert np.array_equal(got[k - 1], want), (index, region, membership, k)


def test_the_example_numbers():
    for index, membership in (("example_cons.parquet", False), ("example_memb.parquet", True)):
        s, e, a = G.index_columns(index, "ref_1")
        exact = spectrum_oracle.exact(s, e, a, 0, 20, 5, 128, membership)
        least = spectrum_oracle.atleast(exact)
        assert least.shape == (128, 5)
        assert least[3 - 1][5 - 1] == 8 and least[3 - 1][3 - 1] == 20 and least[4 - 1][3 - 1] == 12 and least[4 - 1][5 - 1] == 1, index
        assert (least[:, 0] == 20).all() or not membership            # the pivot holds its own k-mers at every k
        assert (exact.sum(axis=1) == 20).all()
    # the two index kinds give one table
    cs, ms = (G.index_columns(i, "ref_1") for i in ("example_cons.parquet", "example_memb.parquet"))
    assert np.array_equal(spectrum_oracle.exact(*cs, 0, 20, 5, 40, False), spectrum_oracle.exact(*ms, 0, 20, 5, 40, True))


def test_atleast_is_a_count_over_the_kth_largest():
    rng = np.random.default_rng(7)
    for n, L, kmax in ((1, 9, 4), (5, 40, 12), (9, 33, 1), (33, 70, 50)):
        qs = 100
        s = rng.integers(qs - 5, qs + L + kmax + 5, 6 * L)
        e = s + rng.integers(0, 2 * kmax, len(s))
        a = rng.integers(-1, n + 1, len(s))
        exact = spectrum_oracle.exact(s, e, a, qs, qs + L, n, kmax, True)
        least = spectrum_oracle.atleast(exact)
        for t in range(1, n + 1):
            kth = lengths_oracle.kth(s, e, a, qs, qs + L, kmax, n, t).astype(np.int64)
            assert least[:, t - 1].tolist() == [int((kth >= k).sum()) for k in range(1, kmax + 1)], (n, t)
        from memo_amd import spectrum
        assert np.array_equal(spectrum.atleast(exact), least)
        assert spectrum.emit(exact) == spectrum_oracle.text(exact) and spectrum.emit(exact, True) == spectrum_oracle.text(exact, True)
    assert spectrum_oracle.text(np.array([[1, 0, 2], [3, 0, 0]])) == b"k\t0\t1\t2\n1\t1\t0\t2\n2\t3\t0\t0\n"
    assert spectrum_oracle.text(np.array([[1, 0, 2], [3, 0, 0]]), True) == b"k\t1\t2\n1\t2\t2\n2\t0\t0\n"


def test_the_oracle_on_a_hand_made_column():
    # three genomes, one position each pattern; kmax = 4
    planes = np.array([[4, 0, 3, 9], [4, 0, 1, 2], [4, 0, 2, 0]], np.uint32)
    memb = spectrum_oracle.table(planes, 4, True)
    #          v = 0  1  2  3
    assert memb.tolist() == [[1, 0, 1, 2],      # k = 1: the values >= 1 per column: 3, 0, 3, 2
                             [1, 0, 2, 1],      # k = 2: 3, 0, 2, 2
                             [1, 2, 0, 1],      # k = 3: 3, 0, 1, 1
                             [2, 1, 0, 1]]      # k = 4: 3, 0, 0, 1 (the 9 is taken as 4)
    cons = spectrum_oracle.table(planes, 4, False)
    # running minima down the planes: column 2 is 3, 1, 1; column 3 is 4, 2, 0
    assert cons[0].tolist() == [1, 0, 1, 2] and cons[1].tolist() == [1, 1, 1, 1] and cons[2].tolist() == [1, 2, 0, 1] and cons[3].tolist() == [2, 1, 0, 1]


@pytest.mark.parametrize("n", (1, 2, 5, 33))
def test_the_table_by_rank_is_the_table(n):
    """the fast form the many-tile GPU tests compare with (tests/test_many_tiles_gpu.py) against the definition, in both modes"""
    from tests.test_spectrum_gpu import PATTERNS, pattern_values
    above = 0
    for kmax in (1, 2, 31, 256):
        rng = np.random.default_rng([n, kmax])
        values = pattern_values(rng, n, 257, kmax, shift=kmax)
        assert 257 > 2 * PATTERNS                                     # (every pattern, the bit widths above KMAX too, many times)
        above += int((values > kmax).sum())
        for membership in (False, True):
            for L in (0, 1, 257):
                want = spectrum_oracle.table(values[:, :L], kmax, membership)
                got = spectrum_oracle.table_by_rank(values[:, :L], kmax, membership)
                assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape == (kmax, n + 1)
                assert np.array_equal(got, want), (n, kmax, membership, L)
                assert (got.sum(axis=1) == L).all()
    assert above > 50                                                 # (values above KMAX are taken as KMAX by both)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def test_usage_bytes():
    from memo_amd import spectrum_cli
    usage = _fixture("memo_spectrum_usage.txt")
    assert usage == spectrum_cli.USAGE.encode() and usage.startswith(b"\nMEMO spectrum - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("spectrum", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"  -m  ", b"-K [INT]", b"  -c  "):
        assert flag in usage
    assert b"-k " not in usage and b"-t " not in usage


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_spectrum_usage.txt")
    r = _memo("spectrum", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("spectrum", "-n", "5", "-K")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- K\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"spectrum" not in _fixture("memo_usage.txt")       # the reference's text: the sub-command is documented in the README
    assert _memo("lengths").stdout == _fixture("memo_lengths_usage.txt")          # `memo lengths` is as it was


def test_refusals_before_the_library_is_touched(tmp_path):
    """(-b names no file and the library path names none: a refusal that came later would be another message)"""
    out = str(tmp_path / "never.tsv")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-o", out)
    for extra, env, message in ((("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5", "-m"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-n", "five"), None, b"invalid literal for int()"),
                                (("-n", "0"), None, b"-n must be in [1, 2048]"),
                                (("-n", "2049"), None, b"-n must be in [1, 2048]"),
                                (("-n", "2049", "-m", "-c"), None, b"-n must be in [1, 2048]"),
                                (("-n", "5", "-K", "0"), None, b"-K must be an integer in [1, 1024]"),
                                (("-n", "5", "-m", "-K", "1025"), None, b"-K must be an integer in [1, 1024]"),
                                (("-n", "5", "-K", "2.5"), None, b"-K must be an integer in [1, 1024]"),
                                (("-n", "5", "-c", "-K", "many"), None, b"-K must be an integer in [1, 1024]"),
                                (("-n", "5"), {"MEMO_LENGTHS_SLICE": "0"}, b"MEMO_LENGTHS_SLICE must be an integer")):
        r = _memo("spectrum", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - spectrum\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo spectrum: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    for extra in (("-n", "5"), ("-n", "2048", "-m", "-K", "1024"), ("-n", "5", "-c", "-K", "1")):
        r = _memo("spectrum", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo spectrum: " in r.stderr
        assert b"must be" not in r.stderr
    assert os.listdir(tmp_path) == []


def test_missing_flags_are_named():
    r = _memo("spectrum", "-b", "x.parquet", "-K", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - spectrum\n" and r.stderr == b"memo spectrum: -r, -n, -o required\n"
    r = _memo("spectrum", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-m")
    assert r.returncode == 2 and r.stderr == b"memo spectrum: -b required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, spectrum
    assert memo_amd.spectrum is spectrum and memo_amd.region_exact is spectrum.region_exact
    assert all(callable(f) for f in (spectrum.table, spectrum.exact, spectrum.region_exact, spectrum.atleast, spectrum.tile))
    new = {"memo_spectrum_scratch_bytes", "memo_spectrum_begin_dev", "memo_spectrum_add_dev", "memo_spectrum_finish_dev", "memo_spectrum_tile"}
    assert new <= set(_lib.SYMBOLS) and "memo_debug_spectrum_times" in _lib.DEBUG_SYMBOLS and "memo_debug_spectrum_times" not in _lib.SYMBOLS
    for bad in (dict(kmax=0), dict(kmax=1025), dict(n_docs=0), dict(n_docs=2049)):
        with pytest.raises(ValueError):
            spectrum.exact([], [], [], 0, 10, **{"n_docs": 3, "kmax": 5, "membership": True, **bad})
