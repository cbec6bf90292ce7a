"""`memo pairs` without a GPU: the definition (tests/pairs_oracle.py) against the restated reference on the golden membership windows
-- at one k it is `memo matrix`'s matrix, over a range of k the sum of them --, the worked example of DESIGN.md 10.16, the distances,
the usage bytes, and every refusal that never reaches the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import lengths_oracle
from tests import pairs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1

EXAMPLE = {(3, 3): [[20, 10, 16, 20, 18], [10, 10, 8, 10, 8], [16, 8, 16, 16, 16], [20, 10, 16, 20, 18], [18, 8, 16, 18, 18]],
           (4, 4): [[20, 2, 12, 12, 6], [2, 2, 1, 1, 1], [12, 1, 12, 10, 5], [12, 1, 10, 12, 3], [6, 1, 5, 3, 6]],
           (1, 8): [[160, 52, 82, 83, 64], [52, 52, 49, 51, 49], [82, 49, 82, 72, 61], [83, 51, 72, 83, 61], [64, 49, 61, 61, 64]],
           (3, 8): [[120, 12, 42, 43, 24], [12, 12, 9, 11, 9], [42, 9, 42, 32, 21], [43, 11, 32, 43, 21], [24, 9, 21, 21, 24]]}


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def usable_windows():
    """the membership goldens that do not raise and whose index has only rows with end >= start"""
    out = []
    for c in G.cases(raises=False, membership=True):
        rec, qs, qe = G.region(c)
        s, e, _ = G.index_columns(c["index"], rec)
        if (e >= s).all():
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------
def test_the_oracle_on_hand_made_planes():
    v = [[9, 9, 9, 9], [0, 1, 2, 3], [5, 0, 7, 2]]
    assert O.weights(v, 1, 9).tolist() == v and O.weights(v, 1, 4).tolist() == [[4, 4, 4, 4], [0, 1, 2, 3], [4, 0, 4, 2]]
    assert O.weights(v, 3, 6).tolist() == [[4, 4, 4, 4], [0, 0, 0, 1], [3, 0, 4, 0]]
    assert O.weights(v, 2, 2).tolist() == [[1, 1, 1, 1], [0, 0, 1, 1], [1, 0, 1, 1]]
    assert O.sums(v, 1, 9).tolist() == [[36, 6, 14], [6, 6, 4], [14, 4, 14]]
    assert O.sums(v, 3, 6).tolist() == [[16, 1, 7], [1, 1, 0], [7, 0, 7]]
    got = O.sums(np.full((2, 3), CAP_MAX), 1, CAP_MAX)
    assert got.dtype == np.uint64 and got.tolist() == [[3 * CAP_MAX] * 2] * 2
    assert O.sums(np.zeros((3, 0), np.int64), 1, 5).tolist() == [[0] * 3] * 3


def _membership_matrix(s, e, a, qs, qe, k, n):
    """`memo matrix -k k` on the restated reference: the co-occurrence of its membership bits"""
    from oracle import memo_oracle
    f = (s > qs) & (s < qe + k)                                    # the reference's own filter (memo_query.py:25-27 with main's + k)
    bits = memo_oracle.bits_to_matrix(memo_oracle.np_membership(s[f], e[f], a[f], qs, qe, k, n), n).astype(np.int64)      # [L, N]
    return (bits.T @ bits).astype(np.uint64)


def test_identities_1_and_2_on_the_golden_windows():
    """S(k, k) is `memo matrix -k k`'s matrix; S(kmin, kmax) is the sum of them over k"""
    windows = usable_windows()
    assert len(G.cases(raises=False, membership=True)) == 151 and len(windows) == 139
    seen = set()
    for c in windows:
        rec, qs, qe = G.region(c)
        key = (c["index"], rec, qs, qe, c["n"])
        if key in seen:                                            # (the goldens ask several k of one window)
            continue
        seen.add(key)
        n = c["n"]
        s, e, a = G.index_columns(c["index"], rec)
        ks = sorted({1, 3, 8, 31, int(c["k"])})
        at = {k: _membership_matrix(s, e, a, qs, qe, k, n) for k in set(ks) | set(range(1, 9))}
        planes = lengths_oracle.planes(s, e, a, qs, qe, max(ks) + 300, n)    # (a cap above every k asked: the clamp to kmax is the oracle's)
        for k in ks:
            got = O.sums(planes, k, k)
            assert np.array_equal(got, at[k]), (key, k)
            assert np.array_equal(got, O.window_sums(s, e, a, qs, qe, k, k, n)), (key, k)
        for kmin, kmax in ((1, 8), (3, 8)):
            want = sum(at[k] for k in range(kmin, kmax + 1))
            assert np.array_equal(O.window_sums(s, e, a, qs, qe, kmin, kmax, n), want), (key, kmin, kmax)
        whole = O.window_sums(s, e, a, qs, qe, 1, 300, n)
        assert np.array_equal(whole, whole.T) and np.array_equal(whole[0], np.diag(whole)) and whole[0, 0] == 300 * (qe - qs)
    assert len(seen) >= 40


def test_the_worked_example_from_the_goldens():
    """ref_1:0-20 of the example index, N = 5: the tables of the README and of DESIGN.md 10.16"""
    from tests import breaks_oracle
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    for (kmin, kmax), want in EXAMPLE.items():
        assert O.window_sums(s, e, a, 0, 20, kmin, kmax, 5).tolist() == want, (kmin, kmax)
    assert np.diag(np.array(EXAMPLE[(3, 3)])).tolist() == [20, 10, 16, 20, 18]                 # `memo matrix -k 3`'s diagonal
    sums8 = breaks_oracle.window_table(s, e, a, 0, 20, np.array([0, 20]), 8, 5)[1, :, 0]       # identity 3: `memo breaks -m -s -B 1 -K 8`
    assert np.diag(np.array(EXAMPLE[(1, 8)])).tolist() == sums8.tolist() == [160, 52, 82, 83, 64]
    top = O.window_sums(s, e, a, 0, 20, 1, CAP_MAX, 5)
    assert top[1:, 1:].tolist() == [row[1:] for row in EXAMPLE[(1, 8)][1:]]
    assert top[0, 0] == 42949672940 == 20 * CAP_MAX and top[0, 1:].tolist() == np.diag(top)[1:].tolist() == [52, 82, 83, 64]


def test_the_distances_go_through_matrix_jaccard():
    from memo_amd import matrix, pairs
    s8 = np.array(EXAMPLE[(1, 8)], np.uint64)
    d = matrix.jaccard(s8)
    assert np.round(d[1], 4).tolist() == [0.675, 0.0, 0.4235, 0.3929, 0.2687] and round(float(d[2, 3]), 4) == 0.2258
    assert np.array_equal(d, d.T) and (np.diag(d) == 0).all()
    w = O.weights(lengths_oracle.planes(*G.index_columns("example_memb.parquet", "ref_1"), 0, 20, 8, 5), 1, 8)
    for g in range(5):                                             # max = a + b - min: 1 - sum of min / sum of max
        for h in range(5):
            assert d[g, h] == 1.0 - np.minimum(w[g], w[h]).sum() / np.maximum(w[g], w[h]).sum()
    for x in range(5):                                             # a metric: the triangle inequality on the example
        for y in range(5):
            for z in range(5):
                assert d[x, z] <= d[x, y] + d[y, z] + 1e-15
    mean = pairs.mean_lengths(s8, 20)
    assert mean.dtype == np.float64 and mean[0].tolist() == [8.0, 2.6, 4.1, 4.15, 3.2]
    assert matrix.format_matrix(mean[:2, :2]) == "8.0\t2.6\n2.6\t2.6\n"


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import pairs_cli
    usage = pairs_cli.USAGE.encode()
    assert usage.startswith(b"\nMEMO pairs - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("pairs", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-l [INT]", b"-K [INT]", b"  -j  ", b"  -f  ", b"-g [FILE]",
                 b"[1]", b"[2147483647]", b"33554431"):
        assert flag in usage
    assert b"-k" not in usage and b"MEMBERSHIP" in usage and b"conservation index" in usage
    r = _memo("pairs", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("pairs", "-k", "31")                                    # no -k, as for `memo maxk`
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("pairs", "-b")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- b\n")
    r = _memo("pairs", "-b", "x.parquet", "-K", "8")
    assert r.returncode == 2 and r.stdout == b"MEMO - pairs\n" and r.stderr == b"memo pairs: -r, -n, -o required\n"
    r = _memo("pairs", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-j")
    assert r.returncode == 2 and r.stderr == b"memo pairs: -b required\n"


def test_the_other_sub_commands_print_what_they_printed():
    """`memo`, `memo -h` and `memo bogus` keep the reference's bytes, `memo matrix` its usage and its -k default"""
    from memo_amd import matrix_cli
    fixture = lambda name: open(os.path.join(G.GOLD, "cli", name), "rb").read()      # noqa: E731
    for argv, name in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == fixture(name), argv
    assert b"pairs" not in fixture("memo_usage.txt")
    assert _memo("matrix").stdout == fixture("memo_matrix_usage.txt") == matrix_cli.USAGE.encode()
    assert matrix_cli.cli.defaults == {"-k": "31"}


def test_names_are_exported():
    import memo_amd
    from memo_amd import _lib, pairs
    assert memo_amd.region_pairs is pairs.region_pairs and memo_amd.plane_sums is pairs.plane_sums and memo_amd.pairs is pairs
    assert {"memo_pairs_dev", "memo_pairs_tile", "memo_pairs_chunk", "memo_pairs_narrow_span"} <= set(_lib.SYMBOLS)
    assert "memo_debug_pairs_times" in _lib.DEBUG_SYMBOLS and "memo_debug_pairs_times" not in _lib.SYMBOLS
    src = open(EXE).read()
    assert '"pairs"' in src and "memo_amd/pairs_cli.py" in src


def test_refusals_before_the_library_is_touched(tmp_path):
    """exit status 1, one message, nothing written (-b names no file and the library path names none: a refusal that came later
    would be another message)"""
    out = str(tmp_path / "never.tsv")
    four = tmp_path / "four.txt"
    four.write_text("a.fa\n\nb.fa\nc.fa\n  \nd.fa\n")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-o", out)
    for extra, env, message in ((("-n", "5", "-j", "-f"), None, b"-j cannot be combined with -f"),
                                (("-n", "0"), None, b"-n must be an integer in [1, 2048]"),
                                (("-n", "2049"), None, b"-n must be an integer in [1, 2048]"),
                                (("-n", "five"), None, b"-n must be an integer in [1, 2048]"),
                                (("-n", "5", "-K", "0"), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-K", "2147483648"), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-K", "3.5"), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-l", "0"), None, b"-l must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-l", "x"), None, b"-l must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-K", "7", "-l", "8"), None, b"-l must be an integer in [1, 7]"),
                                (("-n", "5", "-g", str(four)), None, b"names 4 genomes, -n says 5"),
                                (("-n", "5", "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                                (("-n", "5", "-r", "ref_1:20-0"), None, b"negative dimensions"),
                                (("-n", "5", "-r", "ref_1"), None, b"memo pairs: "),
                                (("-n", "5", "-r", "ref_1:-3-20"), None, b"memo pairs: "),
                                (("-n", "5", "-r", f"ref_1:0-{2 ** 31}"), None, f"at most {2 ** 31 - 1} positions".encode()),
                                (("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch")):
        r = _memo("pairs", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - pairs\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo pairs: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    r = _memo("pairs", *common, "-n", "4", "-g", str(four), "-K", "8", "-l", "3", "-j")
    assert r.returncode == 1 and not os.path.exists(out)
    assert b"Traceback" in r.stderr or b"memo pairs: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["four.txt"]


def test_the_driver_refuses_before_any_device_call(monkeypatch):
    from memo_amd import _lib, pairs

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(pairs, "lib", never)
    for kw, message in ((dict(kmax=0), "kmax must be in"), (dict(kmax=2 ** 31), "kmax must be in"), (dict(kmin=0), "kmin must be in"),
                        (dict(kmax=7, kmin=8), r"kmin must be in \[1, 7\]"), (dict(kmin=2 ** 31), "kmin must be in")):
        with pytest.raises(ValueError, match=message):
            pairs.region_pairs("no.parquet", "ref_1:0-20", 5, **kw)
        with pytest.raises(ValueError, match=message):
            pairs.plane_sums(np.zeros((2, 4), np.uint32), **{"kmax": 9, **kw})
    for n in (0, 2049):
        with pytest.raises(ValueError, match=r"n_docs must be in \[1, 2048\]"):
            pairs.region_pairs("no.parquet", "ref_1:0-20", n)
    with pytest.raises(ValueError, match="negative dimensions"):
        pairs.region_pairs("no.parquet", "ref_1:20-0", 5)
    with pytest.raises(ValueError):                                                            # (a window string cannot spell qs < 0)
        pairs.region_pairs("no.parquet", "ref_1:-5-20", 5)
    with pytest.raises(ValueError, match=f"at most {2 ** 31 - 1} positions"):
        pairs.region_pairs("no.parquet", f"ref_1:0-{2 ** 31}", 5)
    with pytest.raises(ValueError, match=r"cells must be \[planes, L\]"):
        pairs.plane_sums(np.zeros(4, np.uint32), kmax=9)
    empty = pairs.region_pairs("no.parquet", "ref_1:5-5", 5)                                   # an empty window touches nothing
    assert empty.shape == (5, 5) and empty.dtype == np.uint64 and not empty.any()
