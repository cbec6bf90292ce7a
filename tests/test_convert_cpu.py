"""`memo convert` without a GPU: the definition (tests/convert_oracle.py) against the golden indexes and the restated reference
(oracle.memo_oracle.np_conservation / np_membership), the command line (usage bytes, every refusal with the library pointed at a file
that is not there), and pass A's bookkeeping restated on the host against the definition of a slice's carry."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import convert_oracle
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
# the golden membership records whose rows all have end >= start: (index, record, N)
RECORDS = (("example_memb.parquet", "ref_1", 5), ("rnd_n4.parquet", "chrA", 4), ("rnd_n4.parquet", "chrB", 4), ("rnd_n8.parquet", "chr1", 8),
           ("rnd_n40.parquet", "chr1", 40), ("rnd_n40.parquet", "chr2", 40), ("rnd_n70_sparse.parquet", "chr1", 70),
           ("rnd_n130.parquet", "chr1", 130))
KS = (1, 2, 3, 4, 8, 31, 32, 33, 64, 65, 101, 257)


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def windows(L):
    """three windows inside [0, L]"""
    return ((0, L), (L // 3, L - L // 4), (max(L - 7, 0), L))


# ---------------------------------------------------------------------------------------
# the three facts the feature rests on, as tests of the oracle
# ---------------------------------------------------------------------------------------
def test_the_records_the_promise_is_checked_on():
    for index, rec, n in RECORDS:
        s, e, a = G.index_columns(index, rec)
        assert len(s) and (e >= s).all() and a.min() >= 1 and a.max() <= n - 1, (index, rec)


def test_the_example_converts_to_the_committed_indexes():
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    cons = convert_oracle.rows(s, e, a, 5, order=True)
    assert len(cons[0]) == 56 and all(np.array_equal(g, w) for g, w in zip(cons, G.index_columns("example_cons.parquet", "ref_1")))
    memb = convert_oracle.rows(s, e, a, 5, order=False)
    assert len(memb[0]) == 48 and all(np.array_equal(g, w) for g, w in zip(memb, (s, e, a)))


@pytest.mark.parametrize("index,rec,n", RECORDS)
def test_conservation_of_the_converted_rows_counts_the_membership_bits(index, rec, n):
    from oracle import memo_oracle as O
    s, e, a = G.index_columns(index, rec)
    cs, ce, ca = convert_oracle.rows(s, e, a, n, order=True)
    ms, me, ma = convert_oracle.rows(s, e, a, n, order=False)
    for qs, qe in windows(int(s.max())):
        for k in KS:
            bits = O.bits_to_matrix(O.np_membership(s, e, a, qs, qe, k, n), n)
            assert np.array_equal(O.np_conservation(cs, ce, ca, qs, qe, k, n), bits.sum(axis=1)), (index, rec, qs, qe, k)
            assert np.array_equal(O.bits_to_matrix(O.np_membership(ms, me, ma, qs, qe, k, n), n), bits), (index, rec, qs, qe, k)


def test_the_membership_round_trip_is_a_fixed_point_and_smaller():
    sizes = {}
    for index, rec, n in RECORDS:
        s, e, a = G.index_columns(index, rec)
        once = convert_oracle.rows(s, e, a, n, order=False)
        again = convert_oracle.rows(*once, n, order=False, length=int(s.max()))
        assert all(np.array_equal(g, w) for g, w in zip(again, once)), (index, rec)
        assert len(once[0]) <= len(s)
        sizes[(index, rec)] = (len(s), len(once[0]))
    assert sizes[("rnd_n4.parquet", "chrA")] == (503, 187) and sizes[("rnd_n40.parquet", "chr1")] == (60039, 8846)


def test_a_longer_record_than_the_largest_start():
    """with a length, the record ends where the length says: the rows close there, and they say the same lengths as the source rows"""
    s, e, a = G.index_columns("rnd_n4.parquet", "chrB")
    L = int(s.max())
    want = convert_oracle.ms(s, e, a, 4, L + 9)
    assert want.shape == (L + 9, 3) and (want[L:] == (9 - np.arange(9))[:, None]).all()      # nothing bounds the added positions
    for order in (False, True):
        longer = convert_oracle.rows(s, e, a, 4, order=order, length=L + 9)
        assert int(longer[0].max()) == L + 9
    assert np.array_equal(convert_oracle.ms(*convert_oracle.rows(s, e, a, 4, order=False, length=L + 9), 4), want)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def test_usage_bytes():
    from memo_amd import convert_cli
    usage = _fixture("memo_convert_usage.txt")
    assert usage == convert_cli.USAGE.encode() and usage.startswith(b"\nMEMO convert - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("convert", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-o [FILE]", b"  -m  ", b"-f [FILE]"):
        assert flag in usage
    r = _memo("convert", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("convert", "-b", "x", "-n")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- n\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"convert" not in _fixture("memo_usage.txt")       # the reference's text: the sub-command is documented in the README
    assert _memo("lengths").stdout == _fixture("memo_lengths_usage.txt")         # `memo lengths` is as it was


def test_missing_flags_are_named():
    r = _memo("convert", "-b", "x.parquet", "-m")
    assert r.returncode == 2 and r.stdout == b"MEMO - convert\n" and r.stderr == b"memo convert: -n, -o required\n"
    r = _memo("convert", "-n", "5", "-o", "x")
    assert r.returncode == 2 and r.stderr == b"memo convert: -b required\n"


def _write(path, f0, s, e, a):
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table({"f0": pa.array(f0, pa.utf8()), "f1": pa.array(s, pa.int64()), "f2": pa.array(e, pa.int64()),
                             "f3": pa.array(a, pa.int64())}), path)


def test_refusals_before_the_library_is_touched_and_before_anything_is_written(tmp_path):
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    out = str(tmp_path / "never.parquet")
    far = str(tmp_path / "far.parquet")
    _write(far, ["c", "c"], [5, 2 ** 31], [9, 2 ** 31 + 4], [1, 1])
    long = str(tmp_path / "long.parquet")
    _write(long, ["c", "c"], [5, 2 ** 30], [9, 2 ** 30 + 4], [1, 1])
    fai = str(tmp_path / "pivot.fa.fai")
    open(fai, "w").write("ref_1\t25\t7\t60\t61\nother\t100\t40\t60\t61\n")
    nofai = str(tmp_path / "other.fa.fai")
    open(nofai, "w").write("other\t100\t40\t60\t61\n")
    copy = str(tmp_path / "copy.parquet")
    with open(copy, "wb") as fh:
        fh.write(open(memb, "rb").read())
    before = sorted(os.listdir(tmp_path))
    for argv, env, message in ((("-b", memb, "-n", "5", "-o", out), {"WORLD_SIZE": "2"}, b"sharded launch"),
                               (("-b", memb, "-n", "5", "-o", out), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                               (("-b", memb, "-n", "five", "-o", out), None, b"invalid literal for int()"),
                               (("-b", memb, "-n", "1", "-o", out), None, b"-n must be in [2, 2048]"),
                               (("-b", memb, "-n", "2049", "-o", out, "-m"), None, b"-n must be in [2, 2048]"),
                               # a wrong -n: the first row whose annot does not fit is named
                               (("-b", memb, "-n", "4", "-o", out), None, b"has annot 4 outside [1, 3]"),
                               (("-b", memb, "-n", "4", "-o", out), None, b"-n value is probably wrong"),
                               (("-b", os.path.join(G.GOLD, "rnd_negoverlap.parquet"), "-n", "12", "-o", out), None, b"ends before it starts"),
                               (("-b", far, "-n", "2", "-o", out), None, b"above 2^31 - 1"),
                               (("-b", long, "-n", "2", "-o", out, "-m"), None, b"above 2^30 - 1"),
                               (("-b", memb, "-n", "5", "-o", out, "-f", fai), None, b"below its largest row start 26"),
                               (("-b", memb, "-n", "5", "-o", out, "-f", nofai), None, b"'ref_1'"),
                               (("-b", memb, "-n", "5", "-o", out, "-f", str(tmp_path / "no.fai")), None, b"no.fai"),
                               (("-b", copy, "-n", "5", "-o", copy), None, b"is the input file"),
                               (("-b", copy, "-n", "5", "-o", os.path.join(str(tmp_path), ".", "copy.parquet"), "-m"), None, b"is the input file"),
                               (("-b", str(tmp_path / "no.parquet"), "-n", "5", "-o", out), None, b"no.parquet"),
                               (("-b", memb, "-n", "5", "-o", out), {"MEMO_CONVERT_SLICE": "0"}, b"MEMO_CONVERT_SLICE must be"),
                               (("-b", memb, "-n", "5", "-o", out), {"MEMO_CONVERT_BATCH": "many"}, b"MEMO_CONVERT_BATCH must be")):
        r = _memo("convert", *argv, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - convert\n", (argv, r.stderr)
        assert r.stderr.startswith(b"memo convert: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (argv, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before
    assert open(copy, "rb").read() == open(memb, "rb").read()
    # the first offending row is the one that is named
    r = _memo("convert", "-b", os.path.join(G.GOLD, "rnd_negoverlap.parquet"), "-n", "12", "-o", out)
    s, e, a = G.index_columns("rnd_negoverlap.parquet", "chrN")
    i = int(np.flatnonzero(e < s)[0])
    assert f"row {i} ends before it starts ({s[i]}, {e[i]}, {a[i]})".encode() in r.stderr
    # the same command with nothing to refuse does reach the library, which is not there
    r = _memo("convert", "-b", memb, "-n", "5", "-o", out)
    assert r.returncode == 1 and (b"Traceback" in r.stderr or b"memo convert: " in r.stderr) and b"must be" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_the_library_functions_refuse_what_the_command_refuses():
    from memo_amd import convert
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    for bad, message in ((lambda: convert.rows(s, e, a, 1), "n_docs must be in"), (lambda: convert.rows(s, e, a, 2049), "n_docs must be in"),
                         (lambda: convert.rows(s, e, a, 4), "annot 4 outside"), (lambda: convert.rows(s, s - 1, a, 5), "ends before it starts"),
                         (lambda: convert.rows(s, e, a, 5, length=25), "below its largest row start"),
                         (lambda: convert.rows([2 ** 31], [2 ** 31], [1], 2), "the length 2147483648 is above 2.31 - 1"),
                         (lambda: convert.rows(s, e, a[:-1], 5), "differ in length"),
                         (lambda: convert.rows(s, e, a, 5, slice_positions=0), "slice_positions must be"),
                         (lambda: convert.rows(s, e, a, 5, batch_positions=-3), "batch_positions must be")):
        with pytest.raises(ValueError, match=message):
            bad()
    assert convert.default_batch_positions(100) * 99 * 4 <= 128 << 20 < (convert.default_batch_positions(100) + 1) * 99 * 4
    assert convert.default_batch_positions(2) == 32 << 20
    import memo_amd
    assert memo_amd.convert is convert and memo_amd.convert_index is convert.convert_index


# ---------------------------------------------------------------------------------------
# pass A: every slice's carry, from the right
# ---------------------------------------------------------------------------------------
def test_the_carries_from_the_right_are_the_definitions():
    from memo_amd import convert
    rng = np.random.default_rng(77)
    runs = 0
    for trial in range(100):
        n = int(rng.integers(2, 8))
        L = int(rng.integers(1, 150))
        rows = int(rng.integers(0, 160))
        s = rng.integers(-3, L + (L if trial % 3 == 0 else 1) + 3, rows)      # (every third set has rows right of the record, some past its reach)
        e = s + rng.integers(0, 60, rows)
        a = rng.choice(np.array(list(range(n)) + [-1, n], np.int64), rows)
        for step in (1, 3, 7, 64):
            got = convert.slice_carries(s, e, a, L, n, step)
            want = convert_oracle.carries(s, e, a, L, n, step)
            assert list(got) == sorted(want, reverse=True) and len(got) == -(-L // step), (trial, step)
            for key in want:
                assert np.array_equal(got[key], want[key]), (trial, step, key)
            runs += 1
    assert runs == 400
