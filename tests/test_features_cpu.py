"""`memo features` without a GPU: the BED reader, the cut of overlapping features into elementary segments, the text writer, the
two forms of the oracle (tests/features_oracle.py), and the command line's refusals that never reach the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import features_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def _write(tmp_path, text, name="f.bed"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


# ---------------------------------------------------------------------------------------
# read_bed
# ---------------------------------------------------------------------------------------
def test_read_bed_skips_what_is_no_feature_and_keeps_the_order(tmp_path):
    from memo_amd import features
    bed = features.read_bed(_write(tmp_path, "# a comment\n"
                                             "track name=genes\n"
                                             "browser position ref_1:0-20\n"
                                             "\n"
                                             "   \n"
                                             "ref_2\t15\t15\tc\n"
                                             "ref_1\t5\t20\tb\t0\t+\tmore\tcolumns\n"
                                             "ref_1\t0\t10\n"
                                             "ref_1\t0\t10\t\n"
                                             "ref_1\t7\t9\ta name\r\n"
                                             "#ref_1\t1\t2\tcommented out\n"
                                             "ref_1\t+3\t4\tlast"))                      # (no newline at the end of the file)
    assert len(bed) == 6
    assert bed.chroms == ["ref_2", "ref_1", "ref_1", "ref_1", "ref_1", "ref_1"]
    assert bed.starts.dtype == np.int64 and bed.starts.tolist() == [15, 5, 0, 0, 7, 3] and bed.ends.tolist() == [15, 20, 10, 10, 9, 4]
    assert bed.names == ["c", "b", ".", ".", "a name", "last"]                            # a missing name is `.`
    empty = features.read_bed(_write(tmp_path, "# nothing\n\ntrack\n", "empty.bed"))
    assert len(empty) == 0 and empty.starts.shape == (0,)
    big = features.read_bed(_write(tmp_path, f"chr1\t{2 ** 33}\t{2 ** 33 + 5}\tfar\n", "big.bed"))
    assert big.starts.tolist() == [2 ** 33] and big.ends.tolist() == [2 ** 33 + 5]


@pytest.mark.parametrize("line,what", [("ref_1\t5", "fields"), ("ref_1", "fields"), ("ref_1 5 10 spaces", "fields"),
                                       ("ref_1\tfive\t10", "start"), ("ref_1\t5\t1e3", "end"), ("ref_1\t5.0\t10", "start"),
                                       ("ref_1\t\t10", "start"), ("ref_1\t5\t", "end"), ("ref_1\t-1\t10", "negative"),
                                       ("ref_1\t10\t9", "less than")])
def test_read_bed_refuses_a_line_with_its_number(tmp_path, line, what):
    from memo_amd import features
    with pytest.raises(ValueError) as exc:
        features.read_bed(_write(tmp_path, "# header\nref_1\t0\t10\ta\n\n" + line + "\nref_1\t1\t2\n"))
    assert "line 4" in str(exc.value) and what in str(exc.value)


# ---------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------
HAND_MADE = {"overlapping": ([0, 5, 8], [10, 20, 12]),
             "nested": ([0, 2, 4, 5], [100, 50, 6, 6]),
             "identical": ([7, 7, 7], [19, 19, 19]),
             "empty among others": ([0, 5, 5, 30, 12], [10, 5, 20, 30, 12]),
             "only empty": ([4, 4], [4, 4]),
             "touching": ([0, 10, 20], [10, 20, 30]),
             "unsorted": ([50, 0, 25, 10, 49], [60, 30, 26, 55, 50]),
             "one": ([3], [4]),
             "far": ([2 ** 33, 2 ** 33 + 5], [2 ** 33 + 10, 2 ** 33 + 6])}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_segments_and_prefix_differences_equal_direct_sums(name):
    from memo_amd import features
    starts, ends = (np.array(x, np.int64) for x in HAND_MADE[name])
    edges, lo, hi = features.segments(starts, ends)
    assert edges.dtype == np.int64 and lo.dtype == np.int32 and hi.dtype == np.int32
    assert edges.tolist() == sorted(set(starts.tolist() + ends.tolist())) and len(edges) <= 2 * len(starts)
    assert np.array_equal(edges[lo], starts) and np.array_equal(edges[hi], ends)
    assert np.array_equal(lo == hi, starts == ends)                                       # no positions: no segments
    segs = len(edges) - 1
    rng = np.random.default_rng(len(name))
    # a random value per position, summed per segment: the prefix differences along the segments are the direct sums per feature
    first, L = int(edges[0]), int(edges[-1] - edges[0])
    per_position = rng.integers(0, 1000, (3, L)).astype(np.int64)
    table = np.array([[per_position[r, a - first:b - first].sum() for a, b in zip(edges[:-1], edges[1:])] for r in range(3)], np.int64).reshape(3, segs)
    prefix = np.concatenate([np.zeros((3, 1), np.int64), np.cumsum(table, axis=1)], axis=1)
    direct = np.array([[per_position[r, s - first:e - first].sum() for r in range(3)] for s, e in zip(starts, ends)])
    assert np.array_equal((prefix[:, hi] - prefix[:, lo]).T, direct)
    assert np.array_equal(O.feature_sums(table.astype(np.uint64), lo, hi).astype(np.int64), direct)


def test_segments_refuses_an_end_below_its_start():
    from memo_amd import features
    with pytest.raises(ValueError):
        features.segments([5], [4])
    edges, lo, hi = features.segments([], [])
    assert len(edges) == 0 and len(lo) == 0 and len(hi) == 0


def test_ranges_batches_and_the_table_cap():
    from memo_amd import features
    bed = features.Bed(["a"] * 4, [0, 10, 10, 10], [10, 12, 13, 10], ["."] * 4)
    assert features.feature_ranges(bed, 3)[1].tolist() == [10, 12, 13, 10]
    assert features.feature_ranges(bed, 3, inside=True)[1].tolist() == [8, 10, 11, 10]    # [start, max(start, end - k + 1))
    assert np.array_equal(features.feature_ranges(bed, 3, inside=True)[1], O.inside_ends(bed.starts, bed.ends, 3))
    assert features.BATCH_FEATURES == 1 << 19 and features.SEGMENT_TABLE_BYTES == 2 << 30
    assert features.batch_limit(2) == 1 << 19 and features.batch_limit(2, 3) == 3
    assert features.batch_limit(2048) == (2 << 30) // (16 * 2048) == 65536                # 2F segments x 2048 rows x 8 bytes: 2 GiB
    for bad in (0, (1 << 19) + 1):
        with pytest.raises(ValueError):
            features.batch_limit(2, bad)


# ---------------------------------------------------------------------------------------
# the oracle's two forms
# ---------------------------------------------------------------------------------------
def test_the_two_forms_of_the_oracle_agree():
    rng = np.random.default_rng(5)
    L, N, first = 700, 9, 1000
    B = (rng.random((L, N)) < 0.4).astype(np.uint8)
    v = rng.integers(0, N + 1, L)
    starts = rng.integers(first - 20, first + L + 20, 60)
    ends = starts + rng.integers(0, 300, 60)
    assert np.array_equal(O.memb(B, starts, ends, first), O.memb_fast(B, starts, ends, first))
    for T in (0, 1, N, N + 1):
        assert np.array_equal(O.cons(v, starts, ends, T, first), O.cons_fast(v, starts, ends, T, first))
    edges = np.sort(rng.integers(first, first + L + 1, 30))
    assert np.array_equal(O.segment_table(v, edges, 4, first), O.segment_table_fast(v, edges, 4, first))
    assert O.memb(B, [first], [first + L], first)[0].tolist() == B.sum(axis=0).tolist()
    assert O.cons(v, [first + 5], [first + 5], 1, first).tolist() == [[0, 0]]


# ---------------------------------------------------------------------------------------
# format_features, shares, calls
# ---------------------------------------------------------------------------------------
def _bed():
    from memo_amd import features
    return features.Bed(["ref_1", "ref_1", "ref_2"], [0, 5, 15], [10, 20, 15], ["a", "b", "."])


def test_format_features_against_literals():
    from memo_amd import features
    bed, positions = _bed(), np.array([10, 15, 0])
    counts = np.array([[10, 5], [15, 2 ** 32 + 7], [0, 0]], np.uint64)
    assert features.format_features(bed, positions, counts, True) == ("chrom\tstart\tend\tname\tpositions\t0\t1\n"
                                                                     "ref_1\t0\t10\ta\t10\t10\t5\n"
                                                                     "ref_1\t5\t20\tb\t15\t15\t4294967303\n"
                                                                     "ref_2\t15\t15\t.\t0\t0\t0\n")
    assert features.format_features(bed, positions, counts, True, ["pivot", "g1"]).startswith("chrom\tstart\tend\tname\tpositions\tpivot\tg1\n")
    assert features.format_features(bed, positions, counts, False) == ("chrom\tstart\tend\tname\tpositions\tsum\tshared\n"
                                                                      "ref_1\t0\t10\ta\t10\t10\t5\n"
                                                                      "ref_1\t5\t20\tb\t15\t15\t4294967303\n"
                                                                      "ref_2\t15\t15\t.\t0\t0\t0\n")
    small = np.array([[10, 5], [15, 7], [0, 0]], np.uint64)
    share = features.shares(small, positions)
    assert share.dtype == np.float64
    assert features.format_features(bed, positions, share, True) == ("chrom\tstart\tend\tname\tpositions\t0\t1\n"
                                                                    "ref_1\t0\t10\ta\t10\t1.0\t0.5\n"
                                                                    f"ref_1\t5\t20\tb\t15\t1.0\t{7 / 15!r}\n"
                                                                    "ref_2\t15\t15\t.\t0\tnan\tnan\n")
    assert features.format_features(bed, positions, share, False).startswith("chrom\tstart\tend\tname\tpositions\tmean\tshared_fraction\n")
    empty = features.Bed([], [], [], [])
    assert features.format_features(empty, np.zeros(0, np.int64), np.zeros((0, 5), np.uint64), True) == "chrom\tstart\tend\tname\tpositions\t0\t1\t2\t3\t4\n"
    assert features.format_features(empty, np.zeros(0, np.int64), np.zeros((0, 2), np.uint64), False) == "chrom\tstart\tend\tname\tpositions\tsum\tshared\n"
    with pytest.raises(ValueError):
        features.format_features(bed, positions, counts, True, ["only one"])
    with pytest.raises(ValueError):
        features.format_features(bed, positions, counts[:2], True)
    with pytest.raises(ValueError):
        features.format_features(bed, positions, counts, False, ["a", "b"])


def test_the_call_rule_at_equality():
    """1 where positions > 0 and count >= FRACTION * positions in float64: equality calls, one count below does not"""
    from memo_amd import features
    positions = np.array([10, 10, 10, 4, 3, 0, 7])
    counts = np.array([[5], [4], [6], [1], [1], [0], [7]], np.uint64)
    assert features.calls(counts, positions, 0.5).reshape(-1).tolist() == [1, 0, 1, 0, 0, 0, 1]
    assert features.calls(counts, positions, 0.25).reshape(-1).tolist() == [1, 1, 1, 1, 1, 0, 1]      # 1 >= 0.25 * 4 exactly
    assert features.calls(counts, positions, 1.0).reshape(-1).tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert features.calls(counts, positions, 1 / 3).reshape(-1).tolist() == [1, 1, 1, 0, 1, 0, 1]     # 1 >= (1 / 3) * 3 in float64
    for fraction in (0.5, 0.25, 1.0, 1 / 3, 0.1, 0.7):
        want = [int(p > 0 and float(c) >= fraction * float(p)) for c, p in zip(counts.reshape(-1).tolist(), positions.tolist())]
        assert features.calls(counts, positions, fraction).reshape(-1).tolist() == want
    bed = features.Bed(["r"] * 7, [0] * 7, positions, ["."] * 7)
    text = features.format_features(bed, positions, features.calls(counts, positions, 0.5), True)
    assert text.splitlines()[1:3] == ["r\t0\t10\t.\t10\t1", "r\t0\t10\t.\t10\t0"] and text.splitlines()[6] == "r\t0\t0\t.\t0\t0"


# ---------------------------------------------------------------------------------------
# the command line, as far as it goes without the library
# ---------------------------------------------------------------------------------------
def test_usage_and_dispatch():
    from memo_amd import features_cli
    usage = features_cli.USAGE.encode()
    assert usage.startswith(b"\nMEMO features - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("features", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-k [INT]", b"-n [INT]", b"-a [FILE]", b"-o [FILE]", b"  -m  ", b"  -f  ", b"-p [FLOAT]", b"-t [INT]", b"  -i  ",
                 b"-g [FILE]", b"[31]"):
        assert flag in usage
    assert b"MEMBERSHIP" in usage and b"conservation index" in usage and b"nothing in the file tells them apart" in usage
    r = _memo("features", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("features", "-b", "x.parquet", "-k", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - features\n" and r.stderr == b"memo features: -a, -n, -o required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import features
    assert memo_amd.bed_features is features.bed_features and memo_amd.read_bed is features.read_bed


def test_refusals_before_the_library_is_touched(tmp_path):
    """exit status 1, one message, nothing written (-b names no file and the library path names none: a refusal that came later
    would be another message)"""
    out = str(tmp_path / "never.tsv")
    good = _write(tmp_path, "ref_1\t0\t10\ta\nref_1\t5\t20\tb\n", "good.bed")
    bad = _write(tmp_path, "ref_1\t0\t10\ta\nref_1\t20\t5\tb\n", "bad.bed")
    short = _write(tmp_path, "ref_1\t0\t10\ta\n\nref_1\t7\n", "short.bed")
    common = ("-b", str(tmp_path / "no.parquet"), "-k", "3", "-n", "5", "-o", out)
    for extra, env, message in ((("-a", good, "-m", "-f", "-p", "0.5"), None, b"-f and -p together"),
                                (("-a", good, "-p", "0.5"), None, b"-p needs -m"),
                                (("-a", good, "-g", good), None, b"-g needs -m"),
                                (("-a", good, "-m", "-t", "3"), None, b"-t has no meaning with -m"),
                                (("-a", good, "-m", "-p", "0"), None, b"-p must be a fraction in (0, 1]"),
                                (("-a", good, "-m", "-p", "1.5"), None, b"-p must be a fraction in (0, 1]"),
                                (("-a", good, "-m", "-p", "-0.1"), None, b"-p must be a fraction in (0, 1]"),
                                (("-a", good, "-m", "-p", "nan"), None, b"-p must be a fraction in (0, 1]"),
                                (("-a", good, "-m", "-p", "half"), None, b"-p must be a fraction in (0, 1]"),
                                (("-a", good, "-t", "0"), None, b"-t must be an integer in [1, 5]"),
                                (("-a", good, "-t", "6"), None, b"-t must be an integer in [1, 5]"),
                                (("-a", good, "-m", "-n", "2049"), None, b"-n must be in [1, 2048]"),
                                (("-a", good, "-n", "five"), None, b"invalid literal for int()"),
                                (("-a", bad), None, b"line 2"),
                                (("-a", bad, "-m"), None, b"less than"),
                                (("-a", short), None, b"line 3"),
                                (("-a", str(tmp_path / "no.bed")), None, b"cannot read the BED file"),
                                (("-a", good, "-m", "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                                (("-a", good), {"WORLD_SIZE": "2"}, b"sharded launch")):
        r = _memo("features", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - features\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo features: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    r = _memo("features", *common, "-a", good, "-m", "-p", "1")
    assert r.returncode == 1 and not os.path.exists(out)
    assert b"Traceback" in r.stderr or b"memo features: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.bed", "good.bed", "short.bed"]
