"""Coordinates past 2^31 and 2^32 on the host side (no GPU).  tests/test_far_coordinates_gpu.py leans on one property: shifting every
row and the window by D changes no result byte.  Here the oracle is held to it against itself and against its NumPy restatement, and
the host rules that take a coordinate -- memo_split_window, the generator's row ranges, the Parquet region slice -- are checked at
such coordinates against restatements in Python's unbounded integers."""
from fractions import Fraction

import numpy as np
import pytest

SHIFTS = (0, 2 ** 31 - 60_001, 2 ** 32 - 59_997, 2 ** 32, 2 ** 33 + 12_345, 2 ** 40 + 3, 2 ** 60)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    memo_amd.build()
    memo_amd.lib()
    return memo_amd


def _small_rows(seed, n=4000, length=3000, n_docs=40):
    """ties, duplicates, overlaps longer than any k here, rows with end < start"""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.integers(1, length, n)).astype(np.int64)
    e = s + rng.integers(0, 120, n)
    e[::7] = s[::7] + rng.integers(250, 900, len(s[::7]))
    e[3::97] = s[3::97] - rng.integers(1, 700, len(s[3::97]))
    o = rng.integers(1, n_docs, n).astype(np.int64)
    return s, e, o


def test_oracle_is_translation_invariant(oracle):
    """literal port, closed forms and the NumPy restatement: the same bytes at every shift, windows on and across the rows' extent"""
    n_docs, length = 40, 3000
    s, e, o = _small_rows(1, length=length, n_docs=n_docs)
    windows = ((0, length + 50), (1, length - 1), (997, 1003), (1500, 1500), (2990, 3400))
    checked = 0
    for k in (2, 31, 101, 300):
        base = {}
        for qs, qe in windows:
            rows = oracle.filter_rows(s, e, o, qs, qe, k)
            cons = oracle.conservation(*rows, qs, qe, k, n_docs, literal=False)
            memb = oracle.membership(*rows, qs, qe, k, n_docs, literal=False)
            assert np.array_equal(cons, oracle.conservation(*rows, qs, qe, k, n_docs, literal=True))
            assert np.array_equal(memb, oracle.membership(*rows, qs, qe, k, n_docs, literal=True))
            base[qs, qe] = (rows, cons, memb)
        for D in SHIFTS[1:]:
            for (qs, qe), (rows0, cons0, memb0) in base.items():
                rows = oracle.filter_rows(s + D, e + D, o, qs + D, qe + D, k)
                assert all(np.array_equal(a, b + d) for a, b, d in zip(rows, rows0, (D, D, 0))), (k, D, qs)
                for literal in (False, True):
                    assert np.array_equal(oracle.conservation(*rows, qs + D, qe + D, k, n_docs, literal=literal), cons0), (k, D, qs)
                    assert np.array_equal(oracle.membership(*rows, qs + D, qe + D, k, n_docs, literal=literal), memb0), (k, D, qs)
                # the NumPy restatement, independent of the C file
                assert np.array_equal(oracle.np_conservation(*rows, qs + D, qe + D, k, n_docs), cons0), (k, D, qs)
                assert np.array_equal(oracle.np_membership(*rows, qs + D, qe + D, k, n_docs), memb0), (k, D, qs)
                checked += 1
    assert checked == 4 * 6 * 5


def _split_rule(qs, qe, parts, align, weight):
    """memo_split_window restated in exact arithmetic: part 0 takes `weight` shares, every other part one; lengths rounded up to
    whole positions, then to `align`; the tail takes what is left"""
    L = max(qe - qs, 0)
    w = Fraction(weight)
    shares = w + parts - 1

    def round_up(x):
        v = -((-x.numerator) // x.denominator)
        return -(-v // align) * align
    per = round_up(Fraction(L) / shares) if shares > 0 else 0
    first = L if parts == 1 else (round_up(Fraction(L) * w / shares) if shares > 0 else 0)
    cuts, at = [qs], qs
    for g in range(parts):
        at = min(at + (first if g == 0 else per), qs + L)
        cuts.append(at)
    cuts[parts] = qs + L
    for g in range(parts, 0, -1):
        cuts[g - 1] = min(cuts[g - 1], cuts[g])
    return cuts


def test_split_window_far_from_the_origin(memo):
    from memo_amd import shard
    cases = 0
    for base in (2 ** 31, 2 ** 32, 2 ** 60):
        for off in (-60_001, -8, -1, 0, 1, 12_345):
            for L in (0, 1, 7, 9, 1000, 123_457, 120_000, 10 ** 8 + 3):
                for parts in range(1, 10):
                    for align in (1, 8, 32):
                        for w in (0.0, 0.5, 1.0):
                            qs = base + off
                            wins, per = shard.split_window(qs, qs + L, parts, align=align, root_weight=w)
                            cuts = [wins[0][0]] + [b for _, b in wins]
                            want = _split_rule(qs, qs + L, parts, align, w)
                            assert cuts == want, (qs, L, parts, align, w, cuts, want)
                            assert all(a == c for (a, _), c in zip(wins, cuts[:-1]))
                            assert cuts[0] == qs and cuts[-1] == qs + L
                            assert all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
                            lens = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
                            nonempty = [x for x in lens if x]
                            assert all(x % align == 0 for x in nonempty[:-1]), (qs, L, parts, align, w, lens)
                            cases += 1
    assert cases == 3 * 6 * 8 * 9 * 3 * 3


def test_generator_rows_past_2_pow_32(oracle):
    """synth.shard_rows, synth.host_rows and oracle.synth_rows at the rows of positions up to 2^33 (row numbers up to 1.2e11)
    against the closed form start_i = 1 + floor(i den / num) in Python integers"""
    from memo_amd import synth
    pivot, k = 2 ** 33, 31
    for n_docs in (20, 100, 500):                                 # 1, 5 and 25 rows per position
        num, den = synth.rows_per_position(n_docs)
        total = synth.first_row_at_or_after(pivot, num, den)

        def start(i):
            return 1 + (i * den) // num
        assert start(total) >= pivot > start(total - 1)
        for a in (2 ** 31 - 150_000, 2 ** 32 - 150_000, 2 ** 32 + 2 ** 31 + 777, 2 ** 33 - 70_001):
            b = a + 3001
            r0, r1 = synth.shard_rows(a, b, k, num, den, pivot)
            hi = min(b + k, pivot)
            assert start(r0) > a >= start(r0 - 1), (n_docs, a)
            assert start(r1 - 1) < hi <= start(r1) or r1 == total, (n_docs, a)
            assert r1 - r0 == sum(1 for i in range(r0 - 2, r1 + 2) if a < start(i) < hi)
            s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, n_docs)
            assert s.tolist() == [start(i) for i in range(r0, r1)], (n_docs, a)
            assert ((e - s >= 0) & (e - s < 60)).all() and ((o >= 1) & (o < n_docs)).all()
            hs, he, ho = synth.host_rows(r0, r1 - r0, num, den, n_docs)
            assert np.array_equal(hs, s) and np.array_equal(he, e) and np.array_equal(ho, o), (n_docs, a)
        # a window that reaches past the pivot's last row is clipped to it
        r0, r1 = synth.shard_rows(pivot - 100, pivot + 5000, k, num, den, pivot)
        assert r1 == total and start(r0) > pivot - 100 >= start(r0 - 1)


def test_region_slice_of_a_parquet_index_past_2_pow_32(memo, tmp_path):
    """filter_pq and region_chunks (row groups pruned by their statistics) on starts on both sides of 2^32, against a NumPy filter;
    the region string of the command line parsed as main() parses it"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import memo_query as mq
    rng = np.random.default_rng(6)
    D, n = 2 ** 32 - 59_997, 60_000
    s = np.sort(rng.integers(1, 120_000, n)).astype(np.int64) + D
    e = s + rng.integers(0, 90, n)
    e[5::101] = s[5::101] - rng.integers(1, 300, len(s[5::101]))
    o = rng.integers(1, 70, n).astype(np.int64)
    other = pa.table({"f0": pa.array(["chrA"] * 5000, pa.utf8()), "f1": np.arange(5000) + 2 ** 32 - 2500,
                      "f2": np.arange(5000) + 2 ** 32 - 2400, "f3": np.ones(5000, np.int64)})
    path = str(tmp_path / "far.parquet")
    pq.write_table(pa.concat_tables([other, pa.table({"f0": pa.array(["chrZ"] * n, pa.utf8()), "f1": s, "f2": e, "f3": o})]), path,
                   row_group_size=4096, compression="ZSTD")
    for region in (f"chrZ:{D + 1000}-{D + 100_000}", f"chrZ:{2 ** 32 - 3}-{2 ** 32 + 3}", f"chrZ:{2 ** 32}-{2 ** 32 + 40_000}",
                   f"chrZ:{D - 500}-{2 ** 32}", f"chrZ:{2 ** 31}-{2 ** 31 + 10}", f"chrZ:0-{2 ** 33}"):
        args = mq.parse_arguments(["-b", path, "-o", "x", "-n", "70", "-k", "31", "-r", region])
        record, start_end = args.genome_region.split(":")
        qs, qe = map(int, start_end.split("-"))
        k = int(args.k)
        keep = (s > qs) & (s < qe + k)
        rows = mq.filter_pq(path, record, qs, qe + k)
        assert np.array_equal(rows.start, s[keep]) and np.array_equal(rows.end, e[keep]) and np.array_equal(rows.annot, o[keep]), region
        assert rows.start.dtype == np.int64
        arr = rows.as_array()
        assert arr.dtype == np.uint64 and arr.shape == (int(keep.sum()), 3)
        bound, chunks = mq.region_chunks(path, record, qs, qe + k)
        got = [np.concatenate(c) if c else np.empty(0, np.int64) for c in zip(*chunks)] or [np.empty(0, np.int64)] * 3
        assert bound >= int(keep.sum())
        assert np.array_equal(got[0], s[keep]) and np.array_equal(got[1], e[keep]) and np.array_equal(got[2], o[keep]), region
