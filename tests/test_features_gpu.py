"""`memo features` on the GPU: the two kernels (memo_amd/csrc/memo_features.hip) against NumPy on the host, the BED route against
the goldens, the command line against the formatter.

The oracle everywhere is tests/features_oracle.py; every comparison is exact."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import features_oracle as O
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
GRID_X = 1024                                                   # workgroups at most (memo_features.hip: kMaxGridX)
MAX_SEGS = (1 << 20) + 1


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


class Resident:
    """bytes uploaded once; parts of them are device pointers"""

    def __init__(self, host):
        from memo_amd._lib import check, lib
        self.host = np.ascontiguousarray(host)
        self.d = C.c_void_p()
        check(lib().memo_dev_malloc(0, max(self.host.nbytes, 16), C.byref(self.d)))
        check(lib().memo_dev_upload(0, self.d, self.host.ctypes.data, self.host.nbytes, None))

    def download(self):
        from memo_amd._lib import check, lib
        out = np.empty_like(self.host)
        check(lib().memo_dev_download(0, out.ctypes.data, self.d, out.nbytes, None))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from memo_amd._lib import lib
        lib().memo_dev_free(0, self.d)


def same(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, np.asarray(want).astype(np.uint64))


# ---------------------------------------------------------------------------------------
# memo_feature_sums_dev against numpy.cumsum
# ---------------------------------------------------------------------------------------
def wrapping_table(rows, segs, seed=0):
    """values just above 2^63: the second prefix of a row has wrapped already"""
    rng = np.random.default_rng([seed, rows, segs])
    return np.uint64(2 ** 63) + rng.integers(0, 2 ** 20, (rows, segs)).astype(np.uint64)


def some_features(segs, count, seed=0):
    """lo == hi, lo = 0 and hi = segs, one segment many times, and random ranges"""
    rng = np.random.default_rng([seed, segs, count])
    lo = rng.integers(0, segs + 1, count)
    hi = np.array([rng.integers(a, segs + 1) for a in lo], np.int64).reshape(count)
    fixed = [(0, segs), (0, 0), (segs, segs), (segs - 1, segs), (0, 1)] + [(segs // 2, segs // 2 + 1)] * 9 + [(segs // 2, segs // 2)]
    for i, (a, b) in enumerate(fixed[:count]):
        lo[i], hi[i] = a, min(max(b, a), segs)
    return lo.astype(np.int32), hi.astype(np.int32)


@pytest.mark.parametrize("rows", (1, 2, 5, 64, 2048))
def test_feature_sums_equal_cumsum_differences(memo, rows):
    from memo_amd import features
    T = features.sums_tile()
    assert T >= 256 and T % 256 == 0
    for segs in (1, 2, T - 1, T, T + 1, 2 * T + 1):
        table = wrapping_table(rows, segs)
        lo, hi = some_features(segs, 257)
        got = features.feature_sums(table, lo, hi)
        assert same(got, O.feature_sums(table, lo, hi)), (rows, segs)
        if segs >= 2:
            assert int(np.cumsum(table[0], dtype=np.uint64)[1]) < 2 ** 22 and int(table[0, 0]) >= 2 ** 63      # the prefixes do wrap
        direct = np.array([[int(table[r, a:b].astype(object).sum()) % 2 ** 64 for r in (0, rows - 1)] for a, b in zip(lo[:20], hi[:20])], np.uint64)
        assert np.array_equal(got[:20][:, [0, rows - 1]], direct), (rows, segs)                   # ... and the oracle is the plain sum


@pytest.mark.parametrize("count", (0, 1, 255, 256, 257))
def test_feature_counts_around_a_workgroup(memo, count):
    from memo_amd import features
    rows, segs = 5, features.sums_tile() + 1
    table = wrapping_table(rows, segs, seed=1)
    lo, hi = some_features(segs, count, seed=1)
    got = features.feature_sums(table, lo, hi)
    assert got.shape == (count, rows) and same(got, O.feature_sums(table, lo, hi))
    small = np.arange(rows * segs, dtype=np.uint64).reshape(rows, segs)                          # small values: plain int64 sums
    got = features.feature_sums(small, lo, hi)
    assert np.array_equal(got.astype(np.int64), np.array([small[:, a:b].sum(axis=1) for a, b in zip(lo, hi)], np.int64).reshape(count, rows))


def test_the_scan_of_the_tile_sums_has_more_than_one_round(memo):
    """rows = 1 and segs = 2^20 + 1: 513 tiles, whose sums are scanned 256 at a time with a carry"""
    from memo_amd import features
    segs = MAX_SEGS
    assert -(-segs // features.sums_tile()) > 256
    table = wrapping_table(1, segs, seed=2)
    lo, hi = some_features(segs, 257, seed=2)
    assert same(features.feature_sums(table, lo, hi), O.feature_sums(table, lo, hi))
    ones = np.ones((1, segs), np.uint64)
    assert np.array_equal(features.feature_sums(ones, lo, hi).reshape(-1).astype(np.int64), (hi - lo).astype(np.int64))


def test_a_resident_table_becomes_scratch_and_many_features_share_a_segment(memo):
    from memo_amd import features
    rows, segs = 3, 700
    table = wrapping_table(rows, segs, seed=3)
    lo, hi = np.full(1000, 123, np.int32), np.full(1000, 124, np.int32)
    with Resident(table) as d:
        got = features.feature_sums((d.d.value, rows, segs), lo, hi)
        assert same(got, np.tile(table[:, 123], (1000, 1)))
        assert np.array_equal(d.download(), np.cumsum(table, axis=1, dtype=np.uint64))           # what the call left: the prefix sums


def test_feature_sums_refusals_leave_the_output_as_it_was(memo):
    from memo_amd._lib import MEMO_EINVAL, lib
    rows, segs, count = 4, 10, 3
    table = np.arange(rows * segs, dtype=np.uint64).reshape(rows, segs)
    seed = np.full((count, rows), 0xABCD, np.uint64)
    good_lo, good_hi = np.array([0, 2, 5], np.int32), np.array([10, 2, 6], np.int32)
    with Resident(table) as d_table, Resident(seed) as d_out:
        def call(d_sums, r, s, lo, hi, n, out):
            lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
            return lib().memo_feature_sums_dev(d_sums, r, s, lo.ctypes.data, hi.ctypes.data, n, out, 0, None)
        for what, rc in (("rows 0", call(d_table.d, 0, segs, good_lo, good_hi, count, d_out.d)),
                         ("rows 2049", call(d_table.d, 2049, segs, good_lo, good_hi, count, d_out.d)),
                         ("segs 0", call(d_table.d, rows, 0, good_lo, good_hi, count, d_out.d)),
                         ("segs above 2^20 + 1", call(d_table.d, rows, MAX_SEGS + 1, good_lo, good_hi, count, d_out.d)),
                         ("features -1", call(d_table.d, rows, segs, good_lo, good_hi, -1, d_out.d)),
                         ("no table", call(None, rows, segs, good_lo, good_hi, count, d_out.d)),
                         ("a table 4 bytes off", call(d_table.d.value + 4, rows, segs, good_lo, good_hi, count, d_out.d)),
                         ("no output", call(d_table.d, rows, segs, good_lo, good_hi, count, None)),
                         ("an output 4 bytes off", call(d_table.d, rows, segs, good_lo, good_hi, count, d_out.d.value + 4)),
                         ("lo < 0", call(d_table.d, rows, segs, [0, -1, 5], good_hi, count, d_out.d)),
                         ("lo > hi", call(d_table.d, rows, segs, [0, 3, 5], good_hi, count, d_out.d)),
                         ("hi > segs", call(d_table.d, rows, segs, good_lo, [10, 2, 11], count, d_out.d))):
            assert rc == MEMO_EINVAL, what
            assert lib().memo_last_error(), what
        assert np.array_equal(d_out.download(), seed) and np.array_equal(d_table.download(), table)
        assert call(d_table.d, rows, segs, good_lo, good_hi, 0, d_out.d) == 0                    # features == 0: nothing is written
        assert np.array_equal(d_out.download(), seed)
        assert call(d_table.d, rows, segs, good_lo, good_hi, count, d_out.d) == 0               # nothing to refuse: it answers
        assert np.array_equal(d_out.download(), O.feature_sums(table, good_lo, good_hi))


# ---------------------------------------------------------------------------------------
# memo_segment_conservation_dev against NumPy
# ---------------------------------------------------------------------------------------
def values(L, top, seed=0):
    """conservation values up to `top`, a tenth of them `top` itself"""
    rng = np.random.default_rng([seed, L, top])
    v = rng.integers(0, top + 1, L)
    v[rng.random(L) < 0.1] = top
    return v.astype(np.uint16)


def thresholds(n):
    return (0, 1, n, n + 1, 65535)


def test_every_length_and_segment_count_equals_numpy(memo):
    from memo_amd import features, view
    T = features.segment_tile()
    assert T >= 64 and T % 8 == 0
    Ls = tuple(sorted({1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1}))
    for n in (12, 65535):
        v = values(Ls[-1], n)
        with Resident(v) as d:
            for L in Ls:
                for i, segs in enumerate(sorted({b for b in (1, 2, 3, 7, L - 1, L) if 1 <= b <= L})):
                    edges = view.bin_edges(L, segs)
                    for t in (thresholds(n) if L in (9, T + 1) else thresholds(n)[(i + L) % 5:][:1]):
                        got = features.segment_conservation((d.d.value, L), edges, t)
                        assert same(got, O.segment_table_fast(v[:L], edges, t)), (n, L, segs, t)
    assert np.array_equal(O.segment_table_fast(v, view.bin_edges(len(v), 7), 3), O.segment_table(v, view.bin_edges(len(v), 7), 3))


@pytest.mark.parametrize("n", (5, 65535))
def test_hand_made_edges(memo, n):
    from memo_amd import features
    T = features.segment_tile()
    L = 2 * T + 1
    v = values(L, n, seed=11)
    with Resident(v) as d:
        for name, edges in (("empty segments", [0, 0, 10, 10, 10, 40, L, L]),
                            ("segments of one position", [0, 1, 2, 3, 8, 9, 10, T - 1, T, T + 1, T + 2, L - 1, L]),
                            ("five edges inside one lane's positions", [0, 33, 34, 36, 37, 39, L]),
                            ("an edge at T - 1, at T and at T + 1", [0, T - 1, T, T + 1, L]),
                            ("every edge on a lane", [0, 8, 64, 96, T, T + 8, L]),
                            ("one segment", [0, L]),
                            ("before the values and behind them", [-1000, -5, 17, L + 3, L + 3, L + 2000])):
            for t in thresholds(min(n, 5)):
                got = features.segment_conservation((d.d.value, L), edges, t)
                assert same(got, O.segment_table(v, edges, t)), (n, name, t)
                assert int(got[0].sum()) == int(v.astype(np.int64).sum()), (n, name)      # the edges cover the values: each is summed once
                assert int(got[1].sum()) == int((v >= t).sum()), (n, name, t)
        # ... and with the values somewhere inside the edges: a first that is no multiple of 8
        for first, edges in ((77, [0, 50, 77, 78, 100, 77 + T, 77 + L, 5000]), (1000003, [1000000, 1000003 + T - 1, 1000003 + L])):
            got = features.segment_conservation((d.d.value, L), edges, 3, first=first)
            assert same(got, O.segment_table(v, edges, 3, first)) and int(got[0].sum()) == int(v.astype(np.int64).sum()), (n, first)


def test_slices_accumulate_to_the_whole_from_a_table_near_2_to_the_32(memo):
    """the same window cut at 1, 7, 8, 9, T and T + 5, each slice with its `first`: the table of the whole; a slice may end inside a
    segment; the starting table is near 2^32, so the adds are 64-bit"""
    from memo_amd import features, view
    T = features.segment_tile()
    L, origin, n = 2 * T + 41, 123457, 40
    v = values(L, n, seed=12)
    start = np.full((2, 1), 2 ** 32 - 5, np.uint64)
    for segs in (1, 5, L):
        edges = view.bin_edges(L, segs) + origin
        seed = np.tile(start, (1, segs))
        want = O.segment_table_fast(v, edges, n, origin).astype(np.uint64) + seed
        whole = features.segment_conservation(v, edges, n, first=origin, sums=seed)
        assert same(whole, want) and int(whole.max()) >= 2 ** 32, segs
        for cut in (1, 7, 8, 9, T, T + 5):
            head = features.segment_conservation(v[:cut], edges, n, first=origin, sums=seed)
            assert same(head, O.segment_table_fast(v[:cut], edges, n, origin).astype(np.uint64) + seed), (segs, cut)
            both = features.segment_conservation(v[cut:], edges, n, first=origin + cut, sums=head)
            assert same(both, want), (segs, cut)
    untouched = features.segment_conservation(v[:0], [0, 0, 0], n, sums=np.tile(start, (1, 2)))
    assert np.array_equal(untouched, np.tile(start, (1, 2)))                            # L == 0: nothing launched


def test_every_workgroup_more_than_one_tile_and_a_ragged_tail(memo):
    """2050 tiles and 77 positions: 683 workgroups of three tiles and one of one tile and the tail; wide segments (a workgroup's sums
    leave once or twice), segments about a tile wide, and segments narrower than a lane's eight positions"""
    from memo_amd import features, view
    T = features.segment_tile()
    L = (2 * GRID_X + 2) * T + 77
    per = -(-(-(-L // T)) // GRID_X)
    assert per >= 2 and (-(-L // T)) % per >= 2 and L % T
    v = values(L, 9, seed=13)
    with Resident(v) as d:
        assert v.nbytes < 16 << 20
        for segs in (1, 500, 2051, L // 5):
            assert segs <= MAX_SEGS
            edges = view.bin_edges(L, segs)
            got = features.segment_conservation((d.d.value, L), edges, 7)
            assert same(got, O.segment_table_fast(v, edges, 7)), segs
            assert int(got[0].sum()) == int(v.astype(np.int64).sum()) and int(got[1].sum()) == int((v >= 7).sum()), segs


def test_nothing_before_or_behind_the_values_is_read(memo):
    """the values lie inside a larger buffer whose neighbours are 0xFFFF: the table is still the oracle's"""
    from memo_amd import features, view
    T = features.segment_tile()
    for L in (1, 7, 9, 33, T - 1, T + 1):
        v = values(L, 20, seed=8)
        whole = np.concatenate([np.full(8, 0xFFFF, np.uint16), v, np.full(T + 16, 0xFFFF, np.uint16)])
        with Resident(whole) as d:
            edges = view.bin_edges(L, min(L, 3))
            for t in (0, 21):
                assert same(features.segment_conservation((d.d.value + 16, L), edges, t), O.segment_table(v, edges, t)), (L, t)


def test_segment_conservation_refusals_leave_the_table_as_it_was(memo):
    from memo_amd._lib import MEMO_EINVAL, lib
    L, segs = 100, 4
    seed = np.arange(2 * segs, dtype=np.uint64).reshape(2, segs) + 7
    good = np.array([0, 25, 50, 75, 100], np.int64)
    with Resident(np.full(L + 16, 3, np.uint16)) as vec, Resident(seed) as table:
        assert vec.d.value % 16 == 0 and table.d.value % 8 == 0

        def call(d_vec, first, edges, n, t, d_sums, length=L):
            edges = np.ascontiguousarray(edges, np.int64)
            return lib().memo_segment_conservation_dev(d_vec, length, first, edges.ctypes.data, n, t, d_sums, 0, None)
        for what, rc in (("values 2 bytes off", call(vec.d.value + 2, 0, good, segs, 3, table.d)),
                         ("values 8 bytes off", call(vec.d.value + 8, 0, good, segs, 3, table.d)),
                         ("a table 4 bytes off", call(vec.d, 0, good, segs, 3, table.d.value + 4)),
                         ("no table", call(vec.d, 0, good, segs, 3, None)),
                         ("segs 0", call(vec.d, 0, good, 0, 3, table.d)),
                         ("segs above 2^20 + 1", call(vec.d, 0, good, MAX_SEGS + 1, 3, table.d)),
                         ("a negative threshold", call(vec.d, 0, good, segs, -1, table.d)),
                         ("decreasing edges", call(vec.d, 0, [0, 50, 49, 75, 100], segs, 3, table.d)),
                         ("a slice that begins before the edges", call(vec.d, -1, good, segs, 3, table.d)),
                         ("a slice that ends behind the edges", call(vec.d, 1, good, segs, 3, table.d)),
                         ("an empty slice behind the edges", call(vec.d, 101, good, segs, 3, table.d, length=0))):
            assert rc == MEMO_EINVAL, what
            assert lib().memo_last_error(), what
        assert np.array_equal(table.download(), seed)
        assert call(vec.d, 0, good, segs, 3, table.d) == 0                              # and the same call with nothing to refuse counts
        assert np.array_equal(table.download(), seed + np.array([[75], [25]], np.uint64))


# ---------------------------------------------------------------------------------------
# end to end: a BED of the goldens' regions against the goldens
# ---------------------------------------------------------------------------------------
GROUPS = collections.defaultdict(list)
for _c in G.cases(raises=False):
    GROUPS[_c["index"], _c["k"], _c["n"], _c["membership"]].append(_c)


def _bed_of(cases):
    from memo_amd import features
    regions = [G.region(c) for c in cases]
    return features.Bed([r[0] for r in regions], [r[1] for r in regions], [r[2] for r in regions], [c["name"] for c in cases])


def _golden_table(cases, threshold):
    rows = []
    for c in cases:
        z = G.load(c)
        if c["membership"]:
            rows.append(G.expected_matrix(c, z).sum(axis=0, dtype=np.int64))
        else:
            v = np.asarray(z["vec"], np.int64)
            rows.append(np.array([v.sum(), (v >= threshold).sum()], np.int64))
    return np.array(rows, np.int64)


def _has_long_rows(index, cases):
    return any(np.any(e < s) for s, e, _ in (G.index_columns(index, rec) for rec in {G.region(c)[0] for c in cases}))


@pytest.mark.parametrize("index,k,n,membership", sorted(GROUPS))
def test_bed_features_equal_the_goldens_however_they_are_swept(memo, index, k, n, membership):
    """the regions of all the goldens of one index, k and n as one BED: they overlap and lie on several records, and every line is
    its golden reduced.  Rows with end < start answer for the window they are swept in, so there every region is a BED of its own."""
    from memo_amd import features
    cases = GROUPS[index, k, n, membership]
    path = os.path.join(G.GOLD, index)
    beds = [cases[i:i + 1] for i in range(len(cases))] if _has_long_rows(index, cases) else [cases]
    for members in beds:
        bed = _bed_of(members)
        want = _golden_table(members, n)
        table, positions = features.bed_features(path, bed, k, n, membership)
        assert positions.tolist() == [G.region(c)[2] - G.region(c)[1] for c in members]
        assert same(table, want), [c["name"] for c in members]
        if membership:
            assert np.all(table[:, 0].astype(np.int64) <= positions)
            for step in (1, 7, 64):
                again, _ = features.bed_features(path, bed, k, n, membership, slice_positions=step)
                assert np.array_equal(again, table), step
        else:
            t = (n + 1) // 2
            assert same(features.bed_features(path, bed, k, n, threshold=t)[0], _golden_table(members, t))
        for most in (1, 3):
            again, _ = features.bed_features(path, bed, k, n, membership, batch_features=most)
            assert np.array_equal(again, table), most
        turned = features.Bed(bed.chroms[::-1], bed.starts[::-1], bed.ends[::-1], bed.names[::-1])
        again, again_positions = features.bed_features(path, turned, k, n, membership)
        assert np.array_equal(again, table[::-1]) and np.array_equal(again_positions, positions[::-1])


def test_the_goldens_overlap_lie_on_several_records_and_hold_long_rows():
    assert len(GROUPS) >= 90 and sum(len(v) for v in GROUPS.values()) >= 250
    assert any(len({G.region(c)[0] for c in cs}) > 1 for cs in GROUPS.values())
    assert any(_has_long_rows(key[0], cs) for key, cs in GROUPS.items()) and not all(_has_long_rows(key[0], cs) for key, cs in GROUPS.items())
    overlapping = 0
    for cs in GROUPS.values():
        spans = sorted(G.region(c) for c in cs)
        overlapping += any(a[0] == b[0] and b[1] < a[2] for a, b in zip(spans, spans[1:]))
    assert overlapping >= 20


def test_the_readme_example(memo):
    from memo_amd import features
    bed = features.Bed(["ref_1"] * 3, [0, 5, 15], [10, 20, 15], ["a", "b", "c"])
    table, positions = features.bed_features(os.path.join(G.GOLD, "example_memb.parquet"), bed, 3, 5, membership=True)
    assert positions.tolist() == [10, 15, 0]
    assert table.dtype == np.uint64 and table.tolist() == [[10, 5, 9, 10, 9], [15, 7, 12, 15, 14], [0, 0, 0, 0, 0]]
    whole = features.Bed(["ref_1"], [0], [20], ["."])
    table, positions = features.bed_features(os.path.join(G.GOLD, "example_cons.parquet"), whole, 3, 5)
    assert positions.tolist() == [20] and table.tolist() == [[84, 8]]
    memb, _ = features.bed_features(os.path.join(G.GOLD, "example_memb.parquet"), whole, 3, 5, membership=True)
    assert int(memb.sum()) == 84                                                        # the sum of the five membership columns
    assert features.bed_features(os.path.join(G.GOLD, "example_cons.parquet"), whole, 3, 5, threshold=4)[0].tolist() == [[84, 16]]


@pytest.mark.parametrize("membership", (True, False))
def test_inside_counts_only_the_kmers_wholly_inside(memo, membership):
    """-i: the ends shortened by k - 1, a feature shorter than k a feature of no positions"""
    from memo_amd import features
    for index, k in (("example_memb.parquet" if membership else "example_cons.parquet", 3), ("rnd_n40.parquet", 31)):
        c = next(c for c in G.cases(membership=membership, raises=False) if c["index"] == index and c["k"] == k and c["n"] in (5, 40)
                 and G.region(c)[2] - G.region(c)[1] >= 20)
        rec, qs, qe = G.region(c)
        L, n = qe - qs, c["n"]
        starts = np.array([qs, qs + 5, qs + 4, qs + 7, qs + 3, qs, qs + L - k], np.int64)
        ends = np.minimum(np.array([qs + 10, qe, qs + 4 + k - 1, qs + 7 + k, qs + 3, qe, qe], np.int64), qe)
        ends = np.maximum(ends, starts)
        short = O.inside_ends(starts, ends, k)
        assert np.any(short == starts) and np.any(ends - starts == k - 1) and np.any(ends - starts == k)      # shorter than k, and exactly k
        bed = features.Bed([rec] * len(starts), starts, ends, ["."] * len(starts))
        table, positions = features.bed_features(os.path.join(G.GOLD, index), bed, k, n, membership, inside=True)
        assert np.array_equal(positions, short - starts)
        z = G.load(c)
        want = O.memb(G.expected_matrix(c, z), starts, short, qs) if membership else O.cons(z["vec"], starts, short, n, qs)
        assert same(table, want), (index, k)
        plain, _ = features.bed_features(os.path.join(G.GOLD, index), bed, k, n, membership)
        assert same(plain, O.memb(G.expected_matrix(c, z), starts, ends, qs) if membership else O.cons(z["vec"], starts, ends, n, qs))


@pytest.mark.parametrize("membership", (True, False))
def test_features_past_2_to_the_32(memo, tmp_path, membership):
    """the rows of a golden index shifted past 2^32 and 2^33: the table of the shifted features is the origin's"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import features
    c = next(c for c in G.cases(membership=membership, raises=False) if c["index"] == "rnd_n40.parquet" and c["k"] == 31
             and G.region(c)[2] - G.region(c)[1] >= 500)
    rec, qs, qe = G.region(c)
    s, e, o = G.index_columns(c["index"], rec)
    L = qe - qs
    starts = qs + np.array([0, 10, 10, L // 2, L - 1, 7, 7], np.int64)
    ends = qs + np.array([L, L // 2, 11, L, L, 7, 300], np.int64)
    z = G.load(c)
    want = O.memb(G.expected_matrix(c, z), starts, ends, qs) if membership else O.cons(z["vec"], starts, ends, c["n"], qs)
    assert int(want.sum()) > 0
    for D in (2 ** 32, 2 ** 33 + 12_345):
        path = str(tmp_path / f"far{D}.parquet")
        pq.write_table(pa.table({"f0": pa.array([rec] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": o}), path, compression="ZSTD")
        bed = features.Bed([rec] * len(starts), starts + D, ends + D, ["."] * len(starts))
        for step, most in ((1 << 24, None), (1000, 2)):
            got, positions = features.bed_features(path, bed, c["k"], c["n"], membership, slice_positions=step, batch_features=most)
            assert same(got, want) and np.array_equal(positions, ends - starts), (D, step)


def test_bed_features_raises_what_memo_query_raises(memo):
    from memo_amd import features
    path = os.path.join(G.GOLD, "example_memb.parquet")
    bed = features.Bed(["ref_1"], [0], [20], ["."])
    with pytest.raises(IndexError):                      # the sweep's own: an annot outside the result columns
        features.bed_features(path, bed, 3, 2, membership=True)
    with pytest.raises(ValueError):
        features.bed_features(path, bed, 3, 2049, membership=True)
    with pytest.raises(ValueError):
        features.bed_features(path, bed, 3, 5, membership=True, threshold=3)
    for t in (0, 6):
        with pytest.raises(ValueError):
            features.bed_features(os.path.join(G.GOLD, "example_cons.parquet"), bed, 3, 5, threshold=t)
    # features of no positions touch no index: not even a file that is not there
    empty = features.Bed(["ref_1", "chrX"], [7, 0], [7, 0], [".", "."])
    table, positions = features.bed_features(os.path.join(G.GOLD, "no_such.parquet"), empty, 3, 5, membership=True)
    assert table.shape == (2, 5) and not table.any() and positions.tolist() == [0, 0]
    table, positions = features.bed_features(path, features.Bed([], [], [], []), 3, 5, membership=True)
    assert table.shape == (0, 5) and positions.shape == (0,)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


MEMB, CONS = os.path.join(G.GOLD, "example_memb.parquet"), os.path.join(G.GOLD, "example_cons.parquet")
EXAMPLE_BED = "# three features\nref_1\t0\t10\ta\nref_1\t5\t20\tb\t0\t+\nref_1\t15\t15\tc\n"


def test_cli_writes_counts_fractions_calls_and_labels(memo, tmp_path):
    from memo_amd import features
    memb = MEMB
    bed_path, out = tmp_path / "genes.bed", str(tmp_path / "t.tsv")
    bed_path.write_text(EXAMPLE_BED)
    bed = features.read_bed(str(bed_path))
    counts, positions = np.array([[10, 5, 9, 10, 9], [15, 7, 12, 15, 14], [0, 0, 0, 0, 0]], np.uint64), np.array([10, 15, 0])
    common = ("-b", memb, "-k", "3", "-n", "5", "-a", str(bed_path), "-o", out, "-m")
    r = _memo("features", *common)
    assert (r.returncode, r.stdout) == (0, b"MEMO - features\n"), r.stderr
    text = open(out).read()
    assert text == features.format_features(bed, positions, counts, True)
    assert text == ("chrom\tstart\tend\tname\tpositions\t0\t1\t2\t3\t4\n"
                    "ref_1\t0\t10\ta\t10\t10\t5\t9\t10\t9\n"
                    "ref_1\t5\t20\tb\t15\t15\t7\t12\t15\t14\n"
                    "ref_1\t15\t15\tc\t0\t0\t0\t0\t0\t0\n")
    assert _memo("features", *common, "-f").returncode == 0
    text = open(out).read()
    assert text == features.format_features(bed, positions, features.shares(counts, positions), True)
    assert "ref_1\t0\t10\ta\t10\t1.0\t0.5\t0.9\t1.0\t0.9\n" in text and text.endswith("c\t0\tnan\tnan\tnan\tnan\tnan\n")
    assert _memo("features", *common, "-p", "0.5").returncode == 0
    text = open(out).read()
    assert text == features.format_features(bed, positions, features.calls(counts, positions, 0.5), True)
    assert text.splitlines()[1:] == ["ref_1\t0\t10\ta\t10\t1\t1\t1\t1\t1", "ref_1\t5\t20\tb\t15\t1\t0\t1\t1\t1", "ref_1\t15\t15\tc\t0\t0\t0\t0\t0\t0"]
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    assert _memo("features", *common, "-g", str(genomes)).returncode == 0
    text = open(out).read()
    assert text == features.format_features(bed, positions, counts, True, ["pivot", "g1", "g2", "g3", "g4"])
    assert text.startswith("chrom\tstart\tend\tname\tpositions\tpivot\tg1\tg2\tg3\tg4\n")
    # -i: the k-mers wholly inside: two positions fewer a feature
    assert _memo("features", *common, "-i").returncode == 0
    assert [ln.split("\t")[4] for ln in open(out).read().splitlines()[1:]] == ["8", "13", "0"]
    assert sorted(os.listdir(tmp_path)) == ["genes.bed", "genomes.txt", "t.tsv"]                # written beside its name and renamed


def test_cli_on_a_conservation_index_and_on_a_bed_with_no_features(memo, tmp_path):
    memb, cons, out = MEMB, CONS, str(tmp_path / "t.tsv")
    # the conservation index: one feature 0-20
    whole = tmp_path / "whole.bed"
    whole.write_text("ref_1\t0\t20\n")
    r = _memo("features", "-b", cons, "-k", "3", "-n", "5", "-a", str(whole), "-o", out)
    assert r.returncode == 0 and open(out).read() == "chrom\tstart\tend\tname\tpositions\tsum\tshared\nref_1\t0\t20\t.\t20\t84\t8\n", r.stderr
    r = _memo("features", "-b", cons, "-k", "3", "-n", "5", "-a", str(whole), "-o", out, "-t", "4", "-f")
    assert r.returncode == 0 and open(out).read() == "chrom\tstart\tend\tname\tpositions\tmean\tshared_fraction\nref_1\t0\t20\t.\t20\t4.2\t0.8\n", r.stderr
    # a BED with no features: only the header
    nothing = tmp_path / "nothing.bed"
    nothing.write_text("# no features\n\ntrack name=none\n")
    r = _memo("features", "-b", memb, "-k", "3", "-n", "5", "-a", str(nothing), "-o", out, "-m")
    assert r.returncode == 0 and open(out).read() == "chrom\tstart\tend\tname\tpositions\t0\t1\t2\t3\t4\n", r.stderr
    r = _memo("features", "-b", cons, "-k", "3", "-n", "5", "-a", str(nothing), "-o", out)
    assert r.returncode == 0 and open(out).read() == "chrom\tstart\tend\tname\tpositions\tsum\tshared\n", r.stderr
    assert sorted(os.listdir(tmp_path)) == ["nothing.bed", "t.tsv", "whole.bed"]


def test_cli_says_what_memo_query_raises_and_writes_nothing(memo, tmp_path):
    memb, bed_path, never = MEMB, tmp_path / "genes.bed", str(tmp_path / "never.tsv")
    bed_path.write_text(EXAMPLE_BED)
    r = _memo("features", "-b", memb, "-k", "3", "-n", "2", "-a", str(bed_path), "-o", never, "-m")
    assert r.returncode == 1 and r.stderr.startswith(b"memo features: ") and b"IndexError" in r.stderr and not os.path.exists(never)
    r = _memo("features", "-b", str(tmp_path / "no.parquet"), "-k", "3", "-n", "5", "-a", str(bed_path), "-o", never, "-m")
    assert r.returncode == 1 and r.stderr.startswith(b"memo features: ") and not os.path.exists(never)
    assert sorted(os.listdir(tmp_path)) == ["genes.bed"]
