"""The row block and the fold of the wide-tile sweep (memo_sweep_cons3t.hip: R4; memo_sweep_dense.h: group_rows4; memo_sweep_fold.h:
r4_fold12) on level blocks of 12, 4 and 1.  A row of n positions takes blocks of S = 12 (n >= 12), 4 (n = 4 .. 11) or 1 (n < 4) at its
first cell, at its end - S and, where n > 2S, at first + S; the fold takes a block of 12 as three blocks of 4.  Hand-made rows put
every (k - 1, n) alone on its cells, at the edges of a tile and at the 1024-cell wrap, in piles, and at the ends of a tile's slice
inside a wave's piece of 64 groups; every result is compared bit for bit with the oracle and with the doubling tiles
(MEMO_OPT_WIDE_TILES 0), and every counted query is one the wide-tile kernel answered (memo_index_info_t: last_variant 3, six rows per
group, last_tile_width).

The generator's n are uniform on 1 .. k - 1, so tests/test_wide_tiles.py already meets every n -- but only in piles (five rows per
position), where a row's missing block is as a rule covered by a neighbour's."""
import numpy as np
import pytest

OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_WIDE_TILES = 3, 4, 7
N_DOCS = 100


def _widths(k, cells):
    """positions per tile of the table-driven sweep (tests/test_wide_tiles.py)"""
    km1 = k - 1
    hl, hr = (km1 + 3) & ~3, (km1 + 31 + 3) & ~3
    return (cells - hl - hr) // 32 * 32


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def _rows(start, n, k, annot):
    """start-sorted int64 columns of rows that write n positions at k: end - start = k - 1 - n.  Besides them one row per position with
    an overlap of 40, which writes at no k <= 32: the dense rows answer where an index holds a row per position or more, and the view
    of k's class leaves those out again -- its groups hold the rows asked for and nothing else"""
    start, n, annot = (np.asarray(a, np.int64) for a in (start, n, annot))
    fill = np.arange(int(start.max()) + 64, dtype=np.int64)
    s = np.concatenate([start, fill])
    ov = np.concatenate([k - 1 - n, np.full(len(fill), 40, np.int64)])
    o = np.concatenate([annot, np.ones(len(fill), np.int64)])
    order = np.argsort(s, kind="stable")
    return s[order], (s + ov)[order], o[order]


def _index(memo, s, e, o, k):
    """the rows as dense rows, their six-row view of k's class built and placed, one warm query behind it (a view with dead groups:
    the query that copies it without them)"""
    ix = memo.DeviceIndex.from_host(s, e, o)
    ix.pack(keep_wide=False)
    ix.pack_dense(keep_packed=False)
    ix.set_option(OPT_VIEW_ROWS, 6)
    ix.set_option(OPT_BUILD_COST_PCT, 0)
    ix.prepare(k, N_DOCS)
    ix.conservation(0, int(s[-1]) + 64, k, N_DOCS, np.uint8)
    return ix


def _check(ix, oracle, s, e, o, windows, k, dtypes=(np.uint8,)):
    """every window both ways against the oracle; returns the number of wide-tile queries counted"""
    tw, counted = _widths(k, 1664), 0
    for qs, qe in windows:
        want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
        for dt in dtypes:
            got = ix.conservation(qs, qe, k, N_DOCS, dt)
            inf = ix.info()
            assert ix.set_option(OPT_WIDE_TILES, 0) == 1
            ref = ix.conservation(qs, qe, k, N_DOCS, dt)
            inf0 = ix.info()
            assert ix.set_option(OPT_WIDE_TILES, 1) == 0
            assert (inf["last_variant"], inf["last_view_rows_per_group"], inf["last_tile_width"]) == (3, 6, tw), (k, inf)
            assert (inf0["last_variant"], inf0["last_tile_width"]) == (3, _widths(k, 1024)), (k, inf0)
            assert got.dtype == dt and np.array_equal(got, want), (k, qs, qe, dt, int(np.argmax(got != want)))
            assert np.array_equal(ref, got), (k, qs, qe, dt)
            counted += 1
    return counted


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(17, 33))
def test_every_length_alone(k, memo, oracle):
    """every n = 1 .. k - 1 at every start mod 32 (and so mod 4), 97 positions or more from the next row: a row's own blocks alone decide
    its cells, so a block too few, too many or misplaced shows -- the level choice, the three cells and the n > 2S test at n = 3, 4, 8,
    9, 11, 12, 24, 25, 31.  Rows spread over eight wide tiles (cells on both sides of the 1024-cell wrap); annots cycle through 1 .. 99.
    The pivot is longer than five tiles (128 positions per row): every residue for every n at every k, not over the set of k"""
    n = np.repeat(np.arange(1, k), 32)
    r = np.tile(np.arange(32), k - 1)
    i = np.arange(len(n))
    # (row i at 128 * slot + its residue; the slots dealt so that neighbouring n and residues do not sit side by side)
    slot = (i * 37) % len(n)
    assert len(np.unique(slot)) == len(n)
    start = 64 + 128 * slot + r
    s, e, o = _rows(start, n, k, 1 + i % 99)
    assert np.diff(np.sort(start)).min() >= 97
    L = int(s[-1]) + 64
    with _index(memo, s, e, o, k) as ix:
        dts = (np.uint8, np.uint16) if k in (17, 25, 31) else (np.uint8,)
        assert _check(ix, oracle, s, e, o, [(0, L), (67, L - 129)], k, dts) == 2 * len(dts)


def _edge_rows(k, seed):
    """rows with starts within 40 of every multiple of the wide tile's width inside a pivot of five tiles and of cell 1024 of each
    tile; n from a seeded generator, every n of 1 .. k - 1 present"""
    tw = _widths(k, 1664)
    rng = np.random.default_rng(seed)
    anchors = [t * tw for t in range(1, 5)] + [t * tw + 1024 for t in range(5)]
    start = np.concatenate([a + np.arange(-40, 41) for a in anchors])
    n = rng.integers(1, k, len(start))
    n[:k - 1] = rng.permutation(np.arange(1, k))
    return _rows(start, n, k, rng.integers(1, 100, len(start))), tw


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 17))
def test_tile_edges_and_the_wrap(k, memo, oracle):
    """rows around every tile boundary and every tile's wrap point: the halo cells, the first chunk's context lanes (three, not four),
    the group that passes g_wrap.  Windows: the pivot, and ones that begin and end off the 4-position raster inside one tile, at its
    edges, and across each boundary"""
    counted = 0
    for seed in (1, 2):
        (s, e, o), tw = _edge_rows(k, seed)
        L = 5 * tw
        windows = [(0, L), (3, L - 5)]
        for t in range(1, 5):
            windows += [(t * tw + 1, t * tw + 42), (t * tw - 39, t * tw - 2), (t * tw - 37, t * tw + 41),
                        (t * tw + 1024 - 41, t * tw + 1024 + 39), (t * tw + 5, (t + 1) * tw - 7)]
        windows += [(1024 - 33, 1024 + 35), (1, tw - 1)]
        with _index(memo, s, e, o, k) as ix:
            counted += _check(ix, oracle, s, e, o, windows, k, (np.uint8, np.uint16) if seed == 1 else (np.uint8,))
    assert counted == 24 * 3


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 21, 17))
def test_piles(k, memo, oracle):
    """300 rows in 200 positions, three times: inside a tile, across a tile boundary, across a tile's wrap point.  The lanes of one
    row instruction meet on cells: a wrong block of one row is a wrong minimum"""
    tw = _widths(k, 1664)
    rng = np.random.default_rng(100 + k)
    start = np.concatenate([a + rng.integers(0, 200, 300) for a in (tw + 300, 3 * tw - 100, 2 * tw + 1024 - 100)])
    n = rng.integers(1, k, len(start))
    s, e, o = _rows(start, n, k, rng.integers(1, 100, len(start)))
    L = 5 * tw
    with _index(memo, s, e, o, k) as ix:
        windows = [(0, L), (tw + 301, tw + 498), (3 * tw - 99, 3 * tw + 97), (2 * tw + 1024 - 97, 2 * tw + 1024 + 99)]
        assert _check(ix, oracle, s, e, o, windows, k, (np.uint8, np.uint16)) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 30, 17))
def test_partial_last_piece(k, memo, oracle):
    """tiles whose slices hold 1, 63, 64 and 65 groups: the slice ends 1, 63, 64 and 1 groups into a wave's piece of 64, so the row
    block's form with the mask by group number runs with one lane, with all but one, not at all, and in a second wave (k = 30: a view
    whose cap is not k - 1, the form with the row's own test besides).  A bucket of 32 positions with one row is one group, with seven
    rows two; the rows of a bucket have one length and different starts, so none is dead.  Tiles 1, 3, 5 and 7 hold them in their first
    buckets; the bucket a tile shares with the next one's halo stays empty"""
    tw = _widths(k, 1664)
    nb = tw // 32 - 1
    start, n = [], []
    total = 0
    for tile, groups in ((1, 1), (3, 63), (5, 64), (7, 65)):
        twos = max(groups - nb, 0)                                 # buckets with seven rows: two groups
        ones = groups - 2 * twos
        assert 0 <= ones and ones + twos <= nb
        for b in range(ones + twos):
            base = tile * tw + 32 * b
            rows = 7 if b < twos else 1
            start += [base + 3 + 4 * j for j in range(rows)]
            n += [1 + (b + tile) % (k - 1)] * rows
        total += groups
    i = np.arange(len(start))
    s, e, o = _rows(start, n, k, 1 + i % 99)
    L = 9 * tw
    with _index(memo, s, e, o, k) as ix:
        assert _check(ix, oracle, s, e, o, [(0, L), (tw + 2, 8 * tw - 3)], k) == 2
        assert ix.info()["last_rows_read"] == 6 * total, (k, ix.info()["last_rows_read"], total)


@pytest.mark.gpu
def test_config3_rows(memo, oracle):
    """a short run of config 3's rows at k = 31, whole window, on the copy without dead groups: the sweep reads fewer slots than on
    the flagged view, and the same bytes come out"""
    from memo_amd import synth
    n, L, k = N_DOCS, 60_000, 31
    num, den = synth.rows_per_position(n)
    ix, (r0, r1) = synth.device_index(0, L, k, n, L, pack="dense")
    s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, n)
    with ix:
        ix.prepare(k, n)
        ix.conservation(0, L, k, n, np.uint8)                      # (the flagged view: prepare hands out no copy)
        flagged = ix.info()["last_rows_read"]
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        ix.conservation(0, L, k, n, np.uint8)                      # (the query that builds the copy)
        assert _check(ix, oracle, s, e, o, [(0, L)], k) == 1
        assert 0 < ix.info()["last_rows_read"] < flagged, (ix.info()["last_rows_read"], flagged)
