"""The tail the unclipped conservation sweeps share (memo_sweep_fold.h: the folds in registers, fold_store_chunks, store_cells4; memo_sweep.h:
pack_cells4), forced family by family on one synthetic index of 100 000 positions at 5 rows per position and compared bit for bit with the
oracle's closed form.  The index is built three ways, so that every packed format rides through the tail --

    60 genomes     8-bit annots in the row word (TOP 24), uint8 and uint16 results
    300 genomes    12-bit annots (TOP 20)
    5000 genomes   the 16-bit order column (TOP 0)

-- and as dense rows at 60 and at 300 genomes for the table-driven kernel and its nine-bit form.  Every family runs with a small tile
(the window spans three tiles or more) on windows that begin at every residue mod 4 and are of every length mod 4 (the cell-by-cell edge
path, the whole-quartet store, the store at an address off the 4-position raster), on one of 3 positions, one inside a single tile and one
that begins left of position 0; after every query memo_index_info_t says which family (last_sweep) and which kernel of the dense rows
(last_variant) answered.

Combinations that do not reach the kernel named, and why (everything else below runs and is counted):
    table-driven kernel, a window that begins at a negative position (five-row groups, six-row groups, wide tiles; k = 9, 17, 31): the
        tile table starts at position 0; the library answers with sweep_conservation_halo3_kernel (last_variant 0), whose tail is the
        same halo_fold_store_dpp -- asserted as such
    wide tiles at k = 9: the radix-4 arrays of the table-driven kernel take k - 1 = 16 .. 31 only; k = 9 on a six-row view is the
        six-row case
    nine-bit form (300 genomes) on six-row groups and wide tiles: six-row groups hold eight-bit annots; the nine-bit form runs on
        five-row groups"""
import numpy as np
import pytest

OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_WIDE_TILES = 3, 4, 7
LENGTH = 100_000
NUM, DEN = 5, 1                   # rows per position (memo_amd/synth.py: start_i = 1 + floor(i * DEN / NUM))
Q0 = 40_000                       # where the windows sit: far from both ends of the index
BUCKET = 32                       # positions per bucket (bucket_shift 5, what the six-row views need)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture
def ab(memo):
    """the A/B library (product objects + memo_debug.o): kernel families and tile shapes on demand"""
    from memo_amd import _lib
    _lib.use_ab(True)
    yield _lib
    _lib.use_ab(False)


_ROWS = {}


def _rows(oracle, n_docs):
    """the index's rows on the host, once per genome count"""
    if n_docs not in _ROWS:
        _ROWS[n_docs] = oracle.synth_rows(0, NUM * (LENGTH - 1) // DEN, NUM, DEN, n_docs)
    return _ROWS[n_docs]


def _index(memo, oracle, n_docs):
    s, e, o = _rows(oracle, n_docs)
    return memo.DeviceIndex.synthetic(len(s), 0, NUM, DEN, n_docs, bucket_shift=5), (s, e, o)


def _tile(km1, cells=None, doubling=False, at_least=256):
    """(level array size to ask for, positions per tile): the smallest array the launchers take as it is -- a tile of whole buckets, at
    least half as long as its two halos together (memo_sweep_cons.hip: level_tile and the doubling tile).  The doubling arrays come in
    powers of two (clipped_width rounds another size down, the launcher then doubles it until a tile fits): asked for as such"""
    hl, hr = (km1 + 3) & ~3, (km1 + BUCKET - 1 + 3) & ~3
    sizes = (cells,) if cells else [ls for ls in range(at_least, 8193, 64) if not doubling or ls & (ls - 1) == 0]
    for ls in sizes:
        tw = (ls - hl - hr) // BUCKET * BUCKET
        if tw >= BUCKET and 2 * tw >= hl + hr:
            return ls, tw
    raise AssertionError(km1)


def _windows(tw, negative=True):
    """[(name, qs, qe)]: four windows over three tiles and more with qs mod 4 = 0 .. 3 and (qe - qs) mod 4 = 1, 2, 3, 0; 3 positions;
    inside one tile; from a negative position"""
    t0 = (Q0 // tw + 1) * tw                                        # a tile boundary (tiles are aligned at position 0)
    out = []
    for r in range(4):
        qs = t0 - 8 + r
        qs += (r - qs) % 4
        out.append(("qs%%4=%d" % r, qs, qs + 3 * tw + 16 + (r + 1) % 4))
        assert qs % 4 == r and (out[-1][2] - qs) % 4 == (r + 1) % 4
    out.append(("three", t0 + 5, t0 + 8))
    out.append(("one tile", t0 + 3, t0 + tw - 2))
    if negative:
        out.append(("negative", -37, 2 * tw + 2))
    return out


def _want(oracle, rows, qs, qe, k, n_docs):
    s, e, o = rows
    lo, hi = np.searchsorted(s, qs - 1), np.searchsorted(s, qe + k + 1)   # (the filter sees qs < start < qe + k)
    return oracle.conservation(*oracle.filter_rows(s[lo:hi], e[lo:hi], o[lo:hi], qs, qe, k), qs, qe, k, n_docs, literal=False)


# (family, last_sweep, scatter, k - 1, waves, smallest array): doubling folds in registers up to seven levels -- 0, 1, 1, 2, 4, 8, 16 context
# lanes -- and through LDS and store_conservation at eight; radix-4 on one to four arrays; mixed on every array and on the level plan's.
# The small doubling arrays run with one wave per tile (the launcher's choice below 1024 cells); one case with four waves on arrays of
# 2048 cells, where every wave walks two chunks or more: the stride of fold_store_chunks over the waves
PACKED_CASES = [("doubling", 2, 2, km1, 0, 256) for km1 in (1, 3, 7, 15, 31, 63, 127, 200)] + \
               [("doubling, four waves", 2, 2, 31, 4, 2048)] + \
               [("radix-4", 3, 3, km1, 0, 256) for km1 in (3, 9, 40, 200)] + \
               [("mixed, all arrays", 4, 4, km1, 0, 256) for km1 in (16, 40, 200)] + \
               [("mixed, level plan", 4, 5, km1, 0, 256) for km1 in (16, 40, 200)]


def test_tile_arithmetic():
    """the tiles this module expects of the launchers, at the sizes it asks for (the library reports no tile width for the packed
    families: the windows below are laid out on these)"""
    assert [_tile(km1, doubling=True) for km1 in (1, 31, 63, 127, 200)] == [(256, 192), (256, 160), (256, 96), (512, 224), (1024, 576)]
    assert _tile(31, doubling=True, at_least=2048) == (2048, 1952)
    assert [_tile(km1) for km1 in (3, 40, 200)] == [(256, 192), (256, 128), (704, 256)]
    assert (_widths(31, 1664), _widths(31, 512), _widths(9, 512)) == (1568, 416, 448)


@pytest.mark.gpu
@pytest.mark.parametrize("n_docs,fmt,dtypes", [(60, 4, (np.uint8, np.uint16)), (300, 12, (np.uint16,)), (5000, 6, (np.uint16,))])
def test_packed_rows_every_tail(n_docs, fmt, dtypes, memo, oracle, ab):
    ix, rows = _index(memo, oracle, n_docs)
    ran = 0
    with ix:
        ix.pack(keep_wide=False)
        assert ix.info()["packed_format"] == fmt
        for family, sweep, scatter, km1, waves, at_least in PACKED_CASES:
            k = km1 + 1
            ls, tw = _tile(km1, doubling=scatter == 2, at_least=at_least)
            ix.debug_set_tuning(ls, waves, 0, 0, scatter)
            for name, qs, qe in _windows(tw):
                want = _want(oracle, rows, qs, qe, k, n_docs)
                for dt in dtypes:
                    got = ix.conservation(qs, qe, k, n_docs, dt)
                    assert ix.info()["last_sweep"] == sweep, (family, km1, name, ix.info()["last_sweep"])
                    assert got.dtype == dt and np.array_equal(got, want.astype(dt)), (family, km1, name, qs, qe, dt)
                    ran += 1
        ix.debug_set_tuning()
    assert ran == len(PACKED_CASES) * 7 * len(dtypes)


def _widths(k, cells):
    """positions per tile of the table-driven sweep (tests/test_wide_tiles.py)"""
    return _tile(k - 1, cells)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("n_docs,dtypes", [(60, (np.uint8, np.uint16)), (300, (np.uint16,))])
def test_dense_rows_every_tail(n_docs, dtypes, memo, oracle, ab):
    """the table-driven kernel (last_sweep 5; last_variant 2 on five-row groups, 3 on six-row groups) at k = 9, 17, 31: five-row groups
    (all the dense rows: row source 9), six-row groups (the view of k's class, doubling tiles) and wide tiles (the same view on radix-4
    arrays of 1664 cells, k = 17 and 31); 300 genomes: the nine-bit form, five-row groups"""
    ix, rows = _index(memo, oracle, n_docs)
    ran = 0
    with ix:
        ix.pack(keep_wide=False)
        ix.pack_dense(keep_packed=False)
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        shapes = [("five-row groups", 5, 0)] + ([("six-row groups", 6, 0), ("wide tiles", 6, 1)] if n_docs <= 255 else [])
        for k in (9, 17, 31):
            for shape, rpg, wide in shapes:
                if wide and k == 9:
                    continue                                           # (listed above: radix-4 arrays take k - 1 = 16 .. 31)
                ix.debug_set_tuning(512, 0, 0, 9 if rpg == 5 else 0, 0)
                ix.set_option(OPT_VIEW_ROWS, rpg)
                ix.set_option(OPT_WIDE_TILES, wide)
                if rpg == 6:
                    ix.prepare(k, n_docs)
                    ix.conservation(0, LENGTH, k, n_docs, dtypes[0])     # (a view with dead groups: the query that copies it without them)
                tw = _widths(k, 1664 if wide else 512)
                for name, qs, qe in _windows(tw):
                    want = _want(oracle, rows, qs, qe, k, n_docs)
                    for dt in dtypes:
                        got = ix.conservation(qs, qe, k, n_docs, dt)
                        inf = ix.info()
                        assert inf["last_sweep"] == 5, (shape, k, name, inf)
                        if name == "negative":                         # (listed above: no tile table left of position 0)
                            assert inf["last_variant"] == 0, (shape, k, inf)
                        else:
                            assert (inf["last_variant"], inf["last_tile_width"]) == (2 if rpg == 5 else 3, tw), (shape, k, name, inf)
                        assert got.dtype == dt and np.array_equal(got, want.astype(dt)), (shape, k, name, qs, qe, dt)
                        ran += 1
        ix.debug_set_tuning()
    assert ran == (3 * len(shapes) - (1 if n_docs <= 255 else 0)) * 7 * len(dtypes)
