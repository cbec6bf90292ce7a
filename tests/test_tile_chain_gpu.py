"""The wide-tile sweep's shortened chain (memo_sweep_cons3t.hip: sweep_conservation_wide_kernel): the head that arrives in registers
with the tile descriptor in one scalar load, a wave's two fold chunks in flight together (memo_sweep_fold.h:
fold_chunks_once_or_twice), and the store without the window test in tiles off the window's edges.

Config 3's generator at 100 genomes over ten wide tiles, prepared as tests/test_wide_tiles.py prepares it (the class's view, its copy
without dead groups).  Every result is compared with the oracle's closed form -- one sweep of the whole pivot per k, of which a
window is a slice: a row writes left of its start only, so the rows a window leaves out (start <= qs, start >= qe + k) reach none of
its positions; windows that leave the pivot get an oracle run of their own -- and, byte for byte, with the same query on the doubling
tiles (MEMO_OPT_WIDE_TILES 0).  Every counted query is one the wide-tile kernel answered (memo_index_info_t.last_tile_width)."""
import numpy as np
import pytest

OPT_BUILD_COST_PCT, OPT_WIDE_TILES = 3, 7
N_DOCS = 100
TILES = 10
KS = (17, 31, 32)


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


class _Case:
    """one k: the index, its rows on the host, the closed form over the whole pivot"""

    def __init__(self, oracle, k):
        from memo_amd import synth
        self.k, self.tw = k, _widths(k, 1664)
        self.L = L = TILES * self.tw
        num, den = synth.rows_per_position(N_DOCS)
        self.ix, (r0, r1) = synth.device_index(0, L, k, N_DOCS, L, pack="dense")
        self.rows = oracle.synth_rows(r0, r1 - r0, num, den, N_DOCS)
        self.whole = oracle.conservation(*oracle.filter_rows(*self.rows, 0, L, k), 0, L, k, N_DOCS, literal=False)
        self.oracle = oracle
        self.ix.set_option(OPT_BUILD_COST_PCT, 0)
        self.ix.prepare(k, N_DOCS)
        self.ix.conservation(0, L, k, N_DOCS, np.uint8)        # (the class's view, its copy without dead groups)

    def want(self, qs, qe):
        if 0 <= qs and qe <= self.L:
            return self.whole[qs:qe]
        return self.oracle.conservation(*self.oracle.filter_rows(*self.rows, qs, qe, self.k), qs, qe, self.k, N_DOCS, literal=False)

    def check(self, windows, dtypes=(np.uint8, np.uint16)):
        """every window both ways against the oracle; the number of queries the wide-tile kernel answered"""
        ix, k, wide = self.ix, self.k, 0
        for qs, qe in windows:
            want = self.want(qs, qe)
            assert len(want) == qe - qs
            for dt in dtypes:
                got = ix.conservation(qs, qe, k, N_DOCS, dt)
                inf = ix.info()
                assert ix.set_option(OPT_WIDE_TILES, 0) == 1
                ref = ix.conservation(qs, qe, k, N_DOCS, dt)
                inf0 = ix.info()
                assert ix.set_option(OPT_WIDE_TILES, 1) == 0
                assert got.dtype == dt and np.array_equal(got, want), (k, qs, qe, dt, int(np.argmax(got != want)))
                assert np.array_equal(ref, got), (k, qs, qe, dt)
                if k <= 31:                                     # (k = 32: no six-row view of its class, tests/test_wide_tiles.py)
                    assert (inf["last_variant"], inf["last_view_rows_per_group"], inf["last_tile_width"]) == (3, 6, self.tw), (k, qs, qe, inf)
                    assert inf0["last_tile_width"] == _widths(k, 1024), (k, inf0)
                    wide += 1
                else:
                    assert inf["last_tile_width"] in (0, self.tw, _widths(k, 1024)), inf
        return wide


@pytest.fixture(scope="module")
def cases(memo, oracle):
    made = {}

    def get(k):
        if k not in made:
            made[k] = _Case(oracle, k)
        return made[k]
    yield get
    for c in made.values():
        c.ix.close()


def test_the_widths():
    assert (_widths(31, 1664), _widths(17, 1664), _widths(32, 1664)) == (1568, 1600, 1568)
    # a chunk of the fold: 61 lanes of four cells; a wave's second chunk begins 976 cells on
    assert 4 * (64 - 3) == 244 and 4 * 244 == 976


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_fold_and_store(k, cases):
    """window starts at a tile boundary + 0, 1, 2, 3, 5; lengths around every edge of the fold and the store: a few cells, the end of
    the first chunk (244 cells), of the second and the fourth wave's, where a wave's second chunk begins (976), the tile's end, two
    tiles and a cell"""
    c = cases(k)
    W = c.tw
    lengths = [1, 3, 4, 5, 243, 244, 245, 487, 488, 489, 975, 976, 977, W - 1, W, W + 1, 2 * W + 1]
    windows = [(2 * W + d, 2 * W + d + n) for d in (0, 1, 2, 3, 5) for n in lengths]
    assert c.check(windows) == (2 * len(windows) if k <= 31 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_window_edges_inside_tiles(k, cases):
    """a window wholly inside one tile (its first tile is its last); a last tile cut one position in; a first tile cut at W - 1;
    whole tiles between two edge tiles; a window of whole tiles (no edge tile at all)"""
    c = cases(k)
    W = c.tw
    windows = [(4 * W + 700, 4 * W + 1100), (4 * W + 33, 4 * W + 34), (3 * W, 5 * W + 1), (3 * W + W - 1, 6 * W), (W + 7, 8 * W - 9),
               (2 * W, 7 * W), (0, c.L)]
    assert c.check(windows) == (2 * len(windows) if k <= 31 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (17, 31))
def test_head(k, cases):
    """windows of 1, 7, 8, 9 and 17 tiles from tile 0 and from tile 3: tile_abs0 != 0, workgroups past ntiles that exit (the grid is
    eight times ceil(ntiles / 8)), the rounding of tiles_per_xcd; a window that runs past the index's last row (the table's empty
    slices); a query so far out that its tiles' numbers are clamped to the table's last entry"""
    c = cases(k)
    W = c.tw
    windows = [(t0 * W, (t0 + n) * W) for t0 in (0, 3) for n in (1, 7, 8, 9, 17)]
    windows += [(c.L - W - 5, c.L + 3 * W + 3), (c.L + 40 * W + 3, c.L + 42 * W + 1)]
    assert c.check(windows, (np.uint8,)) == len(windows)
    assert c.check([(3 * W, 12 * W)], (np.uint16,)) == 1
