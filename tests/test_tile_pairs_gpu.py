"""The wide tiles' pair kernel (memo_sweep_cons3t.hip: sweep_conservation_wide_pair_kernel): one workgroup sweeps the tiles 2 j and
2 j + 1 of the pivot raster behind one head -- one descriptor load of 64 bytes, both slices requested at once, each into half a batch
of registers -- tile A first, tile B after it in the same level arrays.

Every result is checked three ways: against the oracle's closed form, byte for byte against the same query with pairs switched off
(memo_debug_set_tuning, scatter bit 11) and byte for byte against the doubling tiles (MEMO_OPT_WIDE_TILES 0).  Every counted query is one
the pair kernel answered (memo_debug_last_tiles_per_group == 2) unless the case says otherwise.  The indexes are config 3's generator
over twelve wide tiles, prepared as tests/test_tile_chain_gpu.py prepares it, and hand-made rows as tests/test_three_block_rows.py
makes them."""
import numpy as np
import pytest

OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_VIEW_PLACES, OPT_WIDE_TILES = 3, 4, 5, 7
PAIRS_OFF = 1 << 11
N_DOCS = 100
TILES = 12
KS = (17, 31, 32)


def _widths(k, cells):
    """positions per tile of the table-driven sweep (tests/test_wide_tiles.py)"""
    km1 = k - 1
    hl, hr = (km1 + 3) & ~3, (km1 + 31 + 3) & ~3
    return (cells - hl - hr) // 32 * 32


@pytest.fixture(scope="module")
def memo():
    """the package on the A/B library (product objects + memo_debug.o): the switch that turns pairs off, the entry that says who answered"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    _lib.use_ab(True)
    yield memo_amd
    _lib.use_ab(False)


def _three_ways(ix, want, qs, qe, k, dt, pairs=True):
    """one window: the pair kernel's bytes == the oracle's == one tile per workgroup's == the doubling tiles'.  Returns 1 (a counted
    query).  pairs: whether the launcher is expected to take the pair kernel"""
    tw = _widths(k, 1664)
    got = ix.conservation(qs, qe, k, N_DOCS, dt)
    inf, per_group = ix.info(), ix.debug_last_tiles_per_group()
    ix.debug_set_tuning(scatter=PAIRS_OFF)
    single = ix.conservation(qs, qe, k, N_DOCS, dt)
    inf1, per_group1 = ix.info(), ix.debug_last_tiles_per_group()
    ix.debug_set_tuning()
    assert ix.set_option(OPT_WIDE_TILES, 0) == 1
    ref = ix.conservation(qs, qe, k, N_DOCS, dt)
    inf0, per_group0 = ix.info(), ix.debug_last_tiles_per_group()
    assert ix.set_option(OPT_WIDE_TILES, 1) == 0
    assert len(want) == qe - qs
    assert got.dtype == dt and np.array_equal(got, want), (k, qs, qe, dt, int(np.argmax(got != want)))
    assert np.array_equal(single, got), (k, qs, qe, dt, int(np.argmax(single != got)))
    assert np.array_equal(ref, got), (k, qs, qe, dt, int(np.argmax(ref != got)))
    for i in (inf, inf1):
        assert (i["last_variant"], i["last_view_rows_per_group"], i["last_tile_width"]) == (3, 6, tw), (k, qs, qe, i)
    assert inf0["last_tile_width"] == _widths(k, 1024), (k, inf0)
    assert (per_group, per_group1, per_group0) == (2 if pairs else 1, 1, 1), (k, qs, qe, per_group, per_group1, per_group0)
    return 1


class _Case:
    """one k of config 3's generator: the index, its rows on the host, the closed form over the whole pivot"""

    def __init__(self, oracle, k, density=None, places=True):
        from fractions import Fraction
        from memo_amd import synth
        density = density or Fraction(5, 100)
        self.k, self.tw = k, _widths(k, 1664)
        self.L = L = TILES * self.tw
        num, den = synth.rows_per_position(N_DOCS, density)
        self.ix, (r0, r1) = synth.device_index(0, L, k, N_DOCS, L, density=density, pack="dense")
        self.rows = oracle.synth_rows(r0, r1 - r0, num, den, N_DOCS)
        self.whole = oracle.conservation(*oracle.filter_rows(*self.rows, 0, L, k), 0, L, k, N_DOCS, literal=False)
        self.oracle = oracle
        self.ix.set_option(OPT_BUILD_COST_PCT, 0)
        if not places:
            self.ix.set_option(OPT_VIEW_PLACES, 0)              # (no dead-group flags, no copy: every row of the class)
        self.ix.prepare(k, N_DOCS)
        self.ix.conservation(0, L, k, N_DOCS, np.uint8)        # (the class's view, its copy without dead groups)

    def want(self, qs, qe):
        if 0 <= qs and qe <= self.L:
            return self.whole[qs:qe]
        return self.oracle.conservation(*self.oracle.filter_rows(*self.rows, qs, qe, self.k), qs, qe, self.k, N_DOCS, literal=False)

    def check(self, windows, dtypes=(np.uint8, np.uint16), pairs=True):
        ix, k, counted = self.ix, self.k, 0
        for qs, qe in windows:
            want = self.want(qs, qe)
            for dt in dtypes:
                if k <= 31:                                     # (k = 32: no six-row view of its class, tests/test_wide_tiles.py)
                    counted += _three_ways(ix, want, qs, qe, k, dt, pairs)
                else:
                    got = ix.conservation(qs, qe, k, N_DOCS, dt)
                    assert got.dtype == dt and np.array_equal(got, want), (k, qs, qe, dt)
        return counted


@pytest.fixture(scope="module")
def cases(memo, oracle):
    made = {}

    def get(k, density=None, places=True):
        if (k, density, places) not in made:
            made[k, density, places] = _Case(oracle, k, density, places)
        return made[k, density, places]
    yield get
    for c in made.values():
        c.ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_window_placement(k, cases):
    """windows that start at an even tile (a whole first pair) and at an odd tile (its A half absent), at the tile boundary + 0, 1, 3, 5;
    1, 2, 3 and 5 tiles long, +- 1 position: they end after an A half (B absent), after a B half, one position into the next half and
    one short of it; windows that lie inside one half, A's and B's; the whole pivot"""
    c = cases(k)
    W = c.tw
    lengths = [n * W + d for n in (1, 2, 3, 5) for d in (-1, 0, 1)]
    windows = [(t0 * W + off, t0 * W + off + n) for t0 in (2, 3) for off in (0, 1, 3, 5) for n in lengths]
    assert c.check(windows, (np.uint8,)) == (len(windows) if k <= 31 else 0)
    inside = [(4 * W + 700, 4 * W + 1100), (5 * W + 700, 5 * W + 1100), (4 * W + 33, 4 * W + 34), (5 * W + 33, 5 * W + 34),
              (4 * W, 5 * W), (5 * W, 6 * W), (0, c.L), (3 * W + 1, 8 * W + 2)]
    assert c.check(inside) == (2 * len(inside) if k <= 31 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (17, 31))
def test_pairs_at_the_ends_of_a_window(k, cases):
    """windows of 1, 2, 7, 8, 9, 16 and 17 tiles from tile 0 and from tile 3: pairs past the window that exit (the grid is eight times
    ceil(pairs / 8)), the rounding of pairs_per_xcd, one pair more than the tiles' halves when the window starts at an odd tile; a
    window that runs past the index's last row (the table's empty slices); windows so far out that their pairs are clamped to the
    table's last pair, from an even and from an odd tile"""
    c = cases(k)
    W = c.tw
    windows = [(t0 * W, (t0 + n) * W) for t0 in (0, 3) for n in (1, 2, 7, 8, 9, 16, 17)]
    windows += [(c.L - W - 5, c.L + 3 * W + 3), (c.L - 2 * W - 5, c.L + 4 * W + 3)]
    windows += [(c.L + 40 * W + 3, c.L + 42 * W + 1), (c.L + 41 * W + 3, c.L + 43 * W + 1), (c.L + 41 * W + 3, c.L + 41 * W + 9)]
    assert c.check(windows, (np.uint8,)) == len(windows)
    assert c.check([(3 * W, 12 * W), (c.L + 41 * W + 3, c.L + 44 * W + 1)], (np.uint16,)) == 2


@pytest.mark.gpu
def test_the_launchers_rule(cases):
    """pairs where the groups of TWO tiles stay under kPairMaxGroups = 418, one tile per workgroup above: config 3's live copy (about
    180 groups a tile), the live copy at 10 rows per 100 genome-positions (about 240), and the generator at 3 per 100 with the view
    swept as built, without places and so without a copy (about 410); the groups per tile worked out as the launcher does from
    what the sweep read.  All are wide tiles (under kR4MaxGroups = 543 groups a tile)"""
    from fractions import Fraction
    k = 31
    seen = set()
    for density, places in ((None, True), (Fraction(10, 100), True), (Fraction(3, 100), False)):   # (None: config 3's own 5 per 100)
        c = cases(k, density, places)
        W = c.tw
        c.ix.conservation(0, c.L, k, N_DOCS, np.uint8)
        inf = c.ix.info()
        assert inf["last_tile_width"] == W, inf
        span = c.rows[0].max() - c.rows[0].min() + 1.0
        pair_groups = inf["last_rows_read"] / 6.0 * 2 * W / span
        assert abs(pair_groups - 418.0) > 20.0, pair_groups        # (no case sits on the threshold)
        pairs = pair_groups < 418.0
        seen.add(pairs)
        assert c.check([(0, c.L), (3 * W + 5, 10 * W - 3)], pairs=pairs) == 4
    assert seen == {True, False}


# ---- hand-made rows ---------------------------------------------------------------------------------------------------------------------

def _rows(start, n, k, annot):
    """start-sorted int64 columns of rows that write n positions at k: end - start = k - 1 - n.  Besides them one row per position with
    an overlap of 40, which writes at no k <= 32 and which the view of k's class leaves out (tests/test_three_block_rows.py)"""
    start, n, annot = (np.asarray(a, np.int64) for a in (start, n, annot))
    fill = np.arange(int(start.max()) + 64, dtype=np.int64)
    s = np.concatenate([start, fill])
    ov = np.concatenate([k - 1 - n, np.full(len(fill), 40, np.int64)])
    o = np.concatenate([annot, np.ones(len(fill), np.int64)])
    order = np.argsort(s, kind="stable")
    return s[order], (s + ov)[order], o[order]


def _index(memo, s, e, o, k):
    ix = memo.DeviceIndex.from_host(s, e, o)
    ix.pack(keep_wide=False)
    ix.pack_dense(keep_packed=False)
    ix.set_option(OPT_VIEW_ROWS, 6)
    ix.set_option(OPT_BUILD_COST_PCT, 0)
    ix.prepare(k, N_DOCS)
    ix.conservation(0, int(s[-1]) + 64, k, N_DOCS, np.uint8)
    return ix


def _check_rows(ix, oracle, s, e, o, windows, k, dtypes=(np.uint8, np.uint16)):
    counted = 0
    for qs, qe in windows:
        want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
        for dt in dtypes:
            counted += _three_ways(ix, want, qs, qe, k, dt)
    return counted


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 17))
@pytest.mark.parametrize("where", ("A", "B", "both"))
def test_the_wrap_in_either_half(k, where, memo, oracle):
    """a half's slice passes the 1024-cell wrap (g_wrap) where it holds rows 1024 positions or more past its tile's start: pairs whose
    A half alone does, whose B half alone does, and both.  The other half's rows all lie in its first 900 positions"""
    tw = _widths(k, 1664)
    rng = np.random.default_rng(7 * k + len(where))
    start = []
    for pair in (1, 2, 3):
        for half, tile in (("A", 2 * pair), ("B", 2 * pair + 1)):
            lo, hi = (40, tw - 40) if where in (half, "both") else (40, 900)
            start.append(tile * tw + rng.integers(lo, hi, 260))
            if where in (half, "both"):
                start.append(tile * tw + 1024 + np.arange(-36, 37))  # (around the wrap itself)
    start = np.concatenate(start)
    n = rng.integers(1, k, len(start))
    s, e, o = _rows(start, n, k, rng.integers(1, 100, len(start)))
    L = 9 * tw
    with _index(memo, s, e, o, k) as ix:
        windows = [(0, L), (2 * tw + 3, 8 * tw - 5), (3 * tw, 6 * tw), (4 * tw + 1024 - 41, 5 * tw + 1024 + 39)]
        assert _check_rows(ix, oracle, s, e, o, windows, k) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 30, 17))
def test_partial_last_piece_in_either_half(k, memo, oracle):
    """slices of 1, 63, 64 and 65 groups in A halves (tiles 2, 4, 6, 8) and in B halves (tiles 3, 5, 7, 9): the mask by group number
    with one lane, with all but one, not at all, and in a second wave, beside a half with another count (k = 30: a view whose cap is
    not k - 1).  Rows as tests/test_three_block_rows.py::test_partial_last_piece makes them"""
    tw = _widths(k, 1664)
    nb = tw // 32 - 1
    start, n, total = [], [], 0
    for tile, groups in ((2, 1), (3, 63), (4, 64), (5, 65), (6, 63), (7, 1), (8, 65), (9, 64)):
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
    L = 11 * tw
    with _index(memo, s, e, o, k) as ix:
        assert _check_rows(ix, oracle, s, e, o, [(0, L), (2 * tw + 2, 10 * tw - 3), (3 * tw, 9 * tw)], k, (np.uint8,)) == 3
        ix.conservation(0, L, k, N_DOCS, np.uint8)
        assert ix.info()["last_rows_read"] == 6 * total, (k, ix.info()["last_rows_read"], total)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 17))
def test_a_pile_in_the_halo(k, memo, oracle):
    """300 rows on eight positions just right of the boundary between the tiles 2 and 3 and again between 3 and 4: they lie in both
    neighbours' slices (the left tile's right halo), inside one pair and across two pairs, and are scattered for both tiles"""
    tw = _widths(k, 1664)
    rng = np.random.default_rng(300 + k)
    start = np.concatenate([t * tw + 2 + rng.integers(0, 8, 300) for t in (3, 4)] + [2 * tw + rng.integers(40, tw - 40, 200)])
    n = rng.integers(1, k, len(start))
    s, e, o = _rows(start, n, k, rng.integers(1, 100, len(start)))
    L = 6 * tw
    with _index(memo, s, e, o, k) as ix:
        windows = [(0, L), (2 * tw + 1, 5 * tw - 1), (3 * tw - 40, 3 * tw + 41), (4 * tw - 40, 4 * tw + 41), (3 * tw - 29, 3 * tw)]
        assert _check_rows(ix, oracle, s, e, o, windows, k) == 10


@pytest.mark.gpu
@pytest.mark.parametrize("half", ("A", "B"))
@pytest.mark.parametrize("buckets", (4, 8))
def test_a_pile_past_half_a_batch(half, buckets, memo, oracle):
    """a half whose slice outgrows its registers (512 groups): the pair does its tiles one after the other, each with its own loads --
    four buckets of 30 rows on every position (640 groups: one batch), eight (1280: two batches).  A row of n written positions has
    order n: the longer overlap has the lower order, so no row contains another of lower order and every row stays in the copy.
    Equality with the oracle, with one tile per workgroup and with the doubling tiles"""
    k = 31
    tw = _widths(k, 1664)
    tile = 4 if half == "A" else 5
    pos = tile * tw + 320 + np.arange(32 * buckets)
    start = np.repeat(pos, k - 1)
    n = np.tile(np.arange(1, k), len(pos))
    other = (tile ^ 1) * tw + 100 + 7 * np.arange(150)                 # (the other half: a slice of its own, well under the limit)
    far = np.array([11 * tw + 5])                                      # (a long index: few groups per tile on average, so pairs are taken)
    start = np.concatenate([start, other, far])
    n = np.concatenate([n, 1 + np.arange(len(other)) % (k - 1), [3]])
    s, e, o = _rows(start, n, k, n)
    L = 12 * tw
    with _index(memo, s, e, o, k) as ix:
        windows = [(0, L), (4 * tw + 3, 6 * tw - 5), (tile * tw + 300, tile * tw + 340 + 32 * buckets)]
        assert _check_rows(ix, oracle, s, e, o, windows, k) == 6
        ix.conservation(0, L, k, N_DOCS, np.uint8)
        assert ix.info()["last_rows_read"] >= 6 * (160 * buckets), ix.info()["last_rows_read"]
