"""The deciding copy of a live copy (memo_view_build.hip: deciding_view_copy; MEMO_OPT_VIEW_DECIDING, option 8): for ONE k the rows that
hold the least (order, slot) at some position they cover.  The minimum over them is the minimum over all the rows, so every result
stays what it was -- while the sweep reads a fifth of the groups at k = 31.

The copy is checked against a NumPy twin that works on the exported live copy (every slot of a group is a row: the places a bucket
left empty hold a copy of one of its rows); the twin against brute force, on the CPU.  Results are checked against the oracle's closed
form and, byte for byte, against the same query with the option at 0.  A slot (start s, overlap ov) covers the n = k - 1 - ov positions
[s - n, s); which slot a position keeps does not change when all intervals move alike, so the twin need not know where the sweep puts
them.

The rule (memo_view.hip: deciding_rows): the live copy must have answered ASK_AFTER queries in a row at one k before the next one
builds the copy -- at MEMO_OPT_BUILD_COST_PCT 0 too."""
import numpy as np
import pytest

OPT_VIEWS, OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_VIEW_DECIDING = 1, 3, 4, 8
ASK_AFTER = 32          # memo_view.hip: kDecidingAskAfter
N_DOCS = 100
TILES = 12
LOSER_BUCKETS = 40


def _widths(k, cells=1664):
    """positions per tile of the table-driven sweep (tests/test_wide_tiles.py)"""
    km1 = k - 1
    hl, hr = (km1 + 3) & ~3, (km1 + 31 + 3) & ~3
    return (cells - hl - hr) // 32 * 32


def test_the_option_is_documented_and_numbered():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "memo_amd.h")).read()
    assert re.search(r"#define MEMO_OPT_VIEW_DECIDING 8\b", text)
    assert "MEMO_OPT_VIEW_DECIDING    1 (default)" in text
    debug = open(os.path.join(os.path.dirname(__file__), "..", "include", "memo_amd_debug.h")).read()
    assert "memo_debug_view_deciding(" in debug and "memo_debug_export_deciding(" in debug


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------

def winners(start, ov, order, km1):
    """the slots that hold the least (order, slot) at some position they cover, ascending: slot i covers [start - n, start), n = km1 - ov"""
    start, ov, order = (np.asarray(a, np.int64) for a in (start, ov, order))
    n = km1 - ov
    slots = np.flatnonzero(n > 0)
    if not len(slots):
        return slots
    lens = n[slots]
    first = np.cumsum(lens) - lens
    pos = np.repeat(start[slots] - lens, lens) + (np.arange(int(lens.sum())) - np.repeat(first, lens))
    R = len(start)
    key = np.repeat(order[slots] * (R + 1) + slots, lens)
    base = int(pos.min())
    best = np.full(int(pos.max()) - base + 1, np.iinfo(np.int64).max)
    np.minimum.at(best, pos - base, key)
    return np.unique(best[best != np.iinfo(np.int64).max] % (R + 1))


def _brute(start, ov, order, km1):
    won = set()
    for p in range(int(min(start)) - km1 - 1, int(max(start)) + 1):
        cover = [(order[i], i) for i in range(len(start)) if start[i] - (km1 - ov[i]) <= p < start[i]]
        if cover:
            won.add(min(cover)[1])
    return np.array(sorted(won), np.int64)


def test_the_twin_against_brute_force():
    """random rows with ties, duplicates, rows that cover nothing, gaps; and the hand cases the GPU tests name"""
    rng = np.random.default_rng(11)
    for case in range(40):
        km1 = int(rng.choice([30, 29, 16, 3]))
        m = int(rng.integers(1, 120))
        start = np.sort(rng.integers(40, 40 + int(rng.choice([30, 200, 900])), m))
        ov = rng.integers(0, km1 + 4, m)
        order = rng.integers(1, int(rng.choice([2, 5, 99])) + 1, m)
        assert np.array_equal(winners(start, ov, order, km1), _brute(start, ov, order, km1)), case
    km1 = 30
    assert list(winners([50, 50], [20, 20], [5, 5], km1)) == [0]                          # equal order, one interval: the lower slot
    assert list(winners([50, 55], [20, 20], [5, 5], km1)) == [0, 1]                       # equal order, overlapping: both
    assert list(winners([60, 55], [10, 25], [3, 9], km1)) == [0]                          # nested, the inner one of higher order
    assert list(winners([60, 55], [10, 25], [3, 2], km1)) == [0, 1]
    assert list(winners([100] * 30, km1 - np.arange(1, 31), np.arange(1, 31), km1)) == list(range(30))
    assert list(winners([70, 80], [35, 30], [1, 2], km1)) == []                           # rows that cover nothing


# ---- the device ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def memo():
    """the package on the A/B library (product objects + memo_debug.o), as tests/test_tile_pairs_gpu.py sets it up"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    _lib.use_ab(True)
    yield memo_amd
    _lib.use_ab(False)


def _slots(view):
    """a six-row view as exported -> per slot: start, overlap, order, bucket, lo | annot << 10; and the table in slots"""
    table = view[1]
    ng = int(table[-1]) // 6
    g = view[0].reshape(-1, 4)[:ng].astype(np.int64)
    x, y, z, w = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    lo = np.stack([x & 1023, y & 1023, z & 1023, w & 1023, (x >> 10) & 1023, (w >> 10) & 1023], 1)
    an = np.stack([x >> 24, y >> 24, z >> 24, w >> 24, (y >> 10) & 255, (z >> 10) & 255], 1)
    bucket = np.searchsorted(table[1:] // 6, np.arange(ng), side="right")
    assert np.array_equal((z >> 18) & 31, bucket & 31)                                     # a group carries its bucket mod 32
    assert not (x & (1 << 20)).any()                                                       # no group is flagged
    b6 = np.repeat(bucket, 6)
    lo, an = lo.ravel(), an.ravel()
    return b6 * 32 + (lo & 31), lo >> 5, an, b6, lo | (an << 10), table


def _check_copy(ix, k):
    """the deciding copy of k == what the twin makes of the exported live copy, bucket by bucket: the winners in slot order, the places
    the last group leaves empty a copy of the bucket's last winner, the table the scan of ceil(winners / 6).  Returns (winners per
    bucket, groups of the live copy, groups of the deciding copy)"""
    live, dec = ix.export_view(k, 6), ix.export_deciding(k)
    assert live is not None and dec is not None, k
    s, ov, o, b6, val, table = _slots(live)
    ds, dov, do, db6, dval, dtable = _slots(dec)
    won = winners(s, ov, o, k - 1)
    nbk = len(table) - 1
    c = np.bincount(b6[won], minlength=nbk)
    groups = (c + 5) // 6
    want_table = 6 * np.concatenate(([0], np.cumsum(groups)))
    assert np.array_equal(dtable, want_table), k
    assert dec[2] == len(won), (k, dec[2], len(won))
    want = np.empty(int(want_table[-1]), np.int64)
    nth = np.arange(len(won)) - np.repeat(np.cumsum(c) - c, c)
    want[want_table[b6[won]] + nth] = val[won]
    has = np.flatnonzero(c)
    pad = 6 * groups[has] - c[has]
    last = val[won][np.cumsum(c)[has] - 1]
    at = np.repeat(want_table[has] + c[has], pad) + (np.arange(int(pad.sum())) - np.repeat(np.cumsum(pad) - pad, pad))
    want[at] = np.repeat(last, pad)
    assert np.array_equal(dval, want), (k, int(np.argmax(dval != want)))
    return c, int(table[-1]) // 6, int(dtable[-1]) // 6


def _both_ways(ix, want, qs, qe, k, dt, live_slots, dec_slots, tw=None, pairs=None):
    """one window on the deciding copy == the oracle == the same query with the option at 0 (the live copy), byte for byte"""
    got = ix.conservation(qs, qe, k, N_DOCS, dt)
    inf, per_group = ix.info(), ix.debug_last_tiles_per_group()
    assert ix.set_option(OPT_VIEW_DECIDING, 0) == 1
    ref = ix.conservation(qs, qe, k, N_DOCS, dt)
    inf0, per_group0 = ix.info(), ix.debug_last_tiles_per_group()
    assert ix.set_option(OPT_VIEW_DECIDING, 1) == 0
    assert got.dtype == dt and np.array_equal(got, want.astype(dt)), (k, qs, qe, dt, int(np.argmax(got != want)))
    assert np.array_equal(ref, got), (k, qs, qe, dt, int(np.argmax(ref != got)))
    assert (inf["last_rows_read"], inf0["last_rows_read"]) == (dec_slots, live_slots), (k, inf, inf0)
    for i in (inf, inf0):
        assert (i["last_variant"], i["last_view_rows_per_group"], i["last_tile_width"]) == (3, 6, tw or _widths(k)), (k, qs, qe, i)
    if pairs:
        assert (per_group, per_group0) == (2, 2), (k, qs, qe, per_group, per_group0)
    return 1


def _ask(ix, L, k, times):
    for _ in range(times):
        ix.conservation(0, L, k, N_DOCS, np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 30, 17))
def test_config3_over_twelve_wide_tiles(k, memo, oracle):
    """config 3's generator: nothing is made before the live copy has answered ASK_AFTER queries, even at cost 0; the next query makes the
    copy; its rows are the twin's winners; every window's result is the oracle's and the live copy's, on the pair kernel"""
    from memo_amd import synth
    tw = _widths(k)
    L = TILES * tw
    from fractions import Fraction
    num, den = synth.rows_per_position(N_DOCS, Fraction(5, 100))
    ix, (r0, r1) = synth.device_index(0, L, k, N_DOCS, L, pack="dense")
    with ix:
        rows = oracle.synth_rows(r0, r1 - r0, num, den, N_DOCS)
        whole = oracle.conservation(*oracle.filter_rows(*rows, 0, L, k), 0, L, k, N_DOCS, literal=False)
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        ix.prepare(k, N_DOCS)
        ix.conservation(0, L, k, N_DOCS, np.uint8)                    # (the query that makes the live copy)
        live_slots = ix.info()["last_rows_read"]
        _ask(ix, L, k, ASK_AFTER - 1)
        ix.prepare(k, N_DOCS)                                         # (prepare never makes it, and is no query of the run)
        _ask(ix, L, k, 1)
        assert ix.debug_view_deciding(k) == (False, 0), k
        assert ix.info()["last_rows_read"] == live_slots and ix.export_deciding(k) is None
        ix.prepare(k, N_DOCS)
        assert ix.debug_view_deciding(k) == (False, 0), k
        got = ix.conservation(0, L, k, N_DOCS, np.uint8)              # ASK_AFTER answered: this one makes it
        assert ix.debug_view_deciding(k) == (True, 1), k
        assert np.array_equal(got, whole.astype(np.uint8))
        c, live_groups, dec_groups = _check_copy(ix, k)
        assert 6 * live_groups == live_slots and 5 * dec_groups <= 4 * live_groups, (k, live_groups, dec_groups)   # (it spares a fifth, or is dropped)
        print("k = %d: %d groups of the live copy, %d of the deciding copy over %d tiles (%.1f -> %.1f a tile); %d winners"
              % (k, live_groups, dec_groups, TILES, live_groups / TILES, dec_groups / TILES, int(c.sum())))
        windows = [(0, L), (3 * tw + 1, 8 * tw + 2), (tw - 3, 2 * tw + 5), (5, L - 7),                 # off the 4-position raster
                   (4 * tw + 700, 4 * tw + 1100), (5 * tw + 33, 5 * tw + 34), (4 * tw, 5 * tw)]       # inside one tile
        counted = 0
        for qs, qe in windows:
            for dt in (np.uint8, np.uint16):
                counted += _both_ways(ix, whole[qs:qe], qs, qe, k, dt, live_slots, 6 * dec_groups, pairs=True)
        assert counted == 2 * len(windows)
        assert ix.debug_view_deciding(k) == (True, 1), k             # (nothing was made again)


def _rows(start, n, k, annot):
    """start-sorted int64 columns of rows that write n positions at k: end - start = k - 1 - n.  Besides them one row per position with
    an overlap of 40, which writes at no k <= 32 and which the view of k's class leaves out (tests/test_three_block_rows.py)"""
    start, n, annot = (np.asarray(a, np.int64) for a in (start, n, annot))
    lo = int(start.min()) - 64
    fill = np.arange(lo, int(start.max()) + 64, dtype=np.int64)
    s = np.concatenate([start, fill])
    ov = np.concatenate([k - 1 - n, np.full(len(fill), 40, np.int64)])
    o = np.concatenate([annot, np.ones(len(fill), np.int64)])
    order = np.argsort(s, kind="stable")
    return s[order], (s + ov)[order], o[order]


def _hand_made(k, D=0):
    """(start, n, order, {name: bucket}) of the hand-made rows at k, moved by D: every case in buckets of its own, two tiles apart"""
    km1, tw = k - 1, _widths(k)
    rows, where = [], {}

    def put(name, base, triples):
        where[name] = base >> 5
        rows.extend((base + ds, n, o) for ds, n, o in triples)
    T = 2 * tw                                                        # (a multiple of 64: bases sit at bucket boundaries)
    m = min(10, km1 // 2)
    put("equal order, one interval", 1 * T + 32, [(20, m, 5), (20, m, 5)])
    put("equal order, overlapping", 2 * T + 32, [(20, m, 5), (20 + m // 2, m, 5)])
    put("nested, the inner one loses", 3 * T + 64, [(4, 2, 9), (6, m, 3)])
    put("nested, the inner one wins", 4 * T + 64, [(4, 2, 2), (6, m, 3)])
    put("wins its leftmost position only", 5 * T + 64, [(10, m, 7), (14, m + 3, 2)])
    put("wins its rightmost position only", 6 * T + 64, [(20, m, 7), (19, m + 3, 2)])
    # a row that starts in one tile (and in one run of 960 cells) and wins only positions of the tile (run) before it
    put("across a tile boundary", 7 * tw, [(3, m, 7), (m, m, 2)])
    put("across a run boundary", 960 * ((8 * T) // 960 + 1), [(3, m, 7), (m, m, 2)])
    put("every length on one start", 9 * T + 32, [(31, n, n) for n in range(1, km1 + 1)])
    put("six winners", 10 * T, [(2 * i + 1, 1, 11 + i) for i in range(6)])
    put("seven winners", 11 * T, [(2 * i + 1, 1, 11 + i) for i in range(7)])
    put("thirteen winners", 12 * T, [(2 * i + 1, 1, 11 + i) for i in range(13)])
    # a bucket whose every row is dead (contained by a row of order 1 in the next bucket): the flagged view has a dead group, so that
    # the class gets a live copy at all (tests/test_live_views.py)
    put("a dead bucket", 13 * T, [(31, n, 7 + n) for n in (1, 2, 3, 4, 5, 6, 7, 8)] + [(32, min(km1, 12), 1)])
    # rows that win nowhere and that no single row contains (two rows of order 1 cover them between them), eight to a bucket: they stay in
    # the live copy, and leaving them out is what makes the deciding copy worth keeping (it must spare a fifth of the groups)
    for j in range(LOSER_BUCKETS):
        put("losers %d" % j, 14 * T + 64 * j, [(10, 10, 1), (20, 10, 1)] + [(12 + i, 6, 50 + i) for i in range(4)] + [(12 + i, 8, 60 + i) for i in range(4)])
    s, n, o = (np.array(col, np.int64) for col in zip(*rows))
    return s + D, n, o, where


def _hand_index(memo, s, e, o, k):
    ix = memo.DeviceIndex.from_host(s, e, o)
    ix.pack(keep_wide=False)
    ix.pack_dense(keep_packed=False)
    ix.set_option(OPT_VIEW_ROWS, 6)
    ix.set_option(OPT_BUILD_COST_PCT, 0)
    return ix


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 30, 17))
def test_hand_made_rows(k, memo, oracle):
    start, n, order, where = _hand_made(k)
    s, e, o = _rows(start, n, k, order)
    L, tw, km1 = int(s[-1]) + 64, _widths(k), k - 1
    with _hand_index(memo, s, e, o, k) as ix:
        ix.prepare(k, N_DOCS)
        _ask(ix, L, k, ASK_AFTER + 2)                                 # (the live copy, ASK_AFTER on it, the deciding copy)
        assert ix.debug_view_deciding(k) == (True, 1), k
        c, live_groups, dec_groups = _check_copy(ix, k)
        want = {"equal order, one interval": 1, "equal order, overlapping": 2, "nested, the inner one loses": 1, "nested, the inner one wins": 2,
                "wins its leftmost position only": 2, "wins its rightmost position only": 2, "across a tile boundary": 2,
                "across a run boundary": 2, "every length on one start": km1, "six winners": 6, "seven winners": 7, "thirteen winners": 13}
        for name, count in want.items():
            assert c[where[name]] == count, (k, name, c[where[name]], count)
        b = where["a dead bucket"]
        assert c[b] == 0 and c[b + 1] == 1, (k, c[b], c[b + 1])
        for j in range(LOSER_BUCKETS):
            assert c[where["losers %d" % j]] == 2, (k, j)
        assert c.sum() == sum(want.values()) + 1 + 2 * LOSER_BUCKETS and (c == 0).sum() > len(c) - 20 - LOSER_BUCKETS      # uncovered stretches, empty buckets
        windows = [(0, L), (3, L - 5), (7 * tw - 40, 7 * tw + 41), (where["across a run boundary"] * 32 - 50, where["across a run boundary"] * 32 + 50),
                   (where["every length on one start"] * 32 - 33, where["every length on one start"] * 32 + 64)]
        for qs, qe in windows:
            w = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
            for dt in (np.uint8, np.uint16):
                _both_ways(ix, w, qs, qe, k, dt, 6 * live_groups, 6 * dec_groups)


@pytest.mark.gpu
def test_starts_past_two_to_the_32(memo, oracle):
    """the hand-made rows moved by 2^32 (a multiple of every raster: bucket, tile, run): the same groups as at the origin, the table moved"""
    k, D = 31, 2 ** 32
    made = {}
    for d in (0, D):
        start, n, order, where = _hand_made(k, d)
        s, e, o = _rows(start, n, k, order)
        lo, hi = int(s[0]), int(s[-1]) + 64
        with _hand_index(memo, s, e, o, k) as ix:
            ix.prepare(k, N_DOCS)
            for _ in range(ASK_AFTER + 2):
                ix.conservation(lo, hi, k, N_DOCS, np.uint8)
            assert ix.debug_view_deciding(k) == (True, 1), d
            for qs, qe in ((lo, hi), (lo + 7 * _widths(k) - 40, lo + 7 * _widths(k) + 105)):
                want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
                got = ix.conservation(qs, qe, k, N_DOCS, np.uint16)
                assert np.array_equal(got, want), (d, qs, qe, int(np.argmax(got != want)))
            groups, table, rows = ix.export_deciding(k)
            made[d] = (groups[: 4 * (int(table[-1]) // 6)].copy(), table[d >> 5:].copy(), rows, int(table[: (d >> 5) + 1].max()))
    assert np.array_equal(made[D][0], made[0][0]) and made[D][2] == made[0][2]
    assert np.array_equal(made[D][1], made[0][1]) and made[D][3] == 0


@pytest.mark.gpu
def test_the_rule(memo, oracle):
    """a query at the class's other k starts the run again and reads the live copy; the first k then reuses its copy; option 0 never makes
    one; dropping the views drops it"""
    k, other = 31, 30
    start, n, order, where = _hand_made(k)
    s, e, o = _rows(start, n, k, order)
    L = int(s[-1]) + 64
    want = {q: oracle.conservation(*oracle.filter_rows(s, e, o, 0, L, q), 0, L, q, N_DOCS, literal=False) for q in (k, other)}
    with _hand_index(memo, s, e, o, k) as ix:
        ix.prepare(k, N_DOCS)
        _ask(ix, L, k, 1)                                             # (makes the live copy)
        live_slots = ix.info()["last_rows_read"]
        assert ix.set_option(OPT_VIEW_DECIDING, 0) == 1
        _ask(ix, L, k, ASK_AFTER + 8)                                 # option 0: never, and no query of a run
        assert ix.debug_view_deciding(k) == (False, 0)
        assert ix.set_option(OPT_VIEW_DECIDING, 1) == 0
        with pytest.raises(Exception):
            ix.set_option(OPT_VIEW_DECIDING, 2)
        _ask(ix, L, k, ASK_AFTER - 4)
        got = ix.conservation(0, L, other, N_DOCS, np.uint16)         # the other k of the class: the run starts again
        assert np.array_equal(got, want[other]) and ix.info()["last_rows_read"] == live_slots
        _ask(ix, L, k, ASK_AFTER)
        assert ix.debug_view_deciding(k) == (False, 0)                # (ASK_AFTER - 4 + ASK_AFTER queries at k, none made)
        _ask(ix, L, k, 1)
        assert ix.debug_view_deciding(k) == (True, 1)
        dec_slots = ix.info()["last_rows_read"]
        assert dec_slots < live_slots
        before = ix.info()
        got = ix.conservation(0, L, other, N_DOCS, np.uint16)         # the other k reads the live copy ...
        assert np.array_equal(got, want[other]) and ix.info()["last_rows_read"] == live_slots
        assert ix.debug_view_deciding(other) == (False, 1) and ix.export_deciding(other) is None
        got = ix.conservation(0, L, k, N_DOCS, np.uint16)             # ... and the first k finds its copy again, without a pass
        assert np.array_equal(got, want[k]) and ix.info()["last_rows_read"] == dec_slots
        assert ix.debug_view_deciding(k) == (True, 1) and ix.info()["last_view_ms"] == 0
        # the other k for ASK_AFTER queries: its copy takes the place of the first k's (one per class)
        _ask(ix, L, other, ASK_AFTER + 1)
        assert ix.debug_view_deciding(other) == (True, 2) and ix.debug_view_deciding(k) == (False, 2)
        _check_copy(ix, other)
        got = ix.conservation(0, L, other, N_DOCS, np.uint16)
        assert np.array_equal(got, want[other]) and ix.info()["last_rows_read"] < live_slots
        # dropping the views drops it, with its bytes
        assert ix.set_option(OPT_VIEWS, 0) == 1
        assert ix.debug_view_deciding(other) == (False, 2) and ix.export_deciding(other) is None
        assert ix.info()["side_bytes"] < before["side_bytes"] and ix.info()["views_resident"] == 0
        assert ix.set_option(OPT_VIEWS, 1) == 0
        got = ix.conservation(0, L, k, N_DOCS, np.uint16)
        assert np.array_equal(got, want[k])
