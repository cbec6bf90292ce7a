"""The run copy of a deciding copy (memo_view_build.hip: run_view_copy; MEMO_OPT_VIEW_RUNS, option 9): for ONE k the conservation results
themselves, run-coded -- per bucket of 32 positions a start mask (bit i: result[i] differs from result[i - 1]; bit 0 always) and the byte
offset of the bucket's first value, per run one byte (255: no row covers it); every group of eight buckets begins its values at a multiple
of four.  A query at that k decodes its window from the copy (memo_sweep_runs.hip; info last_variant 4) instead of sweeping rows.

The copy is checked array for array against a NumPy twin that is handed the closed-form answer; the twin against a brute-force expansion, on
the CPU.  Every window is checked three ways: against the oracle and, byte for byte, against the same query with the option at 0 (the
deciding copy's answer).

The rule (memo_view.hip: run_rows): the deciding copy must have answered ASK_AFTER queries in a row at one k before the next one makes the
run copy -- at MEMO_OPT_BUILD_COST_PCT 0 too."""
import numpy as np
import pytest

from tests.test_deciding_rows_gpu import _hand_index, _hand_made, _widths

OPT_VIEWS, OPT_VIEW_BUDGET_PCT, OPT_BUILD_COST_PCT, OPT_WIDE_TILES, OPT_VIEW_DECIDING, OPT_VIEW_RUNS = 1, 2, 3, 7, 8, 9
DEC_ASK_AFTER = 32      # memo_view.hip: kDecidingAskAfter
ASK_AFTER = 32          # memo_view.hip: kRunsAskAfter
N_DOCS = 100
TILES = 12
GROUP = 8               # memo_view.h: kRunGroup


def test_the_option_is_documented_and_numbered():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "memo_amd.h")).read()
    assert re.search(r"#define MEMO_OPT_VIEW_RUNS 9\b", text)
    assert "MEMO_OPT_VIEW_RUNS        1 (default)" in text
    debug = open(os.path.join(os.path.dirname(__file__), "..", "include", "memo_amd_debug.h")).read()
    assert "memo_debug_view_runs(" in debug and "memo_debug_export_runs(" in debug
    assert "memo_debug_view_runs" not in text and "memo_debug_export_runs" not in text     # (the A/B library's alone)


# ---- the twin -----------------------------------------------------------------------------------------------------------------------------

def twin(res):
    """results (a byte a position, 255: no row; whole groups of 8 buckets) -> masks, offsets, values, runs"""
    r = np.asarray(res, np.uint8).reshape(-1, 32)
    assert len(r) % GROUP == 0
    start = np.ones(r.shape, bool)
    start[:, 1:] = r[:, 1:] != r[:, :-1]
    masks = (start.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    c = start.sum(1)
    gc = c.reshape(-1, GROUP)
    gbytes = (gc.sum(1) + 3) // 4 * 4
    offsets = ((np.cumsum(gbytes) - gbytes)[:, None] + np.cumsum(gc, 1) - gc).ravel()
    values = np.zeros(int(gbytes.sum()), np.uint8)
    rank = (np.cumsum(start, 1) - 1)[start]
    values[np.repeat(offsets, c) + rank] = r[start]
    return masks, offsets.astype(np.uint32), values, int(c.sum())


def expand(masks, offsets, values):
    """brute force: position by position"""
    out = []
    for m, off in zip(masks, offsets):
        j = int(off) - 1
        for i in range(32):
            j += (int(m) >> i) & 1
            out.append(values[j])
    return np.array(out, np.uint8)


def test_the_twin_against_brute_force():
    rng = np.random.default_rng(5)
    for case in range(30):
        groups = int(rng.integers(1, 5))
        n = 256 * groups
        cuts = np.sort(rng.choice(np.arange(1, n), int(rng.integers(0, n // int(rng.choice([2, 8, 60])))), replace=False))
        vals = rng.choice([255, 255, 1, 2, 3, 99, 254], len(cuts) + 1)
        res = np.repeat(vals, np.diff(np.concatenate(([0], cuts, [n])))).astype(np.uint8)
        masks, offsets, values, runs = twin(res)
        assert np.array_equal(expand(masks, offsets, values), res), case
        assert (masks & 1).all() and not (offsets[::GROUP] % 4).any() and runs == int((masks[:, None] >> np.arange(32) & 1).sum())
    # a bucket whose 32 positions are 32 runs; eight of them: 256 values, the most a group holds
    res = np.tile(np.array([3, 4], np.uint8), 128)
    masks, offsets, values, runs = twin(res)
    assert (masks == 0xFFFFFFFF).all() and list(offsets) == list(range(0, 256, 32)) and runs == 256 and np.array_equal(values, res)
    # equal values side by side: one run inside a bucket, two across its boundary; an empty stretch
    res = np.full(512, 255, np.uint8)
    res[40:50] = 7
    res[60:70] = 7
    masks, offsets, values, runs = twin(res)
    assert list(masks[:3]) == [1, (1 << 8) | (1 << 18) | (1 << 28) | 1, 1 | (1 << 6)] and (masks[3:] == 1).all()
    assert list(values[:7]) == [255, 255, 7, 255, 7, 7, 255] and list(offsets[:4]) == [0, 1, 5, 7] and offsets[8] == 12 and runs == 20


# ---- the device ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def memo():
    """the package on the A/B library (product objects + memo_debug.o), as tests/test_deciding_rows_gpu.py sets it up"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    _lib.use_ab(True)
    yield memo_amd
    _lib.use_ab(False)


def closed_form(s, e, o, k, lo, hi):
    """the least order that covers every position of [lo, hi), 255: none -- a row covers [s - n, s), n = k - 1 - (e - s); no end < start here"""
    s, e, o = (np.asarray(a, np.int64) for a in (s, e, o))
    n = np.minimum(k - 1 - (e - s), k - 1)
    keep = n > 0
    s, n, o = s[keep], n[keep], o[keep]
    best = np.full(hi - lo, 255, np.int64)
    if len(s):
        first = np.cumsum(n) - n
        pos = np.repeat(s - n, n) + (np.arange(int(n.sum())) - np.repeat(first, n))
        val = np.repeat(o, n)
        ok = (pos >= lo) & (pos < hi)
        np.minimum.at(best, pos[ok] - lo, val[ok])
    return best.astype(np.uint8)


def _want_copy(s, e, o, k):
    """(first bucket, twin arrays) of the copy an index of these rows gets at k"""
    b0 = (int(s.min()) >> 5) - 1
    buckets = ((int(s.max()) >> 5) - b0 + 1 + GROUP - 1) // GROUP * GROUP
    return b0, twin(closed_form(s, e, o, k, 32 * b0, 32 * (b0 + buckets)))


def _check_copy(ix, s, e, o, k):
    got = ix.export_runs(k)
    assert got is not None, k
    b0, (masks, offsets, values, runs) = _want_copy(s, e, o, k)
    assert (got[4], got[3]) == (b0, runs), (k, got[3:], b0, runs)
    assert np.array_equal(got[0], masks), (k, int(np.argmax(got[0] != masks)))
    assert np.array_equal(got[1], offsets), (k, int(np.argmax(got[1] != offsets)))
    assert np.array_equal(got[2], values), (k, int(np.argmax(got[2] != values)))
    return b0, masks, runs


def _until_run_copy(ix, qs, qe, k, most=2 * (DEC_ASK_AFTER + ASK_AFTER)):
    """same-k queries until the class holds the run copy of k (the live copy, the deciding copy and the run copy on the way)"""
    for _ in range(most):
        if ix.debug_view_runs(k)[0]:
            return
        ix.conservation(qs, qe, k, N_DOCS, np.uint8)
    assert ix.debug_view_runs(k)[0], (k, ix.debug_view_deciding(k), ix.debug_view_runs(k))


def _three_ways(ix, want, qs, qe, k, dt, runs, n_docs=N_DOCS):
    """one window decoded from the run copy == the oracle == the same query with the option at 0 (the deciding copy), byte for byte"""
    got = ix.conservation(qs, qe, k, n_docs, dt)
    inf, pick = ix.info(), ix.debug_last_pick()
    assert ix.set_option(OPT_VIEW_RUNS, 0) == 1
    ref = ix.conservation(qs, qe, k, n_docs, dt)
    inf0, pick0 = ix.info(), ix.debug_last_pick()
    assert ix.set_option(OPT_VIEW_RUNS, 1) == 0
    assert got.dtype == dt and np.array_equal(got, want.astype(dt)), (k, qs, qe, dt, int(np.argmax(got != want)))
    assert np.array_equal(ref, got), (k, qs, qe, dt, int(np.argmax(ref != got)))
    assert (inf["last_variant"], pick["kernel"], inf["last_rows_read"]) == (4, 5, runs), (k, qs, qe, inf, pick)
    assert inf0["last_variant"] == 3 and pick0["kernel"] in (1, 2, 3, 4) and inf0["last_view_rows_per_group"] == 6, (k, qs, qe, inf0, pick0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 30, 17))
def test_config3_over_twelve_wide_tiles(k, memo, oracle):
    """config 3's generator: nothing is made before the deciding copy has answered ASK_AFTER queries, even at cost 0; the next query makes the
    copy; it is the twin's, array for array; every window's result is the oracle's and the deciding copy's"""
    from fractions import Fraction
    from memo_amd import synth
    tw = _widths(k)
    L = TILES * tw
    num, den = synth.rows_per_position(N_DOCS, Fraction(5, 100))
    ix, (r0, r1) = synth.device_index(0, L, k, N_DOCS, L, pack="dense")
    with ix:
        s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, N_DOCS)
        whole = oracle.conservation(*oracle.filter_rows(s, e, o, 0, L, k), 0, L, k, N_DOCS, literal=False)
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        ix.prepare(k, N_DOCS)
        for _ in range(2 * DEC_ASK_AFTER):
            if ix.debug_view_deciding(k)[0]:
                break
            ix.conservation(0, L, k, N_DOCS, np.uint8)
        assert ix.debug_view_deciding(k) == (True, 1), k              # (the query that made it is the first it answered)
        for _ in range(ASK_AFTER - 2):
            ix.conservation(0, L, k, N_DOCS, np.uint8)
        ix.prepare(k, N_DOCS)                                         # (prepare never makes it, and is no query of the count)
        got = ix.conservation(0, L, k, N_DOCS, np.uint8)              # ASK_AFTER answered
        assert ix.debug_view_runs(k) == (False, 0) and ix.export_runs(k) is None and ix.info()["last_variant"] == 3, k
        ix.prepare(k, N_DOCS)
        assert ix.debug_view_runs(k) == (False, 0), k
        side = ix.info()["side_bytes"]
        got = ix.conservation(0, L, k, N_DOCS, np.uint8)              # this one makes it
        inf = ix.info()
        assert ix.debug_view_runs(k) == (True, 1) and (inf["last_variant"], ix.debug_last_pick()["kernel"]) == (4, 5), (k, inf)
        assert inf["last_view_ms"] > 0 and inf["side_bytes"] > side
        assert np.array_equal(got, whole.astype(np.uint8))
        b0, masks, runs = _check_copy(ix, s, e, o, k)
        # the oracle's answer over the positions both know is the closed form the twin was handed
        assert np.array_equal(np.where(whole == N_DOCS, 255, whole), closed_form(s, e, o, k, 0, L))
        print("k = %d: %d runs over %d positions (%.3f a position), %d B of copy; side bytes %d -> %d"
              % (k, runs, 32 * len(masks), runs / (32.0 * len(masks)), inf["side_bytes"] - side, side, inf["side_bytes"]))
        windows = [(0, L), (3 * tw + 1, 8 * tw + 2), (tw - 3, 2 * tw + 5), (5, L - 7),                 # off the 4- and 32-position rasters
                   (4 * tw + 700, 4 * tw + 1100), (5 * tw + 33, 5 * tw + 34), (5 * tw + 35, 5 * tw + 60),   # one position; inside one bucket
                   (4 * tw, 5 * tw)]
        for qs, qe in windows:
            for dt in (np.uint8, np.uint16):
                _three_ways(ix, whole[qs:qe], qs, qe, k, dt, runs)
        assert ix.debug_view_runs(k) == (True, 1), k                  # (nothing was made again)


def _rows(start, n, k, annot, fill_from=None):
    """start-sorted int64 columns of rows that write n positions at k (tests/test_deciding_rows_gpu.py: _rows); the rows of overlap 40 that
    no view of the class keeps begin at fill_from (the least start: a row of the case then reaches below the index's first bucket)"""
    start, n, annot = (np.asarray(a, np.int64) for a in (start, n, annot))
    lo = int(start.min()) if fill_from is None else fill_from
    fill = np.arange(lo, int(start.max()) + 64, dtype=np.int64)
    s = np.concatenate([start, fill])
    ov = np.concatenate([k - 1 - n, np.full(len(fill), 40, np.int64)])
    o = np.concatenate([annot, np.ones(len(fill), np.int64)])
    order = np.argsort(s, kind="stable")
    return s[order], (s + ov)[order], o[order]


def _hand_rows(k, D=0, top=99):
    """the hand-made rows of tests/test_deciding_rows_gpu.py (they give the class its live and deciding copies) and, behind them, this
    format's cases, each in buckets of its own.  The least start is a row's: the copy's first bucket is known here"""
    km1, tw = k - 1, _widths(k)
    start, n, order, where = _hand_made(k)
    rows = []
    first = 32 * 40 + 5                                               # reaches below the index's first bucket (n > 5)
    rows.append((first, min(km1, 12), 9))
    b0 = (first >> 5) - 1
    base = 32 * (((int(start.max()) >> 5) + 8 - b0 + 7) // 8 * 8 + b0)    # (the first bucket of a group of the copy, past everything else)
    where = dict(where)

    def put(name, at, triples):
        where[name] = at >> 5
        rows.extend((at + ds, m, o) for ds, m, o in triples)
    put("32 runs", base + 32 * 3, [(i + 1, 1, 3 + i % 2) for i in range(32)])
    put("a group of 256 runs", base + 256 * 2, [(i + 1, 1, 3 + i % 2 + (top - 3 if i % 64 == 0 else 0)) for i in range(256)])
    m = min(25, km1)
    put("one run over a whole bucket", base + 256 * 4 + 64, [(15, m, 6), (15 + m, m, 6), (15 + 2 * m, m, 6)])   # [15 - m, 15 + 2 m) of one order
    put("equal orders side by side", base + 256 * 5 + 32, [(30, 4, 7), (34, 4, 7)])                            # [26, 34): over a boundary
    put("an empty stretch", base + 256 * 7, [(1, 1, 8)])
    s2, n2, o2 = (np.array(col, np.int64) for col in zip(*rows))
    return np.concatenate([start, s2]) + D, np.concatenate([n, n2]), np.concatenate([order, o2]), where


@pytest.fixture(scope="module")
def hand(memo, oracle):
    """k = 31: the hand-made index with its run copy, its rows, the copy as checked"""
    k = 31
    start, n, order, where = _hand_rows(k)
    s, e, o = _rows(start, n, k, order)
    L = int(s[-1]) + 64
    with _hand_index(memo, s, e, o, k) as ix:
        ix.prepare(k, N_DOCS)
        _until_run_copy(ix, 0, L, k)
        yield ix, (s, e, o), L, where, k


@pytest.mark.gpu
def test_hand_made_buckets(hand):
    ix, (s, e, o), L, where, k = hand
    b0, masks, runs = _check_copy(ix, s, e, o, k)
    assert b0 == (int(s[0]) >> 5) - 1 and masks[0] != 1                                  # a row reaches below the index's first bucket
    c = np.array([bin(int(m)).count("1") for m in masks])
    at = lambda name: where[name] - b0
    assert c[at("32 runs")] == 32
    g = at("a group of 256 runs")
    assert g % GROUP == 0 and (c[g:g + GROUP] == 32).all()
    b = at("one run over a whole bucket")
    assert masks[b] == 1 and masks[b + 1] == 1 and c[b - 1] == 2 and c[b + 2] == 2        # one run goes through buckets b and b + 1
    b = at("equal orders side by side")
    assert c[b] == 2 and c[b + 1] == 2                                                    # [26, 32) and [32, 34): one run cut by the boundary
    b = at("an empty stretch")
    assert (masks[b - 7:b] == 1).all() and c[b] == 2


@pytest.mark.gpu
def test_every_window_three_ways(hand, oracle):
    ix, (s, e, o), L, where, k = hand
    tw, runs = _widths(k), ix.export_runs(k)[3]
    first, last = int(s[0]) - 12, int(s[-1])                          # (about the first and last covered positions)
    g = where["a group of 256 runs"] * 32
    windows = [(0, L), (3, L - 5), (g - 1, g + 258), (g + 1, g + 2), (g + 33, g + 60), (g + 2, g + 250),
               (first - 100, first + 300), (last - 300, last + 100), (last + 5000, last + 9000), (0, max(first - 64, 1)),
               (where["one run over a whole bucket"] * 32 - 7, where["one run over a whole bucket"] * 32 + 131)]
    for qs, qe in windows:
        w = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
        for dt in (np.uint8, np.uint16):
            _three_ways(ix, w, qs, qe, k, dt, runs)


@pytest.mark.gpu
def test_num_docs_is_the_querys(hand, oracle):
    """one copy; num_docs 100, then 99 (the largest order), then 60 -- below some winning orders: the oracle raises and so does the
    library, the copy stays -- then 255 and 254 and, for uint16 results, 300: the copy answers where its deciding copy would, num_docs <= 255, so that
    query is the nine-bit sweep's on the dense rows and only its result is checked"""
    ix, (s, e, o), L, where, k = hand
    runs = ix.export_runs(k)[3]
    for n_docs, dt, decoded in ((100, np.uint8, True), (99, np.uint8, True), (60, np.uint8, False), (100, np.uint16, True),
                                (255, np.uint8, True), (254, np.uint8, True), (255, np.uint16, True), (300, np.uint16, None), (99, np.uint16, True)):
        try:
            want = oracle.conservation(*oracle.filter_rows(s, e, o, 0, L, k), 0, L, k, n_docs, literal=False)
        except oracle.OracleIndexError:
            with pytest.raises(Exception):                            # an order outside the matrix: the library refuses alike
                ix.conservation(0, L, k, n_docs, dt)
            assert not decoded
            continue
        got = ix.conservation(0, L, k, n_docs, dt)
        assert np.array_equal(got, want.astype(dt)), (n_docs, dt, int(np.argmax(got != want)))
        if decoded is not None:
            assert (ix.info()["last_variant"] == 4) == decoded, (n_docs, dt, ix.info())
    assert ix.debug_view_runs(k) == (True, 1) and ix.export_runs(k)[3] == runs


@pytest.mark.gpu
def test_starts_past_two_to_the_32(memo, oracle):
    """the hand-made rows moved by 2^32 (a multiple of every raster): the same copy as at the origin, its first bucket moved"""
    k, D = 31, 2 ** 32
    start, n, order, where = _hand_rows(k, D)
    s, e, o = _rows(start, n, k, order)
    lo, hi = int(s[0]) - 64, int(s[-1]) + 64
    with _hand_index(memo, s, e, o, k) as ix:
        ix.prepare(k, N_DOCS)
        _until_run_copy(ix, lo, hi, k)
        b0, masks, runs = _check_copy(ix, s, e, o, k)
        assert b0 == (D >> 5) + 40 - 1
        for qs, qe in ((lo, hi), (lo + 7 * _widths(k) - 40, lo + 7 * _widths(k) + 105)):
            want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
            for dt in (np.uint8, np.uint16):
                _three_ways(ix, want, qs, qe, k, dt, runs)


@pytest.mark.gpu
def test_an_order_of_255_never_gets_a_copy(memo, oracle):
    k = 31
    start, n, order, where = _hand_rows(k, top=255)
    assert order.max() == 255
    s, e, o = _rows(start, n, k, order)
    L = int(s[-1]) + 64
    want = oracle.conservation(*oracle.filter_rows(s, e, o, 0, L, k), 0, L, k, 255, literal=False)
    with _hand_index(memo, s, e, o, k) as ix:
        ix.prepare(k, 255)
        for _ in range(DEC_ASK_AFTER + 2 * ASK_AFTER + 4):
            got = ix.conservation(0, L, k, 255, np.uint8)
        assert ix.debug_view_deciding(k) == (True, 1) and ix.debug_view_runs(k) == (False, 0)
        assert np.array_equal(got, want.astype(np.uint8)) and ix.info()["last_variant"] == 3


@pytest.mark.gpu
def test_long_rows_are_applied_after_the_decode(memo, oracle):
    """rows with end < start: kept aside by the index and applied to the result after the decode as after a sweep"""
    k = 31
    start, n, order, where = _hand_rows(k)
    s, e, o = _rows(start, n, k, order)
    g = where["a group of 256 runs"] * 32
    ls = np.array([g + 40, g + 300, int(s[0]) + 20], np.int64)        # over the densest group, over an empty stretch, at the copy's first bucket
    le = ls - np.array([25, 60, 5], np.int64)
    lo_ = np.array([1, 2, 1], np.int64)
    s, e, o = (np.concatenate(c) for c in ((s, ls), (e, le), (o, lo_)))
    order_ = np.argsort(s, kind="stable")
    s, e, o = s[order_], e[order_], o[order_]
    L = int(s[-1]) + 64
    with _hand_index(memo, s, e, o, k) as ix:
        assert ix.info()["long_rows"] == 3
        ix.prepare(k, N_DOCS)
        _until_run_copy(ix, 0, L, k)
        runs = ix.export_runs(k)[3]
        for qs, qe in ((0, L), (g + 3, g + 341), (int(ls[2]) - 40, int(ls[2]) + 7)):
            want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, N_DOCS, literal=False)
            for dt in (np.uint8, np.uint16):
                _three_ways(ix, want, qs, qe, k, dt, runs)


@pytest.mark.gpu
def test_the_rule(memo, oracle):
    """a query at the class's other k starts the count again, and so does a change of an option that decides which kernel answers, not one
    of the budget or the cost share; option 0 never makes a copy and leaves one unread; no room: the deciding copy
    answers; dropping the views drops the copy with its bytes"""
    from memo_amd import _lib as ab
    k, other = 31, 30
    start, n, order, where = _hand_rows(k)
    s, e, o = _rows(start, n, k, order)
    L = int(s[-1]) + 64
    want = {q: oracle.conservation(*oracle.filter_rows(s, e, o, 0, L, q), 0, L, q, N_DOCS, literal=False) for q in (k, other)}

    def ask(q, times):
        for _ in range(times):
            got = ix.conservation(0, L, q, N_DOCS, np.uint8)
        assert np.array_equal(got, want[q].astype(np.uint8)), q

    with _hand_index(memo, s, e, o, k) as ix:
        ix.prepare(k, N_DOCS)
        assert ix.set_option(OPT_VIEW_RUNS, 0) == 1
        with pytest.raises(Exception):
            ix.set_option(OPT_VIEW_RUNS, 2)
        with pytest.raises(Exception):
            ix.set_option(OPT_VIEW_RUNS, -1)
        ask(k, 2 + DEC_ASK_AFTER + ASK_AFTER + 8)                     # option 0: never, and no query of a count
        assert ix.debug_view_deciding(k) == (True, 1) and ix.debug_view_runs(k) == (False, 0)
        assert ix.set_option(OPT_VIEW_RUNS, 1) == 0
        ask(k, ASK_AFTER - 4)
        ask(other, 1)                                                 # the other k of the class: the count starts again
        assert ix.info()["last_variant"] == 3
        ask(k, ASK_AFTER)
        assert ix.debug_view_runs(k) == (False, 0)                    # (ASK_AFTER - 4 + ASK_AFTER queries at k, none made: the next one would)
        assert ix.set_option(OPT_WIDE_TILES, 1) == 1                  # an option that decides which kernel answers: the count starts again
        ask(k, ASK_AFTER)
        assert ix.debug_view_runs(k) == (False, 0)
        assert ix.set_option(OPT_VIEW_BUDGET_PCT, 200) == 200         # the budget and the cost share decide neither: the count goes on,
        assert ix.set_option(OPT_BUILD_COST_PCT, 0) == 0              # the next query finds the copy due
        ab.check(ab.lib().memo_debug_fail_side_allocations(1))
        try:
            ask(k, 1)                                                 # due, and no room: the deciding copy answers
            assert ix.debug_view_runs(k) == (False, 0) and ix.info()["last_variant"] == 3
        finally:
            ab.check(ab.lib().memo_debug_fail_side_allocations(0))
        ask(k, 1)                                                     # (cost 0: four times nothing is due at once)
        assert ix.debug_view_runs(k) == (True, 1) and ix.info()["last_variant"] == 4
        before = ix.info()
        ask(other, 1)                                                 # the other k reads the live copy; the copy stays ...
        assert ix.info()["last_variant"] == 3 and ix.debug_view_runs(other) == (False, 1)
        ask(k, 1)                                                     # ... and answers again, without a pass
        assert ix.info()["last_variant"] == 4 and ix.info()["last_view_ms"] == 0 and ix.debug_view_runs(k) == (True, 1)
        assert ix.set_option(OPT_VIEW_RUNS, 0) == 1
        ask(k, 1)                                                     # option 0: it stays, unread
        assert ix.info()["last_variant"] == 3 and ix.debug_view_runs(k) == (True, 1)
        assert ix.set_option(OPT_VIEW_RUNS, 1) == 0
        ask(other, DEC_ASK_AFTER + 1)                                 # the other k's deciding copy takes the place of k's: the run copy goes with it
        assert ix.debug_view_deciding(other) == (True, 2) and ix.debug_view_runs(k) == (False, 1) and ix.export_runs(k) is None
        ask(other, ASK_AFTER)
        assert ix.debug_view_runs(other) == (True, 2) and ix.info()["last_variant"] == 4
        with_copy = ix.info()["side_bytes"]
        assert ix.set_option(OPT_VIEWS, 0) == 1                       # dropping the views drops it, with its bytes
        assert ix.debug_view_runs(other) == (False, 2) and ix.export_runs(other) is None
        assert ix.info()["side_bytes"] < min(before["side_bytes"], with_copy) and ix.info()["views_resident"] == 0
        assert ix.set_option(OPT_VIEWS, 1) == 0
        ask(k, 1)
