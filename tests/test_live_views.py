"""Placed six-row views without their dead groups (memo_view_build.hip: live_view_copy).  The placing pass flags every group of a placed
six-row view that holds no live row (kDeadGroup, bit 20 of its first dword; tests/test_live_rows.py); once a class's queries have lost
to loading those groups what a pass over the view costs, a query copies the view without them -- the unflagged groups unchanged, in
the order they come, with a bucket table of their own -- and the class switches over (MEMO_OPT_VIEW_LIVE, option 6)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

DEAD_GROUP = 1 << 20
OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_VIEW_PLACES, OPT_VIEW_LIVE = 3, 4, 5, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_is_documented_and_numbered():
    with open(os.path.join(ROOT, "include", "memo_amd.h")) as f:
        text = f.read()
    assert re.search(r"#define MEMO_OPT_VIEW_LIVE 6\b", text)
    assert "MEMO_OPT_VIEW_LIVE        1 (default)" in text


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture
def ab(memo):
    """the A/B library: six-row views forced, and the state of a class's view (memo_debug_view_live)"""
    from memo_amd import _lib
    _lib.use_ab(True)
    _lib.check(_lib.lib().memo_debug_six_views(1))
    yield _lib
    _lib.check(_lib.lib().memo_debug_six_views(-1))
    _lib.use_ab(False)


def _live(ab, ix, k):
    """(the six-row view of k's class is the copy without dead groups, copies made over the index's lifetime)"""
    n = C.c_uint64(0)
    is_copy = ab.check(ab.lib().memo_debug_view_live(ix._h, int(k), C.byref(n)))
    return is_copy, n.value


def _groups(view):
    """groups as uint32[g, 4], their bucket, the table in groups"""
    table = view[1] // 6
    ng = int(table[-1])
    g = view[0].reshape(-1, 4)[:ng]
    bucket = np.searchsorted(table[1:], np.arange(ng), side="right")
    return g, bucket, table


def _rows(seed, n=80_000, length=40_000, n_docs=20):
    """more than a row per position (what the dense rows answer), with ties, duplicates, an empty stretch, and buckets whose rows are all dead: rows at 32 b + 31 with overlaps 1 .. 25
    (order 7 and up), contained by a row of order 1 at 32 (b + 1) with overlap 0"""
    rng = np.random.default_rng(seed)
    s = rng.integers(1, length, n)
    s = s[(s < 12_000) | (s >= 15_000)]                           # nothing in [12000, 15000)
    s = s[((s >> 5) < 500) | ((s >> 5) > 504)]                    # (the buckets below hold only the rows put there)
    s = s[((s >> 5) < 700) | ((s >> 5) > 701)]
    ov = rng.integers(0, 40, len(s))
    o = rng.integers(1, n_docs, len(s))
    dup = rng.integers(0, len(s), len(s) // 10)
    s, ov, o = np.concatenate((s, s[dup])), np.concatenate((ov, ov[dup])), np.concatenate((o, o[dup]))
    for b in (500, 501, 503, 700):                                # (bucket 500's container sits at the start of bucket 501, and so on)
        m = 40
        s = np.concatenate((s, np.full(m, 32 * b + 31), [32 * (b + 1)]))
        ov = np.concatenate((ov, rng.integers(1, 26, m), [0]))
        o = np.concatenate((o, rng.integers(7, n_docs, m), [1]))
    idx = np.argsort(s, kind="stable")
    return s[idx].astype(np.int64), ov[idx].astype(np.int64), o[idx].astype(np.int64)


def _index(memo, s, ov, o):
    ix = memo.DeviceIndex.from_host(s, s + ov, o)
    ix.pack(keep_wide=False)
    ix.pack_dense(keep_packed=False)
    return ix


@pytest.mark.gpu
def test_copy_is_the_flagged_views_live_groups(memo, ab, oracle):
    s, ov, o = _rows(3)
    n, L = 20, int(s.max()) + 100
    for k in (9, 21, 31):
        with _index(memo, s, ov, o) as ix:
            ix.prepare(k, n)
            flagged = ix.export_view(k, 6)
            g0, b0, t0 = _groups(flagged)
            flag = (g0[:, 0] & DEAD_GROUP) != 0
            assert flag.any() and not flag.all(), k
            # buckets 500 / 501 / 503 / 700: every row is dead, every group flagged
            for b in (500, 503, 700):
                sel = b0 == b
                assert sel.any() and flag[sel].all(), (k, b)
            before = ix.info()
            assert _live(ab, ix, k) == (0, 0)
            # prepare and one whole-window query: the copy is not built
            ix.conservation(0, L, k, n)
            assert _live(ab, ix, k) == (0, 0), k
            assert ix.info()["last_rows_read"] == 6 * len(g0)
            # MEMO_OPT_BUILD_COST_PCT 0: the next query builds it
            ix.set_option(OPT_BUILD_COST_PCT, 0)
            got = ix.conservation(7, L - 3, k, n)
            assert _live(ab, ix, k) == (1, 1), k
            inf = ix.info()
            copy = ix.export_view(k, 6)
            g1, b1, t1 = _groups(copy)
            # the copy: the unflagged groups, byte for byte, bucket by bucket, in the same order; none flagged; the scan of the live groups
            assert np.array_equal(g1, g0[~flag]), k
            assert np.array_equal(b1, b0[~flag]), k
            assert not ((g1[:, 0] & DEAD_GROUP) != 0).any()
            live_per_bucket = np.bincount(b0[~flag], minlength=len(t0) - 1)
            assert np.array_equal(copy[1], 6 * np.concatenate(([0], np.cumsum(live_per_bucket)))), k
            assert np.array_equal(copy[1][-1:], [6 * int((~flag).sum())])
            assert (np.diff(copy[1]) == 0).sum() > (np.diff(flagged[1]) == 0).sum()     # buckets with no group left
            assert copy[2] == flagged[2] and copy[3] == flagged[3]                     # rows, cap: the class's
            # the ledger: no view built, none added, the tile table replaced by the copy's; the side bytes fall
            for key in ("view_builds", "view_placings", "views_resident", "tile_tables_resident"):
                assert inf[key] == before[key], (k, key, inf[key], before[key])
            assert inf["side_bytes"] < before["side_bytes"], k
            assert inf["last_view_placed"] == 1 and inf["last_variant"] == 3 and inf["last_view_rows_per_group"] == 6
            assert inf["last_rows_read"] == 6 * len(g1)
            want = oracle.conservation(*oracle.filter_rows(s, s + ov, o, 7, L - 3, k), 7, L - 3, k, n, literal=False)
            assert np.array_equal(got, want), k
            # later queries: the copy stays, nothing is built again
            ix.conservation(0, L, k, n)
            assert _live(ab, ix, k) == (1, 1) and ix.info()["view_builds"] == before["view_builds"]


@pytest.mark.gpu
def test_copy_equals_oracle_every_k_class(memo, ab, oracle):
    s, ov, o = _rows(8, n=250_000, length=120_000)
    n, L = 20, int(s.max()) + 100
    rng = np.random.default_rng(9)
    with _index(memo, s, ov, o) as ix:
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        classes = set()
        for k in range(2, 33):
            ix.prepare(k, n)
            for q in range(3):
                qs = int(rng.integers(1, 2_000)) * 4 + int(rng.integers(1, 4))     # off the 4-position raster
                qe = min(qs + int(rng.integers(20_000, 110_000)), L - int(rng.integers(1, 50)))
                if q == 2:
                    qs, qe = 11_001, 16_003                                         # across the empty stretch
                got = ix.conservation(qs, qe, k, n)
                inf = ix.info()
                if k <= 31:                          # (k = 32: six level arrays, which the six-row sweep does not take)
                    assert inf["last_variant"] == 3 and inf["last_view_placed"] == 1, (k, inf)
                want = oracle.conservation(*oracle.filter_rows(s, s + ov, o, qs, qe, k), qs, qe, k, n, literal=False)
                assert np.array_equal(got, want), (k, q, qs, qe, int(np.argmax(got != want)))
            is_copy, made = _live(ab, ix, k)
            if is_copy:
                classes.add(k // 2)          # (k - 1 = 2 c - 1 and 2 c: one class)
            assert made == len(classes), (k, made, classes)
        assert len(classes) >= 10, classes   # (the classes whose placed view flags a group at all)


@pytest.mark.gpu
def test_option_zero_keeps_the_flagged_view(memo, ab, oracle):
    s, ov, o = _rows(5)
    n, L, k = 20, int(s.max()) + 100, 31
    with _index(memo, s, ov, o) as ix:
        assert ix.set_option(OPT_VIEW_LIVE, 0) == 1
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        ix.prepare(k, n)
        flagged = ix.export_view(k, 6)
        for _ in range(4):
            got = ix.conservation(3, L - 1, k, n)
        assert _live(ab, ix, k) == (0, 0)
        assert np.array_equal(ix.export_view(k, 6)[0], flagged[0])
        assert ix.info()["last_rows_read"] == int(flagged[1][-1])
        want = oracle.conservation(*oracle.filter_rows(s, s + ov, o, 3, L - 1, k), 3, L - 1, k, n, literal=False)
        assert np.array_equal(got, want)
        assert ix.set_option(OPT_VIEW_LIVE, 1) == 0
        assert np.array_equal(ix.conservation(3, L - 1, k, n), want)
        assert _live(ab, ix, k) == (1, 1)
        with pytest.raises(Exception):
            ix.set_option(OPT_VIEW_LIVE, 2)


@pytest.mark.gpu
def test_config3_whole_window_on_the_copy(memo, oracle):
    """what bench.py times: config 3 at k = 31, the library's choices, the copy built by the queries (as the clock-ramp launches of
    bench.py build it) -- the whole 10^8-position result against the oracle, and equal to the flagged view's"""
    from memo_amd import _lib, synth
    n, L, k = 100, 100_000_000, 31
    ix, (r0, r1) = synth.device_index(0, L, k, n, L, pack="dense")

    def whole_window(into):
        d = C.c_void_p()
        _lib.check(_lib.lib().memo_dev_malloc(0, into.nbytes, C.byref(d)))
        try:
            ix.conservation_u8_dev(0, L, k, n, d.value)
            ix.check()
            _lib.check(_lib.lib().memo_dev_download(0, into.ctypes.data, d, into.nbytes, None))
        finally:
            _lib.lib().memo_dev_free(0, d)

    with ix:
        ix.prepare(k, n)
        flagged = np.empty(L, np.uint8)
        whole_window(flagged)
        inf0 = ix.info()
        assert inf0["last_variant"] == 3 and abs(inf0["last_rows_read"] / (r1 - r0) - 0.516) < 0.01, inf0
        lost = 1
        for _ in range(64):                        # the ledger: a few whole-window queries pay for the copy
            got = np.empty(L, np.uint8)
            whole_window(got)
            if ix.info()["last_rows_read"] < inf0["last_rows_read"]:
                break
            lost += 1
        inf = ix.info()
        assert 2 <= lost <= 20, lost
        assert inf["last_rows_read"] < 0.5 * inf0["last_rows_read"], inf         # (73 % of the groups were dead at k = 31)
        assert inf["last_view_placed"] == 1 and inf["view_builds"] == inf0["view_builds"]
        whole_window(got)                          # (a query on the copy it did not build)
        assert np.array_equal(got, flagged)
        bad, fnv = oracle.synth_window_compare(got, 0, L, k, n, L)
        assert bad == 0, f"{bad} chunks of the copy's whole-window result differ from the oracle"
