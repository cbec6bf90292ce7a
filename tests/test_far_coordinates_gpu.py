"""Every row format and sweep with its rows at pivot positions past 2^31 and 2^32.  Shifting every row and the window by D changes no
result byte (tests/test_far_coordinates_cpu.py holds the oracle to that), so every result here is compared with the oracle at the
shifted coordinates and with the bytes of the same index at the origin; which kernel answered (info.last_sweep and what goes with it)
must be what answered at the origin too, so that no fallback to another kernel hides a wrong one.

The shifts: 2^31 - 60 001 and 2^32 - 59 997 put the boundary inside the index and move the tile raster (tiles lie at multiples of
their width in pivot coordinates) and the 4-, 32- and 1024-position rasters; 2^32 leaves every stored field as it is at the origin;
2^33 + 12 345 is odd and past 2^33.  Bucket tables start at bucket 0 (8 bytes per 32 positions: 1 GiB at 2^32), which is why no test here
goes past 2^34 and why the 2^33 cases run fewer k."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_VIEW_LIVE, OPT_WIDE_TILES = 3, 4, 6, 7
DEAD_GROUP = 1 << 20
B31, B32 = 60_001, 59_997                 # where 2^31 / 2^32 lie inside an index shifted by the two straddling shifts
FAR = 2 ** 33 + 12_345
SHIFTS = (0, 2 ** 31 - B31, 2 ** 32 - B32, 2 ** 32, FAR)
KS = (2, 3, 17, 31, 32, 33, 64, 65, 101, 256, 300)
KS_FAR = (3, 31, 101)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture
def ab(memo):
    """the A/B library (kernel shapes, six-row views forced or not, the state of a class's view)"""
    from memo_amd import _lib
    _lib.use_ab(True)
    yield _lib
    _lib.check(_lib.lib().memo_debug_six_views(-1))
    _lib.check(_lib.lib().memo_debug_fail_side_allocations(0))
    _lib.check(_lib.lib().memo_debug_one_shot_way(0))
    _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# row sets
# ---------------------------------------------------------------------------------------
def _r1(seed, n=250_000, length=120_000, n_docs=20):
    """tests/test_live_views.py's rows: more than a row per position, ties, duplicates, an empty stretch, buckets whose rows are all dead"""
    from tests.test_live_views import _rows
    return _rows(seed, n=n, length=length, n_docs=n_docs)


_R2 = {}


def _r2(n_docs):
    """tests/test_gpu_parity.py::test_packed_rows_equal_wide_rows's rows (packed formats 4 / 12 / 6 at 70 / 500 / 6000 genomes: every
    seventh overlap saturates the 8-bit length) and 200 rows with end < start, on both sides of position 60 000"""
    if n_docs not in _R2:
        rng = np.random.default_rng(n_docs)
        s = np.sort(rng.integers(1, 150_000, 400_000)).astype(np.int64)
        e = s + rng.integers(0, 300, 400_000)
        o = rng.integers(1, n_docs, 400_000).astype(np.int64)
        e[::7] = s[::7] + rng.integers(250, 5000, len(s[::7]))
        pick = rng.choice(len(s), 200, replace=False)
        e[pick] = s[pick] - rng.integers(1, 400, 200)
        assert ((s[pick] < 59_000).sum() > 20) and ((s[pick] > 61_000).sum() > 20)
        _R2[n_docs] = (s, e, o)
    return _R2[n_docs]


def _windows(L):
    """relative to the shift: the whole index, (1, L - 1), six positions across either boundary, a window that ends at it, one that
    starts one past it, one off every raster"""
    w = [(0, L), (1, L - 1), (4 * 9973 + 3, 4 * 9973 + 3 + 77_777)]
    for b in (B31, B32):
        w += [(b - 3, b + 3), (b - 40_001, b), (b + 1, b + 50_002)]
    return w


def _want_cons(oracle, s, e, o, qs, qe, k, n):
    return oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n, literal=False)


def _want_memb(oracle, s, e, o, qs, qe, k, n):
    return oracle.membership(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n, literal=False)


# ---------------------------------------------------------------------------------------
# 1. resident formats: int64 columns, 4- / 6-byte rows, dense rows
# ---------------------------------------------------------------------------------------
# (tile_w, waves, membership algorithm, scatter): the library's choice, a narrow and a wide tile, scatters 1 / 2 / 3, algorithms 2 / 3 / 4
_TUNINGS = [(0, 0, 0, 0), (256, 1, 2, 1), (256, 4, 3, 2), (2048, 4, 4, 3), (1024, 1, 4, 2), (512, 4, 3, 3), (2048, 4, 2, 1)]
_RESIDENT = {}


def _resident(memo, oracle, n_docs, D, ks):
    """{(k, window, source, what): (result, last_sweep)} of one index of R2 at shift D, every result checked against the oracle at the
    shifted coordinates"""
    s, e, o = _r2(n_docs)
    L = 150_100
    out = {}
    with memo.DeviceIndex.from_host(s + D, e + D, o) as ix:
        ix.pack(keep_wide=True)
        inf = ix.info()
        assert inf["packed_format"] == (4 if n_docs <= 256 else 12 if n_docs <= 4096 else 6) and inf["has_wide"] == 1
        assert inf["long_rows"] == 200
        assert inf["min_start"] == int(s[0]) + D and inf["max_start"] == int(s[-1]) + D
        try:
            for k in ks:
                for iw, (a, b) in enumerate(_windows(L)):
                    qs, qe = a + D, b + D
                    tile_w, waves, algo, scatter = _TUNINGS[(KS.index(k) + iw) % len(_TUNINGS)]
                    want = _want_cons(oracle, s + D, e + D, o, qs, qe, k, n_docs)
                    # the library's choice, the 4- / 6-byte rows, the int64 columns
                    for source in (0, 3, 1) if k <= 256 else (0,):
                        if source == 1 and k not in (3, 31):
                            continue
                        ix.debug_set_tuning(tile_w, waves, algo, source, scatter)
                        got = ix.conservation(qs, qe, k, n_docs)
                        assert np.array_equal(got, want), (n_docs, D, k, a, b, source, int(np.argmax(got != want)))
                        out[k, iw, source, "u16"] = (got, ix.info()["last_sweep"])
                        if n_docs <= 255:
                            got = ix.conservation(qs, qe, k, n_docs, dtype=np.uint8)
                            assert np.array_equal(got, want.astype(np.uint8)), (n_docs, D, k, a, b, source)
                            out[k, iw, source, "u8"] = (got, ix.info()["last_sweep"])
                    if iw % 2 == 0 or b - a < 10:
                        qe = min(qe, qs + 1500)
                        wantb = _want_memb(oracle, s + D, e + D, o, qs, qe, k, n_docs)
                        ix.debug_set_tuning(tile_w, waves, algo, 0, scatter)
                        got = ix.membership(qs, qe, k, n_docs)
                        assert np.array_equal(got, wantb), (n_docs, D, k, a, b)
                        out[k, iw, 0, "bits"] = (got, ix.info()["last_sweep"])
        finally:
            ix.debug_set_tuning()
        ix.check()
    if n_docs > 511:
        return out
    # the dense rows (3.2 B per row) alone: R2 keeps fewer dense rows than it spans positions (the rows that cannot write at k <= 64
    # are left out), so they answer only where the 4-byte rows are gone; R1, denser, is swept in the tests of the views below
    with memo.DeviceIndex.from_host(s + D, e + D, o) as ix:
        ix.pack(keep_wide=False)
        ix.pack_dense(keep_packed=False)
        inf = ix.info()
        assert inf["dense_rows"] == 1 and 0 < inf["dense_row_count"] < 150_000
        try:
            for k in [k for k in ks if k <= 64]:
                for iw, (a, b) in enumerate(_windows(L)):
                    qs, qe = a + D, b + D
                    tile_w, waves = ((0, 0), (1024, 4), (512, 1), (1024, 8))[(KS.index(k) + iw) % 4]
                    ix.debug_set_tuning(tile_w, waves)
                    want = _want_cons(oracle, s + D, e + D, o, qs, qe, k, n_docs)
                    for dt in (np.uint16, np.uint8) if n_docs <= 255 else (np.uint16,):
                        got = ix.conservation(qs, qe, k, n_docs, dtype=dt)
                        assert np.array_equal(got, want.astype(dt)), (n_docs, D, k, a, b, dt, int(np.argmax(got != want)))
                        assert ix.info()["last_sweep"] == 5
                        out[k, iw, "dense", dt.__name__] = (got, 5)
                    if n_docs <= 255 and (iw % 2 == 0 or b - a < 10):      # (bit planes on the dense rows: up to 255 genomes)
                        qe = min(qe, qs + 1500)
                        got = ix.membership(qs, qe, k, n_docs)
                        assert np.array_equal(got, _want_memb(oracle, s + D, e + D, o, qs, qe, k, n_docs)), (n_docs, D, k, a, b)
                        assert ix.info()["last_sweep"] == 6
                        out[k, iw, "dense", "bits"] = (got, 6)
        finally:
            ix.debug_set_tuning()
        ix.check()
    return out


@pytest.mark.parametrize("D", SHIFTS, ids=lambda d: "D%d" % d)
@pytest.mark.parametrize("n_docs", [70, 500, 6000])
def test_resident_formats(n_docs, D, memo, oracle, ab):
    ks = KS_FAR if D == FAR else KS
    if (n_docs, 0) not in _RESIDENT:
        _RESIDENT[n_docs, 0] = _resident(memo, oracle, n_docs, 0, KS)
    twin = _RESIDENT[n_docs, 0]
    got = twin if D == 0 else _resident(memo, oracle, n_docs, D, ks)
    per_k = 9 * (2 if n_docs <= 255 else 1)                       # windows x result types, per row source
    dense = 0 if n_docs > 511 else per_k + (6 if n_docs <= 255 else 0)
    assert len(got) == sum(per_k * (3 if k in (3, 31) else 2 if k <= 256 else 1) + 6 + (dense if k <= 64 else 0) for k in ks)
    sweeps = set()
    for key, (result, sweep) in got.items():
        assert np.array_equal(result, twin[key][0]), (n_docs, D, key)
        assert sweep == twin[key][1], (n_docs, D, key, sweep, twin[key][1])
        sweeps.add(sweep)
    # more than one family of kernels answered, the dense rows' (5) among them where dense rows are resident
    assert len(sweeps) >= 2 and (5 in sweeps) == (n_docs <= 511), sweeps


# ---------------------------------------------------------------------------------------
# 2. stored bytes at D = 2^32: every stored field is a residue the shift leaves alone
# ---------------------------------------------------------------------------------------
_TABLES = {}


def _table(n, slot):
    """a host buffer for a bucket table (1 GiB at 2^32, 2 GiB past 2^33), reused within a test: its pages are faulted in once"""
    if (slot, n) not in _TABLES:
        _TABLES[slot, n] = np.empty(n, np.int64)
    return _TABLES[slot, n]


def _export_packed(ix, slot=0):
    from memo_amd import _lib
    inf = ix.info()
    pk = np.empty(inf["rows"], np.uint32)
    pa = np.empty(inf["rows"] if inf["packed_format"] == 6 else 0, np.uint16)
    boff = _table(inf["buckets"], slot)
    longs = np.empty(3 * inf["long_rows"], np.int64)
    _lib.check(_lib.lib().memo_index_export_packed(ix._h, pk.ctypes.data, pa.ctypes.data if pa.size else None, boff.ctypes.data,
                                                   longs.ctypes.data if longs.size else None))
    return pk, pa, boff, _triples(longs)


def _export_dense(ix, slot=1):
    from memo_amd import _lib
    inf = ix.info()
    g = np.empty(4 * ((inf["dense_row_count"] + 4) // 5), np.uint32)
    boff = _table(inf["buckets"], slot)
    longs = np.empty(3 * inf["long_rows"], np.int64)
    _lib.check(_lib.lib().memo_index_export_dense(ix._h, g.ctypes.data, boff.ctypes.data, longs.ctypes.data if longs.size else None))
    return g, boff, _triples(longs), inf["dense_row_count"]


def _triples(longs):
    """the rows with end < start, (start, end, annot) sorted (the device collects them in no particular order)"""
    t = longs.reshape(3, -1).T
    return t[np.lexsort(t.T[::-1])]


def _table_is_shifted(boff, boff0, D, first_start):
    """a bucket table anchored at position 0: the origin's entries D / 32 buckets further on, zeros before the first row's bucket"""
    nb0, sh = len(boff0), D >> 5
    assert D % 32 == 0 and len(boff) == sh + nb0, (len(boff), sh, nb0)
    assert np.array_equal(boff[sh + 1:], boff0[1:])
    assert not boff[:(first_start + D) >> 5].any() and not boff[:sh + 1].any()
    return True


@pytest.mark.parametrize("n_docs", [70, 500, 6000])
def test_stored_rows_at_2_pow_32(n_docs, memo, ab):
    s, e, o = _r2(n_docs)
    D = 2 ** 32
    exports = []
    for d in (0, D):
        with memo.DeviceIndex.from_host(s + d, e + d, o) as ix:
            ix.pack(keep_wide=False)
            packed = _export_packed(ix)
            dense = None
            if n_docs <= 511:
                ix.pack_dense(keep_packed=False)
                dense = _export_dense(ix)
            exports.append((packed, dense))
    _TABLES.clear()
    (p0, d0), (p1, d1) = exports
    assert np.array_equal(p1[0], p0[0]) and np.array_equal(p1[1], p0[1]) and len(p0[0]) == len(s)
    assert _table_is_shifted(p1[2], p0[2], D, int(s[0]))
    assert np.array_equal(p1[3], p0[3] + np.array([D, D, 0])) and len(p0[3]) == 200
    if n_docs <= 511:
        assert d1[3] == d0[3] and np.array_equal(d1[0], d0[0])
        assert _table_is_shifted(d1[1], d0[1], D, int(s[0]))
        assert np.array_equal(d1[2], d0[2] + np.array([D, D, 0]))


def test_stored_views_at_2_pow_32(memo, ab):
    """the five-row and the (placed, flagged) six-row view of a k class: groups with their flags, rows and cap equal, table shifted"""
    s, ov, o = _r1(3)
    D = 2 ** 32
    views = {}
    for d in (0, D):
        for k in (9, 21, 31):
            for rpg in (5, 6):
                ab.check(ab.lib().memo_debug_six_views(1 if rpg == 6 else 0))
                with memo.DeviceIndex.from_host(s + d, s + ov + d, o) as ix:
                    ix.pack(keep_wide=False)
                    ix.pack_dense(keep_packed=False)
                    ix.prepare(k, 20)
                    views[d, k, rpg] = ix.export_view(k, rpg)
                    assert views[d, k, rpg] is not None, (d, k, rpg)
    checked = 0
    for k in (9, 21, 31):
        for rpg in (5, 6):
            g0, t0, rows0, cap0 = views[0, k, rpg]
            g1, t1, rows1, cap1 = views[D, k, rpg]
            assert (rows1, cap1) == (rows0, cap0) and rows0 > 0, (k, rpg)
            assert np.array_equal(g1, g0), (k, rpg)
            assert _table_is_shifted(t1, t0, D, int(s[0])), (k, rpg)
            if rpg == 6:
                flag = (g0.reshape(-1, 4)[:int(t0[-1]) // 6, 0] & DEAD_GROUP) != 0
                assert flag.any() and not flag.all(), k
            checked += 1
    assert checked == 6


# ---------------------------------------------------------------------------------------
# 3. k-class views, the live copy, wide tiles
# ---------------------------------------------------------------------------------------
def _live(ab, ix, k):
    n = C.c_uint64(0)
    is_copy = ab.check(ab.lib().memo_debug_view_live(ix._h, int(k), C.byref(n)))
    return is_copy, n.value


_WHICH = ("last_sweep", "last_variant", "last_view_placed", "last_view_rows_per_group", "last_tile_width")
_VIEWS = {}
_VIEW_KS = (2, 9, 17, 21, 31, 32)


def _views(memo, ab, oracle, D):
    """{(k, step, window): (result, which kernel and view answered)} on R1 at shift D, one fresh index per k (a view is charged its
    bucket table, which starts at bucket 0: far from the origin a second class would evict the first)"""
    s, ov, o = _r1(8)
    n, L = 20, int(s.max()) + 100
    windows = _windows(L) + [(11_001, 16_003)]                       # (across the empty stretch)
    out, ledger = {}, None
    for k in _VIEW_KS:
        with memo.DeviceIndex.from_host(s + D, s + ov + D, o) as ix:
            ix.pack(keep_wide=False)
            ix.pack_dense(keep_packed=False)
            want = {w: _want_cons(oracle, s + D, s + ov + D, o, w[0] + D, w[1] + D, k, n) for w in windows}

            def run(step, ws=windows):
                for w in ws:
                    dt = np.uint8 if (w[0] + k) % 2 else np.uint16
                    got = ix.conservation(w[0] + D, w[1] + D, k, n, dtype=dt)
                    inf = ix.info()
                    assert np.array_equal(got, want[w].astype(dt)), (D, k, step, w, int(np.argmax(got != want[w])))
                    out[k, step, w] = (got, tuple(inf[key] for key in _WHICH))
                return inf
            ab.check(ab.lib().memo_debug_six_views(1))
            ix.prepare(k, n)
            inf = run("flagged", windows[:1])                            # prepare and one query: the placed, flagged six-row view
            assert _live(ab, ix, k) == (0, 0)
            if k <= 31:
                assert (inf["last_variant"], inf["last_view_placed"], inf["last_view_rows_per_group"]) == (3, 1, 6), (D, k, inf)
            ix.set_option(OPT_BUILD_COST_PCT, 0)
            run("copying", windows[1:2])                                 # the query that builds the copy
            out[k, "live"] = _live(ab, ix, k)
            if k in (9, 17, 21, 31):
                assert out[k, "live"] == (1, 1), (D, k)
            run("wide")
            assert ix.set_option(OPT_WIDE_TILES, 0) == 1
            run("doubling")
            assert ix.set_option(OPT_WIDE_TILES, 1) == 0
            assert ix.set_option(OPT_VIEW_LIVE, 0) == 1                  # the flagged view again
            run("flagged again")
            ab.check(ab.lib().memo_debug_six_views(0))
            ix.set_option(OPT_VIEW_ROWS, 5)
            inf = run("five")
            if k in (9, 17, 21, 31):
                assert inf["last_view_rows_per_group"] == 5 and inf["last_variant"] == 2, (D, k, inf)
            ix.debug_no_views(True)
            run("no views")
            ix.check()
            if k == 31:
                ledger = ix.info()
    print("far from the origin: D = %d: side_bytes %d, device_bytes %d, view_builds %d (k = 31, after its queries)"
          % (D, ledger["side_bytes"], ledger["device_bytes"], ledger["view_builds"]))
    return out


@pytest.mark.parametrize("D", SHIFTS, ids=lambda d: "D%d" % d)
def test_views_live_copy_and_wide_tiles(D, memo, ab, oracle):
    if 0 not in _VIEWS:
        _VIEWS[0] = _views(memo, ab, oracle, 0)
    twin = _VIEWS[0]
    got = twin if D == 0 else _views(memo, ab, oracle, D)
    assert len(got) == len(_VIEW_KS) * (1 + 1 + 5 * 10 + 1)
    for key, value in got.items():
        if key[1] == "live":
            assert value == twin[key], (D, key, value, twin[key])
        else:
            assert np.array_equal(value[0], twin[key][0]), (D, key)
            assert value[1] == twin[key][1], (D, key, value[1], twin[key][1])


def _widths(k, cells):
    """positions per tile of the table-driven sweep (tests/test_wide_tiles.py)"""
    km1 = k - 1
    hl, hr = (km1 + 3) & ~3, (km1 + 31 + 3) & ~3
    return (cells - hl - hr) // 32 * 32


@pytest.mark.parametrize("a", [2 ** 31 - 150_000, 2 ** 32 - 150_000, 2 ** 32 + 2 ** 31 + 777], ids=lambda a: "a%d" % a)
def test_config3_windows_far(a, memo, oracle):
    """config 3's rows generated at far coordinates (the generator is index-addressable: rows 1.07e10 .. 3.2e10), swept on the wide
    and the doubling tiles.  Tiles lie at multiples of their width in pivot coordinates, so the windows of
    tests/test_wide_tiles.py::test_config3_windows are placed from the first tile boundary t0 at or after a.  The boundary B = a + 150 000
    is 2^31 / 2^32 for the first two a.  A tile's slice passes the 1024-cell wrap at (tile start + 1024); that cannot be B itself (no
    tile width here divides 2^31 - 1024 or 2^32 - 1024: they hold the odd factors 49, 25, 29 and 15), so the tile whose wrap point
    lies nearest below B is taken, and its wrap point and B are each crossed by a six-position window."""
    from memo_amd import synth
    n, L, pivot = 100, 300_000, 2 ** 33
    num, den = synth.rows_per_position(n)
    B = a + 150_000
    wide = 0
    for k in (17, 25, 31):
        ix, (r0, r1) = synth.device_index(a, a + L, k, n, pivot, pack="dense")
        assert r0 > 2 ** 33 and r1 - r0 > 5 * L - 10
        s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, n)
        assert a < s[0] <= a + 1 and s[-1] == a + L + k - 1
        tw = _widths(k, 1664)
        t0 = -(-a // tw) * tw - a                                   # (relative to a, like every window below)
        tb = (B - 1024) // tw * tw - a
        windows = [(0, L), (1, L - 1), (t0 + 3 * tw + 5, t0 + L - 7 * tw - 3 - tw), (37, tw + 1030), (t0 + 50 * tw - 1, t0 + 50 * tw + 2),
                   (t0 + 1024 + 3, t0 + 3 * tw + 1023), (t0 + 9 * tw + 1021, t0 + 9 * tw + 1027), (L - tw - 2, L),
                   (B - a - 3, B - a + 3), (tb + 1021, tb + 1027)]
        with ix:
            ix.set_option(OPT_BUILD_COST_PCT, 0)
            ix.prepare(k, n)
            ix.conservation(a, a + L, k, n, np.uint8)                # (the class's view, its copy without dead groups)
            for ra, rb in windows:
                qs, qe = a + ra, a + rb
                want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n, literal=False)
                for dt in (np.uint8, np.uint16):
                    got = ix.conservation(qs, qe, k, n, dt)
                    inf = ix.info()
                    assert ix.set_option(OPT_WIDE_TILES, 0) == 1
                    ref = ix.conservation(qs, qe, k, n, dt)
                    inf0 = ix.info()
                    assert ix.set_option(OPT_WIDE_TILES, 1) == 0
                    assert got.dtype == dt and np.array_equal(got, want), (a, k, ra, rb, dt, int(np.argmax(got != want)))
                    assert np.array_equal(ref, got), (a, k, ra, rb, dt)
                    assert inf["last_sweep"] == 5 and inf0["last_sweep"] == 5, (k, inf)
                    assert inf["last_variant"] == 3 and inf["last_view_rows_per_group"] == 6, (k, inf)
                    assert inf["last_tile_width"] == tw, (k, inf["last_tile_width"])
                    assert inf0["last_variant"] == 3 and inf0["last_tile_width"] == _widths(k, 1024), (k, inf0)
                    wide += 1
            ix.check()
    assert wide == 3 * 10 * 2


def test_kernel_without_a_tile_table_far(memo, ab, oracle):
    """no room on the device for views and tile tables (memo_debug_fail_side_allocations), rows on both sides of 2^32: the dense-row
    kernel that works its tiles out itself (last_variant 0), the same bytes"""
    s, ov, o = _r1(8)
    n, L, D = 20, int(s.max()) + 100, 2 ** 32 - B32
    cases = 0
    ab.check(ab.lib().memo_debug_fail_side_allocations(1))
    try:
        results = {}
        for d in (0, D):
            with memo.DeviceIndex.from_host(s + d, s + ov + d, o) as ix:
                ix.pack(keep_wide=False)
                ix.pack_dense(keep_packed=False)
                ix.set_option(OPT_BUILD_COST_PCT, 0)
                for k in (9, 31, 64):
                    for w in _windows(L):
                        got = ix.conservation(w[0] + d, w[1] + d, k, n)
                        inf = ix.info()
                        assert (inf["last_sweep"], inf["last_variant"]) == (5, 0) and inf["side_bytes"] == 0, (d, k, inf)
                        assert inf["views_resident"] == 0 and inf["tile_tables_resident"] == 0
                        results[d, k, w] = got
                        if d:
                            want = _want_cons(oracle, s + d, s + ov + d, o, w[0] + d, w[1] + d, k, n)
                            assert np.array_equal(got, want), (k, w, int(np.argmax(got != want)))
                            assert np.array_equal(got, results[0, k, w]), (k, w)
                            cases += 1
    finally:
        ab.check(ab.lib().memo_debug_fail_side_allocations(0))
    assert cases == 3 * 9


# ---------------------------------------------------------------------------------------
# 4. the host packers (memo_builder_*) and the one-shot seam
# ---------------------------------------------------------------------------------------
def _cuts(s, D, boundary, pieces, rng):
    """row numbers that cut the rows into `pieces` pieces, two of the cuts five positions either side of the boundary"""
    fixed = [int(np.searchsorted(s, boundary - 5)), int(np.searchsorted(s, boundary + 5))][:max(pieces - 1, 0)]
    more = sorted(int(x) for x in rng.integers(0, len(s), max(pieces - 1 - len(fixed), 0)))
    return [0] + sorted(fixed + more) + [len(s)]


@pytest.mark.parametrize("D", [2 ** 31 - B31, 2 ** 32 - B32, FAR], ids=lambda d: "D%d" % d)
def test_host_packers_equal_device_packing(D, memo, ab):
    """rows narrowed on the host (memo_hostcore.cpp: its vector paths narrow `start` with permutes and mask compares) at far
    coordinates -- DeviceIndex.from_host_packed, and builders fed 1, 7 and 9 pieces cut either side of the boundary, columns and
    the [M, 3] form: the words, groups, bucket tables and long rows that packing on the device gives, at every shift.  (The builders
    refuse annots of more than 12 bits, so the 4-byte words with 8-bit and with 12-bit annots are what there is to compare.)"""
    rng = np.random.default_rng(5)
    boundary = {2 ** 31 - B31: B31, 2 ** 32 - B32: B32}.get(D, 70_000)
    compared = 0
    try:
        for n_docs in (70, 500):                                     # 4-byte words with 8-bit and with 12-bit annots
            ways = ((1, False), (7, False), (9, False), (7, True)) if n_docs == 70 else ((7, False),)
            s, e, o = _r2(n_docs)
            s, e = s + D, e + D
            with memo.DeviceIndex.from_host(s, e, o) as ref:
                ref.pack(keep_wide=True)
                want = _export_packed(ref, 0)
                row_order = ref.info()["row_order"]
            assert len(want[3]) == 200

            def same_words(ix, what):
                inf = ix.info()
                assert inf["rows"] == len(s) and inf["min_start"] == int(s[0]) and inf["max_start"] == int(s[-1])
                assert inf["packed_format"] == (4 if n_docs == 70 else 12) and inf["long_rows"] == 200
                ix.pack(keep_wide=False)                              # (the host packer's rows into the query order)
                assert ix.info()["row_order"] == row_order
                got = _export_packed(ix, 1)
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), (D, n_docs, what)
                return 1
            with memo.DeviceIndex.from_host_packed(s, e, o, dense=False) as ix:
                compared += same_words(ix, "from_host_packed")
            for pieces, rows3 in ways:
                cuts = _cuts(s, D, boundary + D, pieces, rng)
                assert len(cuts) == pieces + 1
                with memo.IndexBuilder(len(s) + 1000) as b:
                    for a, z in zip(cuts[:-1], cuts[1:]):
                        if rows3:
                            b.push_rows(np.stack([s[a:z], e[a:z], o[a:z]], axis=1).astype(np.uint64))
                        else:
                            b.push(s[a:z], e[a:z], o[a:z])
                    with b.finish() as ix:
                        compared += same_words(ix, (pieces, rows3))
        s, e, o = _r2(70)
        s, e = s + D, e + D
        with memo.DeviceIndex.from_host(s, e, o) as ref:
            ref.debug_row_order(1)                                    # (groups in start order, as the host builder emits them)
            ref.pack(keep_wide=False)
            ref.pack_dense(keep_packed=False)
            want = _export_dense(ref, 0)

        def same_groups(ix, what):
            inf = ix.info()
            assert inf["rows"] == len(s) and inf["dense_rows"] == 1
            got = _export_dense(ix, 1)
            assert got[3] == want[3]
            cut = 4 if got[3] % 5 else 0                              # rows behind the last one in its group: never read by number
            assert np.array_equal(got[0][:len(got[0]) - cut], want[0][:len(want[0]) - cut]), (D, what)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (D, what)
            return 1
        with memo.DeviceIndex.from_host_packed(s, e, o, dense=True) as ix:
            compared += same_groups(ix, "from_host_packed")
        for pieces, rows3 in ((1, False), (7, False), (9, False), (9, True)):
            cuts = _cuts(s, D, boundary + D, pieces, rng)
            with memo.IndexBuilder(len(s) + 77, dense=True) as b:
                for a, z in zip(cuts[:-1], cuts[1:]):
                    if rows3:
                        b.push_rows(np.stack([s[a:z], e[a:z], o[a:z]], axis=1))
                    else:
                        b.push(s[a:z], e[a:z], o[a:z])
                with b.finish() as ix:
                    compared += same_groups(ix, (pieces, rows3))
    finally:
        _TABLES.clear()
    assert compared == (1 + 4) + (1 + 1) + (1 + 4)


def test_one_shot_seam_far(memo, ab, oracle):
    """memo_conservation / memo_membership and their [M, 3] forms on host rows at far coordinates: the library's way in (dense rows,
    4-byte words, int64 columns by k) and each way forced; the same kernel family as at the origin.  Every call builds a bucket table
    from bucket 0: a dozen calls far from the origin, no more."""
    s, e, o = _r2(70)
    n, L = 70, 150_100
    rows3 = np.stack([s, e, o], axis=1)
    D1, D2, D3 = 2 ** 32 - B32, 2 ** 31 - B31, FAR
    calls = [(D1, "conservation", 31, 0, 0, L), (D1, "conservation", 101, 0, 1, L - 1), (D1, "conservation", 300, 0, B32 - 40_001, B32),
             (D1, "membership", 31, 0, B32 - 3, B32 + 1500), (D1, "conservation_rows", 31, 0, B32 + 1, B32 + 50_002),
             (D1, "membership_rows", 101, 0, B32 - 700, B32 + 700), (D1, "conservation", 31, 1, 5, L - 7),
             (D1, "conservation", 31, 2, 5, L - 7), (D2, "conservation", 31, 0, B31 - 3, B31 + 3), (D2, "membership", 101, 0, B31 - 900, B31 + 900),
             (D3, "conservation", 31, 0, 0, L), (D3, "conservation_rows", 101, 0, 3, L - 5)]
    families = set()
    for D, form, k, way, a, b in calls:
        memb = form.startswith("membership")
        want = (_want_memb if memb else _want_cons)(oracle, s + D, e + D, o, a + D, b + D, k, n)
        results = []
        for d in (0, D):
            ab.check(ab.lib().memo_debug_one_shot_way(way))
            try:
                if form.endswith("_rows"):
                    got = getattr(memo, form)((rows3 + np.array([d, d, 0])).astype(np.uint64), a + d, b + d, k, n)
                else:
                    got = getattr(memo, form)(s + d, e + d, o, a + d, b + d, k, n)
            finally:
                ab.check(ab.lib().memo_debug_one_shot_way(0))
            results.append((got, ab.lib().memo_debug_last_one_shot_sweep()))
        (got0, family0), (got, family) = results
        assert np.array_equal(got, want), (D, form, k, way, a, b)
        assert np.array_equal(got0, want), (form, k, way, a, b)
        assert family == family0, (D, form, k, way, family, family0)
        families.add((memb, family))
    assert len(calls) == 12
    assert (False, 5) in families                                     # the dense rows' kernel, the benchmarked one


# ---------------------------------------------------------------------------------------
# 5. the multi-device forms, on one GPU named several times
# ---------------------------------------------------------------------------------------
def test_multi_device_forms_far(memo, oracle):
    """memo_split_window's cuts fall near 2^32 (the window is cut in 2, 3 and 5 parts; rows with end < start on both sides, which the
    host form must not split and the resident form filters by the whole window)"""
    from memo_amd import index, _lib
    s, e, o = _r2(70)
    n, L, D = 70, 150_100, 2 ** 32 - B32
    s, e = s + D, e + D
    checked = 0
    queries = ((31, 0, L), (101, B32 - 60_003, B32 + 60_001), (2, B32 - 7, B32 + 6), (300, 5, 2 * B32 - 3))
    want = {q: _want_cons(oracle, s, e, o, q[1] + D, q[2] + D, q[0], n) for q in queries}
    wantb = {q: _want_memb(oracle, s, e, o, q[1] + D, min(q[2], q[1] + 20_000) + D, q[0], n) for q in queries}
    for devices in ([0, 0], [0, 0, 0, 0, 0]):
        for q in queries[:3] if len(devices) == 2 else queries[1:]:
            k, a, b = q
            assert np.array_equal(index.conservation_multi(s, e, o, a + D, b + D, k, n, devices), want[q]), (devices, q)
            assert np.array_equal(index.membership_multi(s, e, o, a + D, min(b, a + 20_000) + D, k, n, devices), wantb[q]), (devices, q)
            checked += 2
    shards = [memo.DeviceIndex.from_host_packed(s, e, o) for _ in range(3)]
    try:
        assert shards[0].info()["long_rows"] == 200
        for root_weight in (1.0, 0.0):
            for q in queries[:2]:                                     # (k <= 256: the packed rows)
                k, a, b = q
                for membership, w, qe in ((False, want[q], b), (True, wantb[q], min(b, a + 20_000))):
                    got = np.empty_like(w)
                    d = C.c_void_p()
                    _lib.check(_lib.lib().memo_dev_malloc(0, max(got.nbytes, 16), C.byref(d)))
                    try:
                        index.query_multi_dev(shards, a + D, qe + D, k, n, d.value, 0, None, root_weight, membership)
                        for ix in shards:
                            ix.check()
                        _lib.check(_lib.lib().memo_dev_download(0, got.ctypes.data, d, got.nbytes, None))
                    finally:
                        _lib.lib().memo_dev_free(0, d)
                    assert np.array_equal(got, w), (root_weight, q, membership)
                    checked += 1
    finally:
        for ix in shards:
            ix.close()
    assert checked == 2 * 3 * 2 + 2 * 2 * 2


# ---------------------------------------------------------------------------------------
# 6. `memo query` and the sidecar cache
# ---------------------------------------------------------------------------------------
def test_cli_and_cache_far(memo, oracle, tmp_path, monkeypatch):
    """a Parquet index of several row groups with its rows around 2^32: `memo query` without a cache, with the cache built, and on a
    hit (memo_amd/_fastquery.py imports a slice of buckets: the one path with bucket_base != 0) -- the reference's text, byte for byte"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import cache, memo_query as mq
    s, e, o = _r2(70)
    n, D, k = 70, 2 ** 32 - B32, 31
    s, e = s + D, e + D
    path = str(tmp_path / "far.parquet")
    pq.write_table(pa.table({"f0": pa.array(["chrZ"] * len(s), pa.utf8()), "f1": s, "f2": e, "f3": o}), path, row_group_size=50_000,
                   compression="ZSTD")
    exe = os.path.join(ROOT, "bin", "memo")
    qs, qe = D + 1000, D + 100_000

    def query(mode, extra=()):
        out = tmp_path / "out.txt"
        r = subprocess.run([sys.executable, exe, "query", "-b", path, "-k", str(k), "-n", str(n), "-r", f"chrZ:{qs}-{qe}", "-o", str(out),
                            *extra], capture_output=True, env=dict(os.environ, MEMO_CACHE=mode, MEMO_TIMING="1"))
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        return out.read_bytes(), r.stderr.decode()
    want = oracle.emit_conservation(_want_cons(oracle, s, e, o, qs, qe, k, n))
    wantm = oracle.emit_membership(_want_memb(oracle, s, e, o, qs, qs + 3000, k, n), n)
    text, err = query("0")
    assert text == want and "sidecar cache" not in err and not os.path.exists(cache.cache_path(path, "chrZ"))
    text, err = query("sync")                                         # miss: answered from the Parquet file, the cache written
    assert text == want and "sidecar cache" not in err and os.path.exists(cache.cache_path(path, "chrZ"))
    text, err = query("1")                                            # hit
    assert text == want and "from the sidecar cache, ctypes-only path" in err, err
    qe_m = qs + 3000
    for mode in ("0", "1"):
        out = tmp_path / "out_m.txt"
        r = subprocess.run([sys.executable, exe, "query", "-b", path, "-k", str(k), "-n", str(n), "-r", f"chrZ:{qs}-{qe_m}", "-o", str(out),
                            "-m"], capture_output=True, env=dict(os.environ, MEMO_CACHE=mode, MEMO_TIMING="1"))
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        assert out.read_bytes() == wantm, mode
        assert ("from the sidecar cache" in r.stderr.decode()) == (mode == "1")
    rows = int(((s > qs) & (s < qe + k)).sum())
    short = int(((s > qs) & (s < qe + k) & (e >= s) & (e - s < 63)).sum())
    assert 1000 < short < rows
    monkeypatch.setenv("MEMO_CACHE", "0")
    with mq.region_index(path, "chrZ", qs, qe + k, k=k, num_docs=n, membership=False) as ix:
        assert ix.cache is None and ix.info()["rows"] == rows and ix.info()["bucket_base"] == 0
        assert np.array_equal(ix.conservation(qs, qe, k, n), _want_cons(oracle, s, e, o, qs, qe, k, n))
    monkeypatch.setenv("MEMO_CACHE", "read")
    for hint in (dict(num_docs=n, membership=False), {}):             # dense rows; 4-byte words
        with mq.region_index(path, "chrZ", qs, qe + k, k=k, **hint) as ix:
            inf = ix.info()
            assert ix.cache == "hit" and inf["bucket_base"] == qs >> 5, (inf["bucket_base"], qs >> 5)
            # (+ the rest of the two edge buckets; the dense rows leave out the rows that can never write at k <= 64: at the
            # least every row with an overlap of 0 .. 62 is there)
            assert (short if inf["dense_rows"] else rows) <= inf["rows"] <= rows + 2 * 32 * 8
            assert np.array_equal(ix.conservation(qs, qe, k, n), _want_cons(oracle, s, e, o, qs, qe, k, n))
            assert (ix.info()["last_sweep"] == 5) == bool(inf["dense_rows"])
