"""`memo maxk` on the GPU: the kernels of memo_amd/csrc/memo_maxk.hip against the definition in NumPy (tests/maxk_oracle.py), against the
existing sweeps on the device ("shared at k" is k <= maxk, for rows with end >= start), and the command line against the oracle's text.

Every comparison is exact.  Rows with end < start are compared with the formula only: equality with a per-k query is not promised
for them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import maxk_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
SCAN_ROUND = 4096                       # tile minima one round of cells_scan_kernel takes (memo_cells.hip: kScanRound)
CAP_MAX = 2 ** 31 - 1
N, T = 7, 3                             # the structure tests: annots 0 .. 2 are selected by threshold 3
ODD_ANNOTS = (-1, N, 2 ** 40)           # never selected by a threshold, whatever it is


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture(scope="module")
def Tt(memo):
    from memo_amd import maxk
    t = maxk.tile()
    assert t >= 512 and t % 64 == 0
    return t


def check_equal(rows, qs, qe, cap, note, **kw):
    """the device's answer for host columns == the oracle's; returns it"""
    from memo_amd import maxk
    pred = {k: kw.pop(k) for k in ("threshold", "genome") if k in kw}
    want = maxk_oracle.maxk(*rows, qs, qe, cap, **pred)
    got = maxk.maxk(*rows, qs, qe, cap=cap, **pred, **kw)
    assert got.dtype == np.uint32 and got.shape == want.shape, note
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{note}: {len(bad)} of {len(want)} positions differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")
    return got


def cols(rows):
    """[(s, e, a), ...] -> three int64 columns"""
    arr = np.asarray(rows, np.int64).reshape(-1, 3)
    return arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy()


def random_rows(rng, qs, qe, cap, n, annots, overlap=300):
    """start-sorted rows with end >= start around the window, some left of it, some right of qe + cap"""
    reach = min(cap, 60)
    s = np.sort(rng.integers(qs - 10, qe + reach + 10, n))
    e = s + rng.integers(0, overlap, n)
    a = rng.choice(np.asarray(annots, np.int64), n)
    return s, e, a


def lengths(Tt):
    return (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, Tt - 1, Tt, Tt + 1, 2 * Tt - 1, 2 * Tt, 2 * Tt + 1)


# ---------------------------------------------------------------------------------------
# row structures at every length around the lane, the wave, the tile
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (40, CAP_MAX))
def test_row_structures_at_every_length(memo, Tt, cap):
    qs = 1000
    annots = tuple(range(N)) + ODD_ANNOTS
    for L in lengths(Tt):
        qe = qs + L
        rng = np.random.default_rng([L, cap % 1000])
        one = lambda s, e, a=0: cols([(s, e, a)])                                    # noqa: E731
        cases = [("no rows", cols([])),
                 ("one row right of the window", one(qe, qe + 3)),
                 ("a row that is not selected", one(qs + 1, qs + 1, T))]
        # one row each at the edges of the start filter: qs and qe + cap are ignored, the others count
        for name, s in (("qs", qs), ("qs + 1", qs + 1), ("qe - 1", qe - 1), ("qe", qe), ("qe + cap - 1", qe + cap - 1), ("qe + cap", qe + cap)):
            cases.append((f"one row at s = {name}", one(s, s + 2)))
        if L >= 1:
            got = check_equal(one(qe + cap - 1, qe + cap - 1), qs, qe, cap, (L, "the last start that counts"), threshold=T)
            assert (got == cap).all()                                                 # e - p >= cap everywhere
            got = check_equal(one(qs + 1, qs + 1), qs, qe, cap, (L, "the first start that counts"), threshold=T)
            assert got[0] == 1 and (got[1:] == cap).all()
        # a bound in the last cell of a tile, in the first cell of the next, and one position either side of them
        for t in (1, 2):
            for d in (-1, 0, 1, 2):
                s = qs + t * Tt + d                                                  # cell s - 1 - qs = t Tt - 1 + d
                cases.append((f"tile {t} edge {d:+d}", one(s, s + 2)))
            cases.append((f"tile {t} edge, all four", cols([(qs + t * Tt + d, qs + t * Tt + 9 - 2 * d, 1) for d in (-1, 0, 1, 2)])))
        cases.append(("nested: a later start has a smaller end", cols([(qs + 2, qs + 50, 0), (qs + 10, qs + 12, 1), (qs + 11, qs + 40, 2)])))
        mid = qs + L // 2 + 1
        cases.append(("10^4 rows on one start", (np.full(10_000, mid), mid + rng.integers(5, 5000, 10_000), rng.integers(0, T, 10_000))))
        rnd = random_rows(rng, qs, qe, cap, min(max(4 * L, 64), 20_000), annots)
        cases.append(("random start-sorted rows", rnd))
        for name, rows in cases:
            check_equal(rows, qs, qe, cap, (L, cap, name), threshold=T)
        want = check_equal(rnd, qs, qe, cap, (L, cap, "random rows"), threshold=T)
        order = rng.permutation(len(rnd[0]))
        shuffled = tuple(c[order] for c in rnd)
        assert np.array_equal(check_equal(shuffled, qs, qe, cap, (L, cap, "shuffled"), threshold=T), want)
        for calls in (1, 2, 7):
            got = check_equal(shuffled, qs, qe, cap, (L, cap, calls), threshold=T, chunk_rows=-(-len(order) // calls))
            assert np.array_equal(got, want), (L, cap, calls)
        if L >= 255:
            assert (want < cap).any() and len(np.unique(want)) > 10                  # (the rows do bound the window)


def test_more_tiles_than_one_round_of_the_tile_scan_and_a_tail(memo, Tt):
    L = (SCAN_ROUND + 1) * Tt + 77
    assert -(-L // Tt) > SCAN_ROUND + 1 and L % Tt
    qs, cap = 5_000_000, 1000
    qe = qs + L
    assert np.array_equal(check_equal(cols([]), qs, qe, cap, "no rows", threshold=T), np.full(L, cap, np.uint32))
    # one row right of the window: every tile of both rounds answers from the carry
    got = check_equal(cols([(qe + 5, qe + 7, 0)]), qs, qe, cap, "one row right", threshold=T)
    assert got[-1] == 8 and got[-990] == 997 and (got[:-1000] == cap).all()
    # bounds around the seam of the two rounds (the tiles are taken from the right: the first round ends at tile ntiles - SCAN_ROUND)
    ntiles = -(-L // Tt)
    seam = (ntiles - SCAN_ROUND) * Tt
    rows = [(qs + seam + d, qs + seam + d + 3 * Tt, 0) for d in (-Tt, -1, 0, 1, 2, Tt)] + [(qs + 1, qs + 2 * seam, 1), (qe - 1, qe + 500, 2)]
    check_equal(cols(rows), qs, qe, cap, "bounds at the seam of the rounds", threshold=T)
    cap = 3 * Tt * SCAN_ROUND                                                       # a carry that crosses every tile
    rng = np.random.default_rng(11)
    rnd = random_rows(rng, qs, qe, cap, 3000, range(N), overlap=2 * L)
    want = check_equal(rnd, qs, qe, cap, "sparse random rows with long overlaps", threshold=T)
    assert len(np.unique(want)) > 1000
    rnd = random_rows(rng, qs, qe, 500, 400_000, range(N), overlap=400)
    check_equal(rnd, qs, qe, 500, "dense random rows", threshold=N, chunk_rows=150_001)


def test_both_row_pass_variants_give_the_same_cells(memo, Tt):
    """one atomic per row (the A/B of DESIGN.md 10.5) against the product's wave-aggregated atomics, through the A/B library: sorted rows (long runs of one cell), shuffled
    rows (runs of one), all rows on one start, nothing selected in a wave"""
    from memo_amd import _lib
    qs, cap = 77, 5000
    _lib.use_ab(True)
    try:
        for L in (1, 65, Tt + 1, 2 * Tt + 1, 40 * Tt + 3):
            qe = qs + L
            rng = np.random.default_rng(L)
            dense = random_rows(rng, qs, qe, cap, 50_000, range(N), overlap=3000)             # many rows per cell at the small lengths
            order = rng.permutation(50_000)
            sparse = random_rows(rng, qs, qe, cap, 50_001, (0,) + (N,) * 200)                 # most waves select nothing
            mid = qs + L // 2 + 1
            one = (np.full(10_000, mid), mid + rng.integers(5, 5000, 10_000), rng.integers(0, T, 10_000))
            for name, rows in (("sorted", dense), ("shuffled", tuple(c[order] for c in dense)), ("sparse", sparse), ("one start", one),
                               ("odd row count", tuple(c[:49_999] for c in dense)), ("three rows", tuple(c[:3] for c in dense))):
                got = []
                for way in (1, 0):
                    _lib.check(_lib.lib().memo_debug_maxk_rows(way))
                    got.append(check_equal(rows, qs, qe, cap, (L, name, way), threshold=T))
                assert np.array_equal(*got), (L, name)
    finally:
        _lib.lib().memo_debug_maxk_rows(0)
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# predicate, cap, rows with end < start, far coordinates
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", (5, 100, 500))
def test_predicates(memo, Tt, n_docs):
    qs, L, cap = 12_345, 2 * Tt + 1, 1000
    qe = qs + L
    rng = np.random.default_rng(n_docs)
    annots = tuple(range(n_docs)) + (-1, n_docs, 2 ** 40) * max(n_docs // 20, 1)
    rows = random_rows(rng, qs, qe, cap, 30_000, annots)
    assert all((rows[2] == odd).any() for odd in (-1, n_docs, 2 ** 40))
    seen = []
    for t in (1, n_docs // 2, n_docs):
        seen.append(check_equal(rows, qs, qe, cap, ("threshold", t), threshold=t))
    assert (seen[0] >= seen[1]).all() and (seen[1] >= seen[2]).all() and (seen[0] != seen[2]).any()      # more rows selected: no longer
    odd_only = tuple(c[np.isin(rows[2], (-1, n_docs, 2 ** 40))] for c in rows)
    assert (check_equal(odd_only, qs, qe, cap, "annots outside [0, N)", threshold=n_docs) == cap).all()  # never selected in mode 0
    for g in (0, 1, n_docs - 1):
        check_equal(rows, qs, qe, cap, ("genome", g), genome=g)
    got = check_equal(rows, qs, qe, cap, "genome 2^40: the annot is compared as the int64 it is", genome=2 ** 40)
    assert (got < cap).any()
    assert (check_equal(rows, qs, qe, cap, "a genome without rows", genome=n_docs + 7) == cap).all()
    from memo_amd import maxk
    with pytest.raises(ValueError):
        maxk.maxk(*rows, qs, qe)
    with pytest.raises(ValueError):
        maxk.maxk(*rows, qs, qe, threshold=1, genome=1)


@pytest.mark.parametrize("cap", (1, 2, 255, 65536, CAP_MAX))
def test_caps(memo, Tt, cap):
    qs = 999
    for L in (1, 257, Tt + 1):
        qe = qs + L
        rng = np.random.default_rng([L, cap % 997])
        check_equal(random_rows(rng, qs, qe, cap, 5000, range(N)), qs, qe, cap, (L, "random rows"), threshold=T)
        ident = L - 1 + cap
        got = check_equal(cols([(qe, qs + ident, 0)]), qs, qe, cap, (L, "a clamp that lands on the identity"), threshold=T)
        assert (got == cap).all()
        got = check_equal(cols([(qe, qs + ident - 1, 0)]), qs, qe, cap, (L, "one position short of it"), threshold=T)
        assert got[-1] == cap - 1 and (L == 1 or got[0] == cap)
        got = check_equal(cols([(qe, qs + ident + 2 ** 33, 0), (qs + 1, 2 ** 61, 1)]), qs, qe, cap, (L, "far beyond it"), threshold=T)
        assert (got == cap).all()
    from memo_amd import maxk
    for bad in (0, -1, CAP_MAX + 1):
        with pytest.raises(ValueError):
            maxk.maxk([], [], [], 0, 10, threshold=1, cap=bad)


def test_rows_with_end_before_start_take_the_formula(memo, Tt):
    """legal input; the result can be 0; no per-k query is compared with"""
    qs, cap = 50_000, 600
    for L in (33, Tt - 1, 2 * Tt + 1):
        qe = qs + L
        rng = np.random.default_rng(L)
        zeros = 0
        for back in (1, 2, 400):
            s, e, a = random_rows(rng, qs, qe, cap, max(L // 8, 8), range(N))
            e = s - back
            got = check_equal((s, e, a), qs, qe, cap, (L, back), threshold=N)
            zeros += int((got == 0).sum())
            mixed = tuple(np.concatenate([x, y]) for x, y in zip((s, e, a), random_rows(rng, qs, qe, cap, L, range(N))))
            check_equal(mixed, qs, qe, cap, (L, back, "mixed with ordinary rows"), threshold=N)
        assert zeros > 0
        check_equal(cols([(qe + 5, qs - 10 ** 12, 0)]), qs, qe, cap, "an end far left of the window", threshold=1)
        check_equal(cols([(qe + 5, -2 ** 62, 0), (qs + 3, 2 ** 62, 0)]), qs, qe, cap, "ends at both ends of int64's middle half", threshold=1)


@pytest.mark.parametrize("qs", (2 ** 32 + 5, 2 ** 33 + 12_345))
def test_coordinates_past_2_to_the_32(memo, Tt, qs):
    L, cap = 2 * Tt + 77, 70_000
    qe = qs + L
    rng = np.random.default_rng(qs % 1000)
    rows = random_rows(rng, qs, qe, cap, 300, range(N), overlap=100_000)
    far = check_equal(rows, qs, qe, cap, "far", threshold=T)
    near = check_equal(tuple((rows[0] - qs + 100, rows[1] - qs + 100, rows[2])), 100, 100 + L, cap, "the same rows at the origin", threshold=T)
    assert np.array_equal(far, near) and (far < cap).any() and (far > 2 * Tt).any()
    # a row whose start differs from one inside the window by exactly 2^32: ignored, not aliased
    check_equal(cols([(qs + 10 + 2 ** 32, qs + 12 + 2 ** 32, 0), (qs + 10 - 2 ** 32, qs + 12, 0)]), qs, qe, cap, "2^32 apart", threshold=T)


# ---------------------------------------------------------------------------------------
# what the kernels may read and write; what is refused
# ---------------------------------------------------------------------------------------
class Device:
    """device buffers the test lays out itself"""

    def __init__(self):
        from memo_amd._lib import check, lib
        self.check, self.lib, self.held = check, lib(), []

    def put(self, host):
        host = np.ascontiguousarray(host)
        d = C.c_void_p()
        self.check(self.lib.memo_dev_malloc(0, max(host.nbytes, 16), C.byref(d)))
        self.held.append(d)
        if host.nbytes:
            self.check(self.lib.memo_dev_upload(0, d, host.ctypes.data, host.nbytes, None))
        assert d.value % 16 == 0
        return d.value

    def get(self, d, n, dtype):
        out = np.empty(n, dtype)
        if out.nbytes:
            self.check(self.lib.memo_dev_download(0, out.ctypes.data, d, out.nbytes, None))
        return out

    def close(self):
        for d in self.held:
            self.lib.memo_dev_free(0, d)


@pytest.fixture()
def dev(memo):
    d = Device()
    yield d
    d.close()


def test_nothing_outside_the_rows_or_the_cells_is_touched(dev, Tt):
    """the columns lie between rows that would zero the whole window, at every alignment the ABI allows (all three 16-byte aligned, all
    three 8 bytes off -- a first row taken alone --, mixed -- 8-byte loads); the cells lie between words that must stay as they are"""
    qs, cap = 4000, 900
    poison = (qs + 1, qs, 0)                                          # start qs + 1, end qs, annot 0: selected, bounds everything with 0
    PAD = 0xABABABAB
    for L in (1, 5, Tt - 1, 2 * Tt + 3):
        qe = qs + L
        for n in (1, 2, 3, 4, 513, 2048, 2049, 4099):
            rng = np.random.default_rng([L, n])
            rows = random_rows(rng, qs, qe, cap, n, (1, 2))          # (annot 0 is the poison's alone)
            want = maxk_oracle.maxk(*rows, qs, qe, cap, threshold=T)
            for offs in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)):
                base, ptrs = [], []
                for col, fill, off in zip(rows, poison, offs):
                    whole = np.concatenate([np.full(4 + off, fill, np.int64), col, np.full(8, fill, np.int64)])
                    d = dev.put(whole)
                    base.append(d)
                    ptrs.append(d + 8 * (4 + off))
                cells = np.full(L + 12, PAD, np.uint32)
                d_cells = dev.put(cells) + 16
                dev.check(dev.lib.memo_maxk_begin_dev(d_cells, L, cap, 0, None))
                dev.check(dev.lib.memo_maxk_rows_dev(*ptrs, n, qs, L, cap, 0, T, d_cells, 0, None))
                dev.check(dev.lib.memo_maxk_finish_dev(d_cells, L, cap, 0, None))
                got = dev.get(d_cells - 16, L + 12, np.uint32)
                assert np.array_equal(got[4:4 + L], want), (L, n, offs)
                assert (got[:4] == PAD).all() and (got[4 + L:] == PAD).all(), (L, n, offs)
            dev.close()
            dev.held = []


def test_refusals(dev):
    from memo_amd._lib import MEMO_EINVAL
    lib = dev.lib
    d = dev.put(np.zeros(64, np.int64))
    cells = dev.put(np.zeros(64, np.uint32))
    ok = (d, d + 128, d + 256, 8, 0, 16, 5, 0, 1, cells, 0, None)                 # start, end, annot, rows, qs, L, cap, mode, arg, cells
    assert lib.memo_maxk_begin_dev(cells, 16, 5, 0, None) == 0 and lib.memo_maxk_rows_dev(*ok) == 0
    assert lib.memo_maxk_rows_dev(d + 8, d + 128 + 8, d + 256 + 8, 8, 0, 16, 5, 0, 1, cells, 0, None) == 0      # 8-byte aligned columns are legal
    assert lib.memo_maxk_finish_dev(cells, 16, 5, 0, None) == 0

    def refused(rc, *words):
        msg = lib.memo_last_error().decode()
        assert rc == MEMO_EINVAL and all(w in msg for w in words), (rc, msg)
    for off in (4, 8, 12):                                                         # cells must be 16-byte aligned
        refused(lib.memo_maxk_begin_dev(cells + off, 16, 5, 0, None), "16-byte aligned")
        refused(lib.memo_maxk_rows_dev(*ok[:9], cells + off, 0, None), "16-byte aligned")
        refused(lib.memo_maxk_finish_dev(cells + off, 16, 5, 0, None), "16-byte aligned")
    for i in range(3):                                                             # each column must be 8-byte aligned
        for off in (1, 4):
            args = list(ok)
            args[i] += off
            refused(lib.memo_maxk_rows_dev(*args), "8-byte aligned")
    for L in (2 ** 31 + 1, 2 ** 40, -1):                                           # refused before anything is allocated or launched
        refused(lib.memo_maxk_begin_dev(cells, L, 5, 0, None), "2^31")
        refused(lib.memo_maxk_rows_dev(*ok[:5], L, *ok[6:]), "2^31")
        refused(lib.memo_maxk_finish_dev(cells, L, 5, 0, None), "2^31")
    for cap in (0, 2 ** 31, 2 ** 32 - 1):
        refused(lib.memo_maxk_begin_dev(cells, 16, cap, 0, None), "cap")
        refused(lib.memo_maxk_rows_dev(*ok[:6], cap, *ok[7:]), "cap")
        refused(lib.memo_maxk_finish_dev(cells, 16, cap, 0, None), "cap")
    refused(lib.memo_maxk_rows_dev(*ok[:7], 2, *ok[8:]), "mode")
    refused(lib.memo_maxk_rows_dev(*ok[:4], 2 ** 61 + 1, *ok[5:]), "2^61")
    refused(lib.memo_maxk_begin_dev(None, 16, 5, 0, None), "NULL")
    # L == 0 and rows == 0: nothing to do, nothing launched, NULL cells are fine
    assert lib.memo_maxk_begin_dev(None, 0, 5, 0, None) == 0 and lib.memo_maxk_finish_dev(None, 0, 5, 0, None) == 0
    assert lib.memo_maxk_rows_dev(d, d, d, 8, 0, 0, 5, 0, 1, None, 0, None) == 0
    assert lib.memo_maxk_rows_dev(None, None, None, 0, 0, 16, 5, 0, 1, cells, 0, None) == 0
    assert lib.memo_maxk_tile() == lib.memo_maxk_tile() >= 512


# ---------------------------------------------------------------------------------------
# "shared at k" of the existing sweeps on the device is k <= maxk
# ---------------------------------------------------------------------------------------
KS = (2, 3, 4, 8, 31, 32, 33, 64, 65, 101, 257)
CAP = 300
LEGAL = sorted({c["index"] for c in G.cases(raises=False)} - {"rnd_negoverlap.parquet"})          # every row has end >= start


@pytest.mark.parametrize("index", LEGAL)
def test_the_sweeps_agree_on_every_golden_window(memo, index):
    from memo_amd import maxk
    from memo_amd.index import DeviceIndex, bits_to_matrix
    windows = sorted({(c["region"], c["n"], c["membership"]) for c in G.cases(raises=False) if c["index"] == index})
    assert windows
    resident = {}
    try:
        for region, n, membership in windows:
            rec, se = region.split(":")
            qs, qe = map(int, se.split("-"))
            s, e, a = G.index_columns(index, rec)
            preds = [dict(genome=g) for g in range(min(6, n))] if membership else [dict(threshold=t) for t in sorted({1, max(n // 2, 1), n})]
            longest = []
            for p in preds:
                want = maxk_oracle.maxk(s, e, a, qs, qe, CAP, **p)
                got = maxk.maxk(s, e, a, qs, qe, cap=CAP, **p)
                assert np.array_equal(got, want), (region, p)
                longest.append(want.astype(np.int64))
            if not len(s):
                assert all((v == CAP).all() for v in longest)          # no rows: every k-mer is shared at every k
                continue
            if rec not in resident:
                resident[rec] = DeviceIndex.from_host(s, e, a)
            ix = resident[rec]
            for p, want in zip(preds, longest):                        # the same from the index's own device columns
                assert np.array_equal(maxk.index_maxk(ix, qs, qe, cap=CAP, **p), want), (region, p)
            for k in KS:
                if membership:
                    bits = bits_to_matrix(ix.membership(qs, qe, k, n), n)
                    shared = [bits[:, p["genome"]].astype(bool) for p in preds]
                else:
                    cons = ix.conservation(qs, qe, k, n).astype(np.int64)
                    shared = [cons >= p["threshold"] for p in preds]
                for p, sweep, length in zip(preds, shared, longest):
                    assert np.array_equal(sweep, k <= length), (index, region, k, p)
    finally:
        for ix in resident.values():
            ix.close()


def test_every_legal_golden_window_is_covered():
    assert len(LEGAL) == 7 and sum(len({(c["region"], c["n"], c["membership"]) for c in G.cases(raises=False) if c["index"] == i}) for i in LEGAL) >= 160


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_writes_one_integer_per_position(memo, tmp_path):
    cons, memb = os.path.join(G.GOLD, "example_cons.parquet"), os.path.join(G.GOLD, "example_memb.parquet")
    out = str(tmp_path / "k.txt")
    s, e, a = G.index_columns("example_cons.parquet", "ref_1")
    r = _memo("maxk", "-b", cons, "-n", "5", "-r", "ref_1:0-26", "-o", out)
    assert (r.returncode, r.stdout) == (0, b"MEMO - maxk\n"), r.stderr
    want = maxk_oracle.maxk(s, e, a, 0, 26, CAP_MAX, threshold=5)                   # -t defaults to N: shared by all
    assert open(out, "rb").read() == maxk_oracle.text(want) and len(want) == 26 and len(np.unique(want)) > 3
    assert _memo("maxk", "-b", cons, "-n", "5", "-r", "ref_1:3-30", "-o", out, "-t", "3", "-K", "2").returncode == 0
    want = maxk_oracle.maxk(s, e, a, 3, 30, 2, threshold=3)
    assert open(out, "rb").read() == maxk_oracle.text(want) and want.max() == 2 and want.min() == 1
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    assert _memo("maxk", "-b", memb, "-n", "5", "-r", "ref_1:0-26", "-o", out, "-m", "-d", "4", "-K", "12").returncode == 0
    want = maxk_oracle.maxk(s, e, a, 0, 26, 12, genome=4)
    assert open(out, "rb").read() == maxk_oracle.text(want) and want.min() < 12
    assert _memo("maxk", "-b", memb, "-n", "5", "-r", "ref_1:0-26", "-o", out, "-m", "-d", "0", "-K", "12").returncode == 0
    assert open(out, "rb").read() == b"12\n" * 26                                   # the pivot has no rows: every line is the cap
    assert _memo("maxk", "-b", cons, "-n", "5", "-r", "ref_1:5-5", "-o", out).returncode == 0
    assert open(out, "rb").read() == b""                                            # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["k.txt"]                                # written beside its name and renamed
    never = str(tmp_path / "never.txt")
    r = _memo("maxk", "-b", cons, "-n", "5", "-r", "ref_1:20-0", "-o", never)
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)


def test_region_maxk_streams_the_rows_of_a_far_window(memo, tmp_path):
    """a Parquet file of several row groups, shifted past 2^32: the chunks come in one by one, the answer is the oracle's"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import maxk
    s, e, a = G.index_columns("rnd_n40.parquet", "chr1")
    D = 2 ** 32 + 999
    path = str(tmp_path / "far.parquet")
    pq.write_table(pa.table({"f0": pa.array(["chr1"] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": a}), path, row_group_size=7001)
    assert pq.ParquetFile(path).metadata.num_row_groups > 5
    lo, hi = int(s.min()) + 100, int(s.max()) - 100
    for kw, cap in ((dict(threshold=40), CAP_MAX), (dict(threshold=7), 50), (dict(genome=3), 1000)):
        got = maxk.region_maxk(path, f"chr1:{lo + D}-{hi + D}", 40, cap=cap, **kw)
        assert np.array_equal(got, maxk_oracle.maxk(s, e, a, lo, hi, cap, **kw)), kw
    assert np.array_equal(maxk.region_maxk(path, f"chr1:{lo + D}-{hi + D}", 40), maxk_oracle.maxk(s, e, a, lo, hi, CAP_MAX, threshold=40))
    cons = os.path.join(G.GOLD, "example_cons.parquet")
    assert maxk.region_maxk(cons, "nochr:0-5", 5, cap=9).tolist() == [9] * 5          # a record without rows
    assert maxk.region_maxk(cons, "ref_1:5-5", 5).tolist() == []
    with pytest.raises(OSError):
        maxk.region_maxk(str(tmp_path / "no.parquet"), "chr1:0-20", 40)
    with pytest.raises(ValueError):
        maxk.region_maxk(path, "chr1:20-0", 40)
    with pytest.raises(ValueError):
        maxk.region_maxk(path, "chr1:0:20", 40)
