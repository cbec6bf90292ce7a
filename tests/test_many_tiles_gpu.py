"""`memo spectrum` and `memo lengths` where a workgroup takes MANY tiles: the loops that the sizes of their own suites never enter, at the
smallest sizes that enter them.

  - spectrum_kernel (memo_spectrum.hip) launches at most kMaxGrid workgroups, each walking tile = blockIdx.x; tile += gridDim.x with its
    LDS state alive across the tiles: 2 kMaxGrid + 1 whole tiles and a ragged one, in all four <MODE, PRIVATE> instances and at every
    mode-1 tile width, against spectrum_oracle.table_by_rank; and the private table flushed once per workgroup, counted.
  - the cell passes that maxk and lengths share (memo_cells.hip) with three planes at more tiles than one round of cells_scan_kernel and
    more cells than one pass of cells_fill_kernel's grid, on a pitch wider than L: begin and finish on the test's own buffer against an
    int64 suffix minimum, and once through the rows, whole and in two slices.
  - lengths_carry_kernel at more chunks than its kCarryWgs workgroups: stream_rows' chunk loop (memo_cells.h) goes round again.

Left out on purpose: the row passes of maxk and lengths are capped at 65 536 chunks (1.3 x 10^8 rows) and maxk's fill at 6.7 x 10^7 cells,
out of reach of a test of a few seconds.  Their chunk loop and fill stride are the same code as the carry pass and the lengths fill here.

Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import lengths_oracle, spectrum_oracle
from tests.test_lengths_gpu import differ as cells_differ
from tests.test_lengths_gpu import random_rows
from tests.test_spectrum_gpu import Device, abi_table, differ, rule_private, rule_tile

pytestmark = pytest.mark.gpu

GRID = 2048                              # memo_spectrum.hip: kMaxGrid, the workgroups of an add at most
FILL_WGS = 4096                          # memo_lengths.hip: cells_fill(P, 1 << 12, ..); a fill workgroup covers 1024 cells a pass
FILL_CELLS = 1024                        # memo_cells.hip: cells_fill_kernel, kThreads lanes of one 16-byte store
SCAN_ROUND = 4096                        # memo_cells.hip: kScanRound, the tile minima one round of cells_scan_kernel takes
CARRY_WGS = 1024                         # memo_lengths.hip: kCarryWgs, the workgroups of the carry pass at most
CHUNK_ROWS = 2048                        # memo_cells.h: 2 * kPairsPerWg, the rows a workgroup takes at a time
PAD = 0xABABABAB
NO_CARRY = np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture(scope="module")
def Tt(memo):
    from memo_amd import lengths
    t = lengths.tile()                   # memo_lengths_tile()
    assert t >= 512 and t % 64 == 0
    return t


@pytest.fixture()
def dev(memo):
    d = Device()
    yield d
    d.close()


# ---------------------------------------------------------------------------------------
# spectrum: every workgroup two tiles or more, and a ragged tail
# ---------------------------------------------------------------------------------------
#                n, kmax, membership, private, P, the ABI runs too
SPECTRUM_CASES = ((3, 31, False, True, 256, True),
                  (31, 1024, False, False, 256, False),     # 32 x 1025 = 32 800 words > 32 768: the smallest n at the largest KMAX
                  (3, 31, True, True, 256, False),
                  (33, 255, True, True, 128, False),
                  (5, 1024, True, True, 32, True),
                  (16, 1024, True, False, 32, True))        # 16 672 words of staging + 17 425 of table > 32 768
KINDS = 6


def spectrum_length(P):
    """(2 GRID + 1) P + r: workgroup 0 takes three whole tiles, workgroup 1 two and the ragged one, every other workgroup two"""
    r = 77 if P >= 128 else 5
    L = (2 * GRID + 1) * P + r
    assert 0 < r < P and r % 4 and L % 4
    ntiles = -(-L // P)
    per = [len(range(w, ntiles, GRID)) for w in range(GRID)]
    assert ntiles == 2 * GRID + 2 and per[:2] == [3, 3] and set(per[2:]) == {2} and L // P == ntiles - 1
    assert list(range(1, ntiles, GRID))[-1] == ntiles - 1          # (the ragged tile is workgroup 1's third)
    return L


def stretch_values(rng, n, L, P, kmax):
    """uint32 [n, L] in stretches of 3 P + 7 columns (their edges drift against the tiles), the kinds in turn: random in [0, KMAX]; all
    at KMAX; every bit width (mostly above KMAX); all 0; (g + p) % (KMAX + 1); all equal to one random value a stretch.  The first
    stretch and the last 2 P columns are random: the first and the last tile are mixed."""
    S = 3 * P + 7
    p = np.arange(L)
    stretch = p // S
    kind = stretch % KINDS
    kind[-2 * P:] = 0
    assert kind[0] == 0 and stretch[-1] >= 2 * KINDS
    v = rng.integers(0, kmax + 1, (n, L), dtype=np.uint32)
    v[:, kind == 1] = kmax
    at = np.flatnonzero(kind == 2)
    v[:, at] = (rng.integers(0, 2 ** 32, (n, len(at)), dtype=np.uint64) >> rng.integers(0, 32, (n, len(at)), dtype=np.uint64)).astype(np.uint32)
    v[:, kind == 3] = 0
    at = np.flatnonzero(kind == 4)
    v[:, at] = ((np.arange(n)[:, None] + at[None, :]) % (kmax + 1)).astype(np.uint32)
    at = np.flatnonzero(kind == 5)
    v[:, at] = rng.integers(0, kmax + 1, int(stretch[-1]) + 1, dtype=np.uint32)[stretch[at]][None, :]
    return v


@pytest.mark.parametrize("n,kmax,membership,private,P,abi", SPECTRUM_CASES)
def test_spectrum_every_workgroup_more_than_one_tile_and_a_ragged_tail(memo, dev, n, kmax, membership, private, P, abi):
    from memo_amd import spectrum
    assert spectrum.tile(n, kmax, membership) == rule_tile(kmax, membership) == P
    assert rule_private(n, kmax, membership) == private
    L = spectrum_length(P)
    values = stretch_values(np.random.default_rng([n, kmax, membership]), n, L, P, kmax)
    want = spectrum_oracle.table_by_rank(values, kmax, membership)
    # the reference alone
    assert (want.sum(axis=1) == L).all()
    assert ((want != 0).sum(axis=1) * 2 >= n + 1).any()            # for some k at least half of the columns v are taken
    assert want[kmax - 1, n] >= 3 * P                              # the stretches all at KMAX
    note = (n, kmax, membership)
    differ(spectrum.table(values, kmax, membership), want, note)
    if not abi:
        return
    # pitch L rounded up to 4, + 64, between poisoned words; then the same columns in two adds into one scratch: 2048 tiles and one
    # position, and what is left
    differ(abi_table(dev, [values], n, kmax, int(membership)), want, (note, "padded"))
    cut = GRID * P + 1
    differ(abi_table(dev, [values[:, :cut], values[:, cut:]], n, kmax, int(membership)), want, (note, "two adds"))


def test_spectrum_flushes_its_private_table_once_a_workgroup(memo):
    """a conserved window: two cells take every update.  The private table leaves a workgroup once, after its last tile -- 2 GRID
    global atomics, where a flush per tile would be 2 (2 GRID + 1); the same count says that the add launched GRID workgroups."""
    from memo_amd import _lib, spectrum
    L_ = _lib.use_ab(True)
    try:
        path, atomics = C.c_int32(-7), C.c_uint64(0)
        assert L_.memo_debug_spectrum_times(3, None, None, None) == 0
        for n, kmax, membership in ((3, 31, False), (3, 31, True), (5, 1024, True), (16, 1024, True)):
            L = spectrum_length(spectrum.tile(n, kmax, membership))
            got = spectrum.table(np.full((n, L), kmax, np.uint32), kmax, membership)
            assert L_.memo_debug_spectrum_times(3, None, C.byref(path), C.byref(atomics)) == 0
            assert (got[:, n] == L).all() and got[:, :n].sum() == 0, (n, kmax, membership)
            if n <= 5:
                assert path.value == 1 and rule_private(n, kmax, membership)
                assert atomics.value == 2 * GRID, (n, kmax, membership, atomics.value)
            else:
                assert path.value == 0 and not rule_private(n, kmax, membership)
                assert atomics.value >= 2, (n, kmax, membership, atomics.value)
    finally:
        L_.memo_debug_spectrum_times(0, None, None, None)
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# the shared cell passes: three planes, more tiles than one round of the scan, more cells than one pass of the fill, pitch > L
# ---------------------------------------------------------------------------------------
PLANES = 3
QS = 5_000_000


def cells_shape(Tt):
    L = (SCAN_ROUND + 1) * Tt + 77
    assert L > FILL_WGS * FILL_CELLS and -(-L // Tt) > SCAN_ROUND + 1 and L % 4 == 1
    return L, ((L + 3) & ~3) + 64


def lay(cells, pitch):
    """[n, L] -> four poisoned words, the planes on `pitch` with [L, pitch) poisoned, four poisoned words"""
    n, L = cells.shape
    whole = np.full(4 + n * pitch + 4, PAD, np.uint32)
    whole[4:-4].reshape(n, pitch)[:, :L] = cells
    return whole


def planes_between_poison(whole, n, L, pitch, note):
    assert (whole[:4] == PAD).all() and (whole[-4:] == PAD).all(), (note, "the words around the cells were written")
    body = whole[4:-4].reshape(n, pitch)
    assert (body[:, L:] == PAD).all(), (note, "cells at [L, pitch) were written")
    return body[:, :L]


def suffix_minimum(cells, cap):
    """int64 cells [n, L] -> what finish leaves: clip(min(cell[i ..]) - i, 0, cap)"""
    L = cells.shape[1]
    want = np.empty(cells.shape, np.uint32)
    for g, plane in enumerate(cells):
        want[g] = np.clip(np.minimum.accumulate(plane[::-1])[::-1] - np.arange(L), 0, cap)
    return want


def finish_on_own_buffer(dev, cells, cap, want, note):
    n, L = cells.shape
    pitch = ((L + 3) & ~3) + 64
    assert cells.min() >= 0 and cells.max() <= L - 1 + cap < 2 ** 32
    d = dev.put(lay(cells, pitch)) + 16
    dev.check(dev.lib.memo_lengths_finish_dev(d, L, pitch, n, cap, 0, None))
    got = planes_between_poison(dev.get(d - 16, 4 + n * pitch + 4, np.uint32), n, L, pitch, note)
    dev.close()
    cells_differ(got, want, note)


def test_cells_begin_fills_three_long_planes_and_takes_the_carry(dev, Tt):
    L, pitch = cells_shape(Tt)
    n, cap = PLANES, 700
    ident = L - 1 + cap
    d = dev.put(np.full(4 + n * pitch + 4, PAD, np.uint32)) + 16
    carry = np.asarray([QS + 5, NO_CARRY, QS + L - 1 + cap], np.int64)             # 5; untouched; lands on the identity
    dev.check(dev.lib.memo_lengths_begin_dev(d, L, pitch, n, cap, QS, dev.put(carry), 0, None))
    got = planes_between_poison(dev.get(d - 16, 4 + n * pitch + 4, np.uint32), n, L, pitch, "begin")
    for g in range(n):
        wrong = np.flatnonzero(got[g, :L - 1] != ident)
        assert not len(wrong), (g, len(wrong), wrong[:5], got[g, wrong[:5]])
    assert got[:, L - 1].tolist() == [ident if c == NO_CARRY else int(np.clip(c - QS, 0, ident)) for c in carry.tolist()] == [5, ident, ident]


def test_cells_finish_dense_bounds_on_three_long_planes(dev, Tt):
    """2 % of the cells bound their neighbourhood: most tiles answer from beyond themselves; plane 1 has one bound, in its last cell, and
    every tile of it answers from the scan's carry alone"""
    L, _ = cells_shape(Tt)
    n, cap = PLANES, 700
    ident = L - 1 + cap
    cells = np.full((n, L), ident, np.int64)
    for g in (0, 2):
        rng = np.random.default_rng([31, g])                                       # every plane its own stream
        hit = np.flatnonzero(rng.random(L) < 0.02)
        cells[g, hit] = np.minimum(hit + rng.integers(1, 3 * cap, len(hit)), ident)
    cells[1, L - 1] = L + 3
    want = suffix_minimum(cells, cap)
    for g in (0, 2):
        assert ((want[g] > 0) & (want[g] < cap)).sum() * 2 >= L, g
    assert not np.array_equal(want[0], want[2])
    assert want[1, L - 1] == 4 and (want[1, :L - cap] == cap).all() and (want[1, L - cap + 4:] < cap).all()
    finish_on_own_buffer(dev, cells, cap, want, "dense")


def test_cells_finish_sparse_long_bounds_and_the_seam_of_the_scan_rounds(dev, Tt):
    """a cap beyond the window: a bound reaches across every tile left of it, so the answers come through the scan's carry, across the
    seam of its two rounds (the tiles are taken from the right: the first round ends at tile ntiles - SCAN_ROUND)"""
    L, _ = cells_shape(Tt)
    n, cap = PLANES, 3 * Tt * SCAN_ROUND
    ident = L - 1 + cap
    ntiles = -(-L // Tt)
    seam = (ntiles - SCAN_ROUND) * Tt
    assert Tt <= seam < L - 2 * Tt
    cells = np.full((n, L), ident, np.int64)
    for g in range(n):
        rng = np.random.default_rng([32, g])
        j = rng.integers(0, L, 3000)
        np.minimum.at(cells[g], j, np.minimum(j + rng.integers(1, 2 * L, len(j)), ident))
        for d in (-Tt, -1, 0, 1, 2, Tt):
            cells[g, seam + d] = min(cells[g, seam + d], seam + d + 3 * Tt)
        cells[g, 0] = min(cells[g, 0], 2 * seam)
        # (those bounds rise with their cell, so each tile still answers from itself.)  One bound just right of the seam and below
        # every bound left of it: both tiles of the second round answer from the first round, through the register that chains them
        cells[g, seam + 3 + g] = seam + Tt // 2 + g
        assert cells[g, seam:].min() == seam + Tt // 2 + g < cells[g, :seam].min()
    want = suffix_minimum(cells, cap)
    for g in range(n):
        assert len(np.unique(want[g])) > 1000, g
        assert want[g, seam - 1] == Tt // 2 + g + 1 < cap, g                        # the answer left of the seam comes from the other round
        assert want[g, 0] == seam + Tt // 2 + g
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    finish_on_own_buffer(dev, cells, cap, want, "sparse")


def test_cells_through_the_rows_whole_and_in_two_slices(memo, Tt):
    from memo_amd import lengths
    L, _ = cells_shape(Tt)
    n, cap = PLANES, 500
    qs, qe = QS, QS + L
    rows = random_rows(np.random.default_rng(33), qs, qe, cap, 400_000, tuple(range(n)) + (-1, n, 2 ** 40))
    want = lengths_oracle.planes(*rows, qs, qe, cap, n)
    assert all(((want[g] > 0) & (want[g] < cap)).sum() * 2 >= L for g in range(n))
    cells_differ(lengths.planes(*rows, qs, qe, n, cap=cap, chunk_rows=150_001), want, "whole")
    step = L // 2 + 3                                                              # two slices, each longer than one pass of the fill
    assert L - step > FILL_WGS * FILL_CELLS and len(lengths.window_slices(qs, L, n, step)) == 2
    cells_differ(lengths.planes(*rows, qs, qe, n, cap=cap, chunk_rows=150_001, slice_positions=step), want, "two slices")
    assert np.array_equal(lengths.kth(*rows, qs, qe, n, threshold=2, cap=cap, chunk_rows=150_001, slice_positions=step), lengths_oracle.select(want, 2))


# ---------------------------------------------------------------------------------------
# the carry pass: more chunks than workgroups
# ---------------------------------------------------------------------------------------
def test_carry_takes_more_chunks_than_it_has_workgroups(dev):
    """1027 chunks over 1024 workgroups: the first three go round again, and the odd last row is taken singly.  The minimum of genome
    0 lies in a workgroup's second chunk, that of genome 1 in the first chunk, that of genome 3 in the very last row; genome 2 has no row.
    The columns lie between rows that would take every minimum, at the three alignments that choose the loads."""
    lib, n = dev.lib, 5
    m = (CARRY_WGS + 3) * CHUNK_ROWS + 1
    assert m % 2 == 1 and -(-(m // 2) // (CHUNK_ROWS // 2)) == CARRY_WGS + 3
    rng = np.random.default_rng(41)
    s, e, a = rng.integers(0, 1000, m), rng.integers(-2 ** 40, 2 ** 40, m), rng.choice(np.array([0, 1, 3, 4, -1, n, 2 ** 40]), m)
    lo, hi = 100, 900
    second, first, last = CARRY_WGS * CHUNK_ROWS + CHUNK_ROWS + 77, 5, m - 1
    assert (second - 1) // CHUNK_ROWS >= CARRY_WGS and first + 1 < CHUNK_ROWS     # (whether or not a head row shifts the chunks by one)
    for row, g, end in ((second, 0, -2 ** 41), (first, 1, -2 ** 41 - 1), (last, 3, -2 ** 41 - 2)):
        s[row], e[row], a[row] = 500, end, g
    want = np.full(n, NO_CARRY, np.int64)
    take = (s > lo) & (s < hi) & (a >= 0) & (a < n)
    np.minimum.at(want, a[take], e[take])
    assert want.tolist()[:4] == [-2 ** 41, -2 ** 41 - 1, NO_CARRY, -2 ** 41 - 2] and -2 ** 40 <= want[4] < 2 ** 40
    assert (e < -2 ** 40).sum() == 3
    for offs in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):                                 # 16-byte loads; 16-byte loads behind a head row; 8-byte loads
        ptrs = []
        for col, fill, off in zip((s, e, a), (500, -2 ** 62, None), offs):
            if fill is None:                                                       # poison rows of every genome
                head, tail = np.arange(4 + off) % n, np.arange(8) % n
            else:
                head, tail = np.full(4 + off, fill), np.full(8, fill)
            ptrs.append(dev.put(np.concatenate([head, col, tail]).astype(np.int64)) + 8 * (4 + off))
        assert [p % 16 for p in ptrs] == [8 * off for off in offs]
        for calls in (1, 3):
            d_carry = dev.put(np.full(n + 2, NO_CARRY, np.int64)) + 8
            step = -(-m // calls)
            for at in range(0, m, step):
                rows = min(step, m - at)
                dev.check(lib.memo_lengths_carry_dev(*(p + 8 * at for p in ptrs), rows, lo, hi, n, d_carry, 0, None))
            got = dev.get(d_carry - 8, n + 2, np.int64)
            assert np.array_equal(got[1:-1], want) and got[0] == got[-1] == NO_CARRY, (offs, calls, got.tolist())
        dev.close()
