"""`memo lengths` on the GPU: the kernels of memo_amd/csrc/memo_lengths.hip against the definition in NumPy (tests/lengths_oracle.py),
against the shipped `memo maxk` genome mode and the shipped membership sweep on the device, the selection kernel alone against
np.sort, and the command line against the oracle's text.

Every comparison is exact.  Rows with end < start are compared with the formula only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import lengths_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
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
    t = lengths.tile()
    assert t >= 512 and t % 64 == 0
    return t


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
        self.held = []


@pytest.fixture()
def dev(memo):
    d = Device()
    yield d
    d.close()


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


def differ(got, want, note):
    assert got.dtype == np.uint32 and got.shape == want.shape, (note, got.shape, want.shape)
    if not np.array_equal(got, want):
        g, p = np.argwhere(got != want)[0]
        raise AssertionError(f"{note}: {(got != want).sum()} of {want.size} cells differ, first at genome {g}, position {p}: got {got[g, p]}, want {want[g, p]}")


def padded_planes(dev, rows, qs, L, cap, n, calls=1):
    """begin, rows (in `calls` calls), finish through the C ABI on planes of pitch L rounded up to 4, + 64, between poisoned words: the
    planes, after the check that every word outside [0, L) of a plane is as it was"""
    pitch = ((L + 3) & ~3) + 64
    whole = np.full(4 + n * pitch + 4, PAD, np.uint32)
    d_cells = dev.put(whole) + 16
    lib = dev.lib
    dev.check(lib.memo_lengths_begin_dev(d_cells, L, pitch, n, cap, qs, None, 0, None))
    m = len(rows[0])
    step = max(-(-m // calls), 1)
    for at in range(0, m, step):
        ptrs = [dev.put(c[at:at + step]) for c in rows]
        dev.check(lib.memo_lengths_rows_dev(*ptrs, len(rows[0][at:at + step]), qs, L, pitch, n, cap, d_cells, 0, None))
    dev.check(lib.memo_lengths_finish_dev(d_cells, L, pitch, n, cap, 0, None))
    got = dev.get(d_cells - 16, len(whole), np.uint32)
    dev.close()
    assert (got[:4] == PAD).all() and (got[-4:] == PAD).all()
    got = got[4:-4].reshape(n, pitch)
    assert (got[:, L:] == PAD).all(), "cells at [L, pitch) were written"
    return got[:, :L].copy()


def check_equal(dev, rows, qs, qe, cap, n, note, padded=True, **kw):
    """the device's planes for host columns == the oracle's, through memo_amd.lengths (pitch: L rounded up to 4) and, with `padded`,
    through the C ABI on a wider pitch; returns them"""
    from memo_amd import lengths
    want = lengths_oracle.planes(*rows, qs, qe, cap, n)
    differ(lengths.planes(*rows, qs, qe, n, cap=cap, **kw), want, note)
    if padded:
        differ(padded_planes(dev, rows, qs, qe - qs, cap, n), want, (note, "pitch L + 64"))
    return want


def lengths_around(Tt):
    return (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, Tt - 1, Tt, Tt + 1, 2 * Tt - 1, 2 * Tt, 2 * Tt + 1)


# ---------------------------------------------------------------------------------------
# rows and finish: row structures at every length around the lane, the wave, the tile, for few and many planes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 5, 33, 100))
def test_row_structures_at_every_length(memo, dev, Tt, n):
    qs = 1000
    odd = (-1, n, 2 ** 40)
    annots = tuple(range(n)) + odd * max(n // 10, 1)
    for L in lengths_around(Tt):
        cap = (40, CAP_MAX)[(L + n) % 2]
        qe = qs + L
        rng = np.random.default_rng([L, n])
        per_genome = lambda s, d=2: cols([(s, s + d + g % 3, g) for g in range(n)])        # noqa: E731
        cases = [("no rows", cols([])),
                 ("rows of no genome", cols([(qs + 1, qs + 1, a) for a in odd]))]
        # one row per genome at the edges of the start filter: qs and qe + cap are ignored, the others count
        for name, s in (("qs", qs), ("qs + 1", qs + 1), ("qe - 1", qe - 1), ("qe", qe), ("qe + cap - 1", qe + cap - 1), ("qe + cap", qe + cap)):
            cases.append((f"one row per genome at s = {name}", per_genome(s)))
        for t in (1, 2):                                                                  # the last cell of a tile, the first of the next
            cases.append((f"tile {t} edge", cols([(qs + t * Tt + d, qs + t * Tt + 9 - 2 * d + g, g) for d in (-1, 0, 1, 2) for g in range(n)])))
        cases.append(("nested: a later start has a smaller end", cols([(qs + 2, qs + 50, 0), (qs + 10, qs + 12, 0), (qs + 11, qs + 40, n - 1)])))
        mid = qs + L // 2 + 1
        cases.append(("10^4 rows on one start and genome", (np.full(10_000, mid), mid + rng.integers(5, 5000, 10_000), np.full(10_000, n - 1))))
        rnd = random_rows(rng, qs, qe, cap, min(max(4 * L, 64), 20_000), annots)
        assert L < 64 or all((rnd[2] == a).any() for a in odd)
        for back in (1, 2, 400):                                                          # rows with end < start: the formula, literally
            s, _, a = random_rows(rng, qs, qe, cap, max(L // 8, 8), annots)
            cases.append((f"e = s - {back}", (s, s - back, a)))
        for name, rows in cases:
            check_equal(dev, rows, qs, qe, cap, n, (L, cap, name))
        want = check_equal(dev, rnd, qs, qe, cap, n, (L, cap, "random sorted rows"))
        order = rng.permutation(len(rnd[0]))
        shuffled = tuple(c[order] for c in rnd)
        for calls in (1, 2, 7):
            assert np.array_equal(check_equal(dev, shuffled, qs, qe, cap, n, (L, cap, "shuffled", calls), padded=False,
                                              chunk_rows=-(-len(order) // calls)), want)
            differ(padded_planes(dev, shuffled, qs, L, cap, n, calls), want, (L, cap, "shuffled, pitch L + 64", calls))
        if L >= 1:
            got = check_equal(dev, per_genome(qe + cap - 1, 0), qs, qe, cap, n, (L, "the last start that counts"))
            assert (got == cap).all()                                                     # e - p >= cap everywhere
            got = check_equal(dev, cols([(qs + 1, qs + 1, g) for g in range(n)]), qs, qe, cap, n, (L, "the first start that counts"))
            assert (got[:, 0] == 1).all() and (got[:, 1:] == cap).all()
        if L >= 255 and n > 1:
            assert (want < cap).any() and len(np.unique(want)) > 10                       # (the rows do bound the window)


@pytest.mark.parametrize("cap", (1, 2, 255, 65536, CAP_MAX))
def test_caps(memo, dev, Tt, cap):
    qs, n = 999, 5
    for L in (1, 257, Tt + 1):
        qe = qs + L
        rng = np.random.default_rng([L, cap % 997])
        check_equal(dev, random_rows(rng, qs, qe, cap, 5000, range(n)), qs, qe, cap, n, (L, "random rows"))
        ident = L - 1 + cap
        got = check_equal(dev, cols([(qe, qs + ident, 1)]), qs, qe, cap, n, (L, "a clamp that lands on the identity"))
        assert (got == cap).all()
        got = check_equal(dev, cols([(qe, qs + ident - 1, 1)]), qs, qe, cap, n, (L, "one position short of it"))
        assert got[1, -1] == cap - 1 and (got[0] == cap).all()
        got = check_equal(dev, cols([(qe, qs + ident + 2 ** 33, 0), (qs + 1, 2 ** 61, 1)]), qs, qe, cap, n, (L, "far beyond it"))
        assert (got == cap).all()
    from memo_amd import lengths
    for bad in (0, -1, CAP_MAX + 1):
        with pytest.raises(ValueError):
            lengths.planes([], [], [], 0, 10, 3, cap=bad)


@pytest.mark.parametrize("n", (5, 33))
def test_every_plane_is_the_shipped_maxk_of_its_genome(memo, Tt, n):
    from memo_amd import lengths, maxk
    qs, L, cap = 12_345, 2 * Tt + 1, 1000
    qe = qs + L
    rng = np.random.default_rng(n)
    rows = random_rows(rng, qs, qe, cap, 30_000, tuple(range(1, n)) + (-1, n, 2 ** 40))
    planes = lengths.planes(*rows, qs, qe, n, cap=cap)
    for g in range(n):
        assert np.array_equal(planes[g], maxk.maxk(*rows, qs, qe, genome=g, cap=cap)), g
    assert (planes[0] == cap).all() and (planes[1:] < cap).any()                         # genome 0 has no rows, as the pivot
    for t in (1, 2, n // 2, n - 1, n):
        assert np.array_equal(lengths.kth(*rows, qs, qe, n, threshold=t, cap=cap), lengths_oracle.select(planes, t)), t


@pytest.mark.parametrize("qs", (2 ** 32 + 5, 2 ** 33 + 12_345))
def test_coordinates_past_2_to_the_32(memo, dev, Tt, qs):
    L, cap, n = 2 * Tt + 77, 70_000, 5
    qe = qs + L
    rng = np.random.default_rng(qs % 1000)
    rows = random_rows(rng, qs, qe, cap, 300, range(n), overlap=100_000)
    far = check_equal(dev, rows, qs, qe, cap, n, "far")
    near = check_equal(dev, tuple((rows[0] - qs + 100, rows[1] - qs + 100, rows[2])), 100, 100 + L, cap, n, "the same rows at the origin")
    assert np.array_equal(far, near) and (far < cap).any() and (far > 2 * Tt).any()
    # a row whose start differs from one inside the window by exactly 2^32: ignored, not aliased
    check_equal(dev, cols([(qs + 10 + 2 ** 32, qs + 12 + 2 ** 32, 1), (qs + 10 - 2 ** 32, qs + 12, 2)]), qs, qe, cap, n, "2^32 apart")
    from memo_amd import lengths
    assert np.array_equal(lengths.planes(*rows, qs, qe, n, cap=cap, slice_positions=Tt + 1), far)


# ---------------------------------------------------------------------------------------
# slices and the carry
# ---------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_slicing(memo, Tt):
    from memo_amd import lengths
    n = 5
    for step, L, cap in ((1, 70, 40), (1, 33, CAP_MAX), (7, 257, 40), (7, 64, 1), (64, 2 * Tt + 1, 300), (Tt + 1, 2 * Tt + 3, CAP_MAX), (Tt + 1, Tt + 1, 2)):
        qs = 5000
        qe = qs + L
        rng = np.random.default_rng([step, L])
        s, e, a = random_rows(rng, qs, qe, cap, 4 * L + 50, tuple(range(n)) + (-1, n, 2 ** 40))
        bounds = [qs + at for at in range(0, L, step)] + [qe]
        edge = []
        for b in bounds:                                             # rows starting at b and b + 1 of every slice bound (at most 40 bounds)
            edge += [(b, b + 3, 1), (b + 1, b + 2, 2)]
        edge = edge[:80] + [(qe - 1, qs - 7, 3),                      # e < s: reaches left across every slice
                            (qs + 2 * step + 1, qs - 1, 4),           # ... from the third slice
                            (qe + min(cap, 50) - 1, qs + 1, 3),       # ... from the tail
                            (qe, qe + 1, 1), (qe + cap - 1, qe + cap + 5, 2), (qe + cap, qs, 2), (qs, qs, 2), (qs + 1, qs + 1, 4)]
        extra = cols(edge)
        rows = tuple(np.concatenate([x, y]) for x, y in zip((s, e, a), extra))
        want = lengths_oracle.planes(*rows, qs, qe, cap, n)
        assert (want[3] == 0).any()
        differ(lengths.planes(*rows, qs, qe, n, cap=cap), want, (step, L, "whole"))
        differ(lengths.planes(*rows, qs, qe, n, cap=cap, slice_positions=step), want, (step, L, "sliced"))
        order = rng.permutation(len(rows[0]))
        differ(lengths.planes(*(c[order] for c in rows), qs, qe, n, cap=cap, slice_positions=step, chunk_rows=len(order) // 3 + 1), want,
               (step, L, "sliced, shuffled, three chunks"))
        for t in (1, 3, n):
            assert np.array_equal(lengths.kth(*rows, qs, qe, n, threshold=t, cap=cap, slice_positions=step), lengths_oracle.select(want, t)), (step, L, t)


def test_begin_takes_the_carry_and_carry_takes_minima(dev):
    """the two calls on their own: the carry's cell, clamped; minima over rows in any number of calls; annots outside [0, N) and starts
    outside (lo, hi) ignored; more workgroups than one"""
    lib, n = dev.lib, 5
    rng = np.random.default_rng(3)
    m = 300_001
    s, e, a = rng.integers(0, 1000, m), rng.integers(-2 ** 40, 2 ** 40, m), rng.choice(np.array([0, 1, 3, 4, -1, n, 2 ** 40]), m)
    lo, hi = 100, 900
    want = np.full(n, NO_CARRY, np.int64)
    take = (s > lo) & (s < hi) & (a >= 0) & (a < n)
    np.minimum.at(want, a[take], e[take])
    assert want[2] == NO_CARRY and (want[[0, 1, 3, 4]] != NO_CARRY).all()
    for calls in (1, 3):
        d_carry = dev.put(np.full(n + 2, NO_CARRY, np.int64)) + 8
        step = -(-m // calls)
        for at in range(0, m, step):
            ptrs = [dev.put(c[at:at + step]) for c in (s, e, a)]
            dev.check(lib.memo_lengths_carry_dev(*ptrs, len(s[at:at + step]), lo, hi, n, d_carry, 0, None))
        got = dev.get(d_carry - 8, n + 2, np.int64)
        assert np.array_equal(got[1:-1], want) and got[0] == got[-1] == NO_CARRY, calls
    # begin with that carry: cell L - 1 of every plane, clamped to [0, ident] relative to qs
    for qs, L, cap in ((0, 9, 50), (int(want[0]) - 3, 1, 7), (-2 ** 41, 130, CAP_MAX)):
        pitch = ((L + 3) & ~3) + 4
        d_cells = dev.put(np.full(n * pitch, PAD, np.uint32))
        carry = want.copy()
        carry[1] = qs + L - 1 + cap                                   # lands on the identity
        carry[3] = NO_CARRY - 1                                       # the largest end there is: e - qs would overflow for qs < 0
        carry[4] = np.iinfo(np.int64).min                             # ... and the smallest, for qs > 0
        dev.check(lib.memo_lengths_begin_dev(d_cells, L, pitch, n, cap, qs, dev.put(carry), 0, None))
        got = dev.get(d_cells, n * pitch, np.uint32).reshape(n, pitch)
        ident = L - 1 + cap
        assert (got[:, L:] == PAD).all() and (got[:, :L - 1] == ident).all()
        assert got[:, L - 1].tolist() == [ident if c == NO_CARRY else int(np.clip(c - qs, 0, ident)) for c in carry.tolist()], (qs, L, cap)
        dev.close()


# ---------------------------------------------------------------------------------------
# what the kernels may read; what is refused; what launches nothing
# ---------------------------------------------------------------------------------------
def test_nothing_outside_the_rows_is_read(dev, Tt):
    """the columns lie between rows that would zero every plane, at every alignment the ABI allows"""
    qs, cap, n = 4000, 900, 3
    for L in (5, Tt + 3):
        qe = qs + L
        for m in (1, 2, 3, 4, 2048, 2049, 4099):
            rng = np.random.default_rng([L, m])
            rows = random_rows(rng, qs, qe, cap, m, (1, 2))
            want = lengths_oracle.planes(*rows, qs, qe, cap, n)
            carry_want = np.full(n, NO_CARRY, np.int64)
            take = (rows[0] > qs) & (rows[0] < qe)
            np.minimum.at(carry_want, rows[2][take], rows[1][take])
            for offs in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)):
                ptrs = []
                for col, fill, off in zip(rows, (qs + 1, qs - 10 ** 6, None), offs):
                    if fill is None:                                   # poison rows of every genome
                        head, tail = np.arange(4 + off) % n, np.arange(8) % n
                    else:
                        head, tail = np.full(4 + off, fill), np.full(8, fill)
                    ptrs.append(dev.put(np.concatenate([head, col, tail]).astype(np.int64)) + 8 * (4 + off))
                pitch = (L + 3) & ~3
                d_cells = dev.put(np.zeros(n * pitch, np.uint32))
                dev.check(dev.lib.memo_lengths_begin_dev(d_cells, L, pitch, n, cap, qs, None, 0, None))
                dev.check(dev.lib.memo_lengths_rows_dev(*ptrs, m, qs, L, pitch, n, cap, d_cells, 0, None))
                dev.check(dev.lib.memo_lengths_finish_dev(d_cells, L, pitch, n, cap, 0, None))
                differ(dev.get(d_cells, n * pitch, np.uint32).reshape(n, pitch)[:, :L].copy(), want, (L, m, offs))
                d_carry = dev.put(np.full(n, NO_CARRY, np.int64))
                dev.check(dev.lib.memo_lengths_carry_dev(*ptrs, m, qs, qe, n, d_carry, 0, None))
                assert np.array_equal(dev.get(d_carry, n, np.int64), carry_want), (L, m, offs)
            dev.close()


def test_refusals_and_empty_calls(dev):
    from memo_amd._lib import MEMO_EINVAL
    lib, n, L, pitch, cap = dev.lib, 3, 16, 20, 5
    d = dev.put(np.zeros(64, np.int64))
    cells_host = np.full(n * pitch + 8, PAD, np.uint32)
    cells = dev.put(cells_host)
    out_host = np.full(32, PAD, np.uint32)
    out = dev.put(out_host)
    carry_host = np.full(n, NO_CARRY, np.int64)
    carry = dev.put(carry_host)
    begin = [cells, L, pitch, n, cap, 0, None, 0, None]              # cells, L, pitch, N, cap, qs, carry
    rows = [d, d + 128, d + 256, 8, 0, L, pitch, n, cap, cells, 0, None]    # start, end, annot, rows, qs, L, pitch, N, cap, cells
    carr = [d, d + 128, d + 256, 8, 0, 100, n, carry, 0, None]      # start, end, annot, rows, lo, hi, N, carry
    fin = [cells, L, pitch, n, cap, 0, None]
    sel = [cells, L, pitch, n, cap, 2, out, 0, None]                # cells, L, pitch, N, cap, T, out

    def unchanged():
        assert np.array_equal(dev.get(cells, len(cells_host), np.uint32), cells_host)
        assert np.array_equal(dev.get(out, 32, np.uint32), out_host) and np.array_equal(dev.get(carry, n, np.int64), carry_host)

    def refused(call, args, at, value, *words):
        args = list(args)
        args[at] = value
        rc = call(*args)
        msg = lib.memo_last_error().decode()
        assert rc == MEMO_EINVAL and all(w in msg for w in words), (at, value, rc, msg)
    with_cells = ((lib.memo_lengths_begin_dev, begin, dict(c=0, L=1, p=2, n=3, cap=4)), (lib.memo_lengths_rows_dev, rows, dict(c=9, L=5, p=6, n=7, cap=8)),
                  (lib.memo_lengths_finish_dev, fin, dict(c=0, L=1, p=2, n=3, cap=4)), (lib.memo_lengths_select_dev, sel, dict(c=0, L=1, p=2, n=3, cap=4)))
    for call, args, at in with_cells:
        for off in (4, 8, 12):
            refused(call, args, at["c"], cells + off, "16-byte aligned")
        refused(call, args, at["c"], None, "NULL")
        for bad in (2 ** 31 + 1, 2 ** 40, -1):
            refused(call, args, at["L"], bad, "2^31")
        for bad in (0, 2 ** 31, 2 ** 32 - 1):
            refused(call, args, at["cap"], bad, "cap")
        for bad in (0, -1, 2049):
            refused(call, args, at["n"], bad, "num_docs")
        for bad in (L - 1, 12, 18, 22, 0):
            refused(call, args, at["p"], bad, "pitch")
        refused(call, args, at["p"], 2 ** 31, "2^32")                # 3 planes of 2^31 cells
    huge = list(sel)
    huge[1:4] = [2 ** 21, 2 ** 21, 2048]                            # N pitch = 2^32 exactly
    refused(lib.memo_lengths_select_dev, huge, 0, cells, "2^32")
    for i in range(3):                                               # each column must be 8-byte aligned
        for off in (1, 4):
            refused(lib.memo_lengths_rows_dev, rows, i, rows[i] + off, "8-byte aligned")
            refused(lib.memo_lengths_carry_dev, carr, i, carr[i] + off, "8-byte aligned")
        refused(lib.memo_lengths_rows_dev, rows, i, None, "NULL")
        refused(lib.memo_lengths_carry_dev, carr, i, None, "NULL")
    for bad in (2 ** 61 + 1, -2 ** 61 - 1):
        refused(lib.memo_lengths_rows_dev, rows, 4, bad, "2^61")
        refused(lib.memo_lengths_begin_dev, begin, 5, bad, "2^61")
    refused(lib.memo_lengths_begin_dev, begin, 6, carry + 4, "d_carry")
    refused(lib.memo_lengths_carry_dev, carr, 7, carry + 4, "d_carry")
    refused(lib.memo_lengths_carry_dev, carr, 7, None, "d_carry")
    for bad in (0, 2049):
        refused(lib.memo_lengths_carry_dev, carr, 6, bad, "num_docs")
    for bad in (0, -1, n + 1):
        refused(lib.memo_lengths_select_dev, sel, 5, bad, "threshold")
    for off in (1, 2):
        refused(lib.memo_lengths_select_dev, sel, 6, out + off, "4-byte aligned")
    refused(lib.memo_lengths_select_dev, sel, 6, None, "NULL")
    unchanged()
    # L == 0 and rows == 0: nothing to do, nothing launched, NULL cells are fine
    assert lib.memo_lengths_begin_dev(None, 0, 0, n, cap, 0, None, 0, None) == 0 and lib.memo_lengths_finish_dev(None, 0, 0, n, cap, 0, None) == 0
    assert lib.memo_lengths_begin_dev(cells, 0, pitch, n, cap, 0, carry, 0, None) == 0 and lib.memo_lengths_finish_dev(cells, 0, pitch, n, cap, 0, None) == 0
    assert lib.memo_lengths_rows_dev(d, d, d, 8, 0, 0, 0, n, cap, None, 0, None) == 0
    assert lib.memo_lengths_rows_dev(None, None, None, 0, 0, L, pitch, n, cap, cells, 0, None) == 0
    assert lib.memo_lengths_carry_dev(None, None, None, 0, 0, 100, n, carry, 0, None) == 0
    assert lib.memo_lengths_carry_dev(d, d, d, 8, 100, 100, n, carry, 0, None) == 0         # an empty (lo, hi)
    assert lib.memo_lengths_select_dev(None, 0, 0, n, cap, 1, None, 0, None) == 0 and lib.memo_lengths_select_dev(cells, 0, pitch, n, cap, n, out, 0, None) == 0
    unchanged()
    # 8-byte aligned columns and a 4-byte aligned result are legal; select leaves the cells as they are
    assert lib.memo_lengths_begin_dev(*begin) == 0 and lib.memo_lengths_rows_dev(d + 8, d + 136, d + 264, 8, 0, L, pitch, n, cap, cells, 0, None) == 0
    assert lib.memo_lengths_finish_dev(*fin) == 0
    before = dev.get(cells, len(cells_host), np.uint32)
    assert lib.memo_lengths_select_dev(cells, L, pitch, n, cap, 2, out + 4, 0, None) == 0
    assert np.array_equal(dev.get(cells, len(cells_host), np.uint32), before) and (before.reshape(-1)[n * pitch:] == PAD).all()
    got = dev.get(out, 32, np.uint32)
    assert got[0] == PAD and (got[1:1 + L] == cap).all() and (got[1 + L:] == PAD).all()
    assert lib.memo_lengths_tile() == lib.memo_lengths_tile() >= 512
    assert [lib.memo_lengths_select_tile(v) for v in (0, 2049, -3)] == [0, 0, 0]
    from memo_amd import lengths
    for bad in (dict(n_docs=0), dict(n_docs=2049), dict(n_docs=3, threshold=0), dict(n_docs=3, threshold=4)):
        with pytest.raises(ValueError):
            lengths.kth([], [], [], 0, 10, **{"threshold": 1, **bad})
    with pytest.raises(ValueError):
        lengths.planes([], [], [], 10, 0, 3)
    assert lengths.planes([], [], [], 7, 7, 3).shape == (3, 0) and lengths.kth([], [], [], 7, 7, 3, threshold=2).shape == (0,)


# ---------------------------------------------------------------------------------------
# the selection kernel alone, against np.sort
# ---------------------------------------------------------------------------------------
# (119 | 120, 191 | 192, 383 | 384, 767 | 768, 1535 | 1536: the last N of a tile shape and the first of the next)
SELECT_N = (1, 2, 31, 32, 33, 63, 64, 65, 100, 119, 120, 129, 191, 192, 257, 383, 384, 500, 767, 768, 1030, 1535, 1536, 2048)
LDS_BUDGET, LDS_STATIC = 120 * 1024, 16      # memo_lengths.hip: kSelectLds, of which the kernel's static words


def select_lds(n, Ps):
    """bytes of LDS a select workgroup takes at n genomes and a tile of Ps positions: rows of Ps words, 5 Ps / 4 where lanes share a position"""
    return n * (Ps if Ps == 256 else Ps + Ps // 4) * 4 + LDS_STATIC
PATTERNS = 9


def select_values(rng, n, L, t, cap, shift):
    """uint32 [n, L]: column p holds pattern (p + shift) % PATTERNS"""
    v = np.empty((n, L), np.uint32)
    top = max(int(cap).bit_length() - 1, 0)                          # the top bit of the cap's range
    for p in range(L):
        kind = (p + shift) % PATTERNS
        x = int(rng.integers(0, min(cap, 2 ** 20) + 1))
        if kind == 0:
            col = np.full(n, x)                                      # all equal
        elif kind == 1:
            col = np.full(n, cap)                                    # all at the cap
        elif kind in (2, 3, 4):                                      # exactly T - 1, T, T + 1 genomes at or above a value
            at_or_above = min(max(t + kind - 3, 0), n)
            x = max(x, 1)
            col = np.concatenate([rng.integers(x, max(cap, x) + 1, at_or_above), rng.integers(0, x, n - at_or_above)])
            col[:min(1, at_or_above)] = x                            # (one of them exactly at it)
        elif kind == 5:
            col = (x >> 1) | (rng.integers(0, 2, n) << max(top - 1, 0))      # differ in the top bit under the cap only
        elif kind == 6:
            col = (x & ~1) | rng.integers(0, 2, n)                   # differ in the lowest bit only
        elif kind == 7:
            col = rng.integers(0, 2 ** 32, n) >> rng.integers(0, 3, n)      # mostly above the cap: taken as the cap
        else:
            col = rng.integers(0, 2 ** 32, n) >> rng.integers(0, 32, n)     # every bit width
        v[:, p] = rng.permutation(col).astype(np.uint32)
    return v


@pytest.mark.parametrize("n", SELECT_N)
def test_select_against_a_sort(memo, n):
    from memo_amd import lengths
    Ps = lengths.select_tile(n)
    assert Ps in (256, 128, 64, 32, 16, 8) and select_lds(n, Ps) <= LDS_BUDGET and (Ps == 256 or select_lds(n, 2 * Ps) > LDS_BUDGET)
    rng = np.random.default_rng(n)
    calls = 0
    for L in (1, Ps - 1, Ps, Ps + 1, 2 * Ps + 1):
        for t in sorted({1, min(2, n), max(n // 2, 1), max(n - 1, 1), n}):
            for cap in (1, 2, 255, CAP_MAX):
                values = select_values(rng, n, L, t, cap, calls)
                got = lengths.select(values, t, cap)
                want = lengths_oracle.select(values, t, cap)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (n, L, t, cap, np.flatnonzero(got != want)[:5])
                calls += 1
    assert calls >= 5 * 4


def test_every_select_tile_shape_is_taken():
    from memo_amd import lengths
    assert sorted({lengths.select_tile(n) for n in SELECT_N}) == [8, 16, 32, 64, 128, 256]
    assert any(select_lds(n, lengths.select_tile(n)) > 64 * 1024 for n in SELECT_N)       # the large-LDS opt-in
    assert max(select_lds(n, lengths.select_tile(n)) for n in range(1, 2049)) == select_lds(1535, 16) == LDS_BUDGET - 64
    assert [lengths.select_tile(n) for n in (119, 120, 191, 192, 383, 384, 767, 768, 1535, 1536)] == [256, 128, 128, 64, 64, 32, 32, 16, 16, 8]
    tiles = [lengths.select_tile(n) for n in range(1, 2049)]
    assert all(a >= b for a, b in zip(tiles, tiles[1:])) and tiles[0] == 256 and tiles[-1] == 8


# ---------------------------------------------------------------------------------------
# the shipped membership sweep on the device: bit g is k <= len[g], popcount >= T is k <= sel_T
# ---------------------------------------------------------------------------------------
KS = (2, 3, 4, 8, 31, 32, 33, 64, 65, 101, 257)
CAP = 300
LEGAL = ("example_memb.parquet", "rnd_n4.parquet", "rnd_n8.parquet", "rnd_n40.parquet", "rnd_n70_sparse.parquet", "rnd_n130.parquet")


@pytest.mark.parametrize("index", LEGAL)
def test_the_membership_sweep_agrees_on_every_golden_window(memo, index):
    from memo_amd import lengths
    from memo_amd.index import DeviceIndex, bits_to_matrix
    windows = sorted({(c["region"], c["n"]) for c in G.cases(raises=False, membership=True) if c["index"] == index})
    assert windows
    resident = {}
    try:
        for region, n in windows:
            rec, se = region.split(":")
            qs, qe = map(int, se.split("-"))
            s, e, a = G.index_columns(index, rec)
            assert (e >= s).all()
            planes = lengths.planes(s, e, a, qs, qe, n, cap=CAP)
            differ(planes, lengths_oracle.planes(s, e, a, qs, qe, CAP, n), (index, region))
            ts = sorted({1, max(n // 2, 1), n})
            sel = [lengths.kth(s, e, a, qs, qe, n, threshold=t, cap=CAP) for t in ts]
            for t, got in zip(ts, sel):
                assert np.array_equal(got, lengths_oracle.select(planes, t)), (index, region, t)
            if not len(s):
                assert (planes == CAP).all()
                continue
            if rec not in resident:
                resident[rec] = DeviceIndex.from_host(s, e, a)
            ix = resident[rec]
            for k in KS:
                bits = bits_to_matrix(ix.membership(qs, qe, k, n), n).astype(bool)       # [L, N]
                assert np.array_equal(bits.T, k <= planes.astype(np.int64)), (index, region, k)
                held = bits.sum(axis=1)
                for t, got in zip(ts, sel):
                    assert np.array_equal(held >= t, k <= got.astype(np.int64)), (index, region, k, t)
    finally:
        for ix in resident.values():
            ix.close()


def test_across_index_kinds(memo):
    """`memo lengths -t T` on the membership index is `memo maxk -t T` on the conservation index of the same genomes"""
    from memo_amd import lengths, maxk
    cons, memb = os.path.join(G.GOLD, "example_cons.parquet"), os.path.join(G.GOLD, "example_memb.parquet")
    for region in ("ref_1:0-20", "ref_1:0-26", "ref_1:3-30"):
        for t in range(1, 6):
            for cap in (CAP_MAX, 4):
                want = maxk.region_maxk(cons, region, 5, threshold=t, cap=cap)
                assert np.array_equal(lengths.region_kth(memb, region, 5, t, cap), want), (region, t, cap)
                assert np.array_equal(lengths.region_kth(memb, region, 5, t, cap, slice_positions=7), want), (region, t, cap)
    assert lengths.region_kth(memb, "ref_1:0-20", 5).tolist() == [3, 2, 3, 2, 2, 2, 2, 4, 3, 2, 3, 2, 2, 3, 2, 3, 2, 3, 2, 2]
    assert lengths.region_kth(memb, "ref_1:0-20", 5, 3).tolist() == [5, 4, 4, 3, 3, 4, 5, 6, 5, 4, 4, 3, 3, 3, 3, 5, 4, 4, 3, 3]
    planes = lengths.region_planes(memb, "ref_1:0-20", 5)
    assert planes[1].tolist() == [3, 2, 3, 2, 3, 2, 2, 4, 3, 2, 3, 2, 4, 3, 2, 3, 2, 3, 2, 2] and (planes[0] == CAP_MAX).all()


def test_region_planes_stream_the_rows_of_a_far_window(memo, tmp_path):
    """a Parquet file of several row groups, shifted past 2^32: the tail and every slice's rows come in chunk by chunk"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import lengths
    s, e, a = G.index_columns("rnd_n8.parquet", "chr1")
    D = 2 ** 32 + 999
    path = str(tmp_path / "far.parquet")
    pq.write_table(pa.table({"f0": pa.array(["chr1"] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": a}), path,
                   row_group_size=max(len(s) // 7, 1))
    assert pq.ParquetFile(path).metadata.num_row_groups > 5
    lo, hi = int(s.min()) + 100, int(s.max()) - 100
    for cap in (CAP_MAX, 50):
        want = lengths_oracle.planes(s, e, a, lo, hi, cap, 8)
        for step in (None, (hi - lo) // 3 + 1, 1000):
            differ(lengths.region_planes(path, f"chr1:{lo + D}-{hi + D}", 8, cap, slice_positions=step), want, (cap, step))
            assert np.array_equal(lengths.region_kth(path, f"chr1:{lo + D}-{hi + D}", 8, 4, cap, slice_positions=step), lengths_oracle.select(want, 4))
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    assert lengths.region_kth(memb, "nochr:0-5", 5, cap=9).tolist() == [9] * 5           # a record without rows
    assert lengths.region_planes(memb, "ref_1:5-5", 5).shape == (5, 0)
    with pytest.raises(OSError):
        lengths.region_kth(str(tmp_path / "no.parquet"), "chr1:0-20", 8)
    with pytest.raises(ValueError):
        lengths.region_kth(path, "chr1:20-0", 8)
    with pytest.raises(ValueError):
        lengths.region_planes(path, "chr1:0:20", 8)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_writes_both_forms(memo, tmp_path):
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    out = str(tmp_path / "k.txt")
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    r = _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:0-26", "-o", out)
    assert (r.returncode, r.stdout) == (0, b"MEMO - lengths\n"), r.stderr
    planes = lengths_oracle.planes(s, e, a, 0, 26, CAP_MAX, 5)
    assert open(out, "rb").read() == lengths_oracle.text(lengths_oracle.select(planes, 5))          # -t defaults to N: held by all
    assert _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:0-26", "-o", out, "-a").returncode == 0
    assert open(out, "rb").read() == lengths_oracle.rows_text(planes) and len(np.unique(planes)) > 4
    capped = lengths_oracle.planes(s, e, a, 3, 30, 3, 5)
    assert _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:3-30", "-o", out, "-a", "-K", "3").returncode == 0
    assert open(out, "rb").read() == lengths_oracle.rows_text(capped) and capped.max() == 3 and capped.min() < 3
    assert _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:3-30", "-o", out, "-t", "3", "-K", "3").returncode == 0
    assert open(out, "rb").read() == lengths_oracle.text(lengths_oracle.select(capped, 3))
    # a window forced into slices of 7 positions: the -a file is still in position order, and nothing is left beside it
    for flags, want in ((("-a",), lengths_oracle.rows_text(planes)), (("-t", "3"), lengths_oracle.text(lengths_oracle.select(planes, 3)))):
        assert _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:0-26", "-o", out, *flags, env={"MEMO_LENGTHS_SLICE": "7"}).returncode == 0
        assert open(out, "rb").read() == want
    for flags in ((), ("-a",)):
        assert _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:5-5", "-o", out, *flags).returncode == 0
        assert open(out, "rb").read() == b""                                        # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["k.txt"]                                # written beside its name and renamed
    never = str(tmp_path / "never.txt")
    r = _memo("lengths", "-b", memb, "-n", "5", "-r", "ref_1:20-0", "-o", never)
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)
    r = _memo("lengths", "-b", str(tmp_path / "no.parquet"), "-n", "5", "-r", "ref_1:0-26", "-o", never, "-a", env={"MEMO_LENGTHS_SLICE": "7"})
    assert r.returncode == 1 and r.stderr.startswith(b"memo lengths: ") and sorted(os.listdir(tmp_path)) == ["k.txt"]
