"""What the side kernels share (memo_amd/csrc: memo::Laps, memo_cells.hip) and their own suites do not pin:

  - the timed form of every command that has one (the memo_debug_*_times switches of the A/B library): a timed call fills the slots
    that are its own with finite positive device times, leaves every other slot as it was, and computes what the untimed call computes;
  - memo_maxk_begin_dev + memo_maxk_finish_dev alone, on cells the test uploads: one plane of the shared plane kernels, at lengths
    around their tile and off the multiple of 4, between guard words.

Shapes: two tiles of the kernel under test (a few thousand positions), 3 planes where there are planes.  Every comparison is exact."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL_TILE = 2048                         # memo_cells.hip: kTile, the cells of a tile of the suffix minimum
PAD = 0xABABABAB
I64_MAX = np.iinfo(np.int64).max


class Device:
    """device buffers the test lays out itself"""

    def __init__(self, lib, check):
        self.lib, self.check, self.held = lib, check, []

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
def ab():
    """the A/B library (it has the switches), a Device on it, and every switch off again afterwards"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when the libraries are up to date
    L_ = _lib.use_ab(True)
    assert L_.memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    d = Device(L_, _lib.check)
    try:
        yield d
    finally:
        d.close()
        for name in SLOTS:
            switch(L_, name, 0)
        _lib.use_ab(False)


SLOTS = {"maxk": 5, "lengths": 7, "mems": 3, "spectrum": 2, "collect": 2, "cooc": 2, "tracks": 1}


def switch(lib, name, on):
    """sets the command's switch; returns its slots as they are"""
    ms = (C.c_float * SLOTS[name])()
    f = getattr(lib, f"memo_debug_{name}_times")
    assert (f(on, ms, None, None) if name == "spectrum" else f(on, ms)) == 0
    return list(ms)


def all_slots(lib, timed):
    """every command's slots, every switch left off but `timed`'s"""
    return {name: switch(lib, name, 1 if name == timed else 0) for name in SLOTS}


def timed_call(lib, name, call, touched):
    """call() with `name`'s switch on: the slots in `touched` are finite and positive afterwards, every other slot of every command is
    what it was.  Returns what call() returns."""
    before = all_slots(lib, name)
    got = call()
    after = all_slots(lib, None)
    for other in SLOTS:
        for i in range(SLOTS[other]):
            if other == name and i in touched:
                assert math.isfinite(after[name][i]) and after[name][i] > 0, (name, i, after[name])
            else:
                assert after[other][i] == before[other][i], (name, "changed", other, i, before[other], after[other])
    return got


def some_rows(rng, L, n, planes):
    """start-sorted rows with end >= start around [0, L), annots 0 .. planes - 1 and some that no plane takes"""
    s = np.sort(rng.integers(-10, L + 70, n)).astype(np.int64)
    e = s + rng.integers(0, 300, n)
    a = rng.choice(np.asarray(list(range(planes)) + [-1, planes, 2 ** 40], np.int64), n)
    return s, e, a


def some_bits(rng, L, n):
    """a membership result uint32 [L][W]: runs of equal rows, bits at or above n clear"""
    W = (n + 31) // 32
    rows = rng.integers(0, 2 ** 32, (L // 7 + 2, W), dtype=np.uint64).astype(np.uint32)
    bits = np.repeat(rows, 7, axis=0)[:L].copy()
    if n % 32:
        bits[:, -1] &= np.uint32((1 << (n % 32)) - 1)
    return bits, W


# ---------------------------------------------------------------------------------------
# (a) the seven timed forms
# ---------------------------------------------------------------------------------------
def test_maxk_timed(ab):
    lib, cap, L, T = ab.lib, 900, CELL_TILE + 77, 2
    rows = some_rows(np.random.default_rng(1), L, 5000, 3)
    cols = [ab.put(c) for c in rows]
    d_cells = ab.put(np.zeros(L, np.uint32))

    def run(wrap):
        wrap(lambda: ab.check(lib.memo_maxk_begin_dev(d_cells, L, cap, 0, None)), {0})
        wrap(lambda: ab.check(lib.memo_maxk_rows_dev(*cols, 5000, 0, L, cap, 0, T, d_cells, 0, None)), {1})
        wrap(lambda: ab.check(lib.memo_maxk_finish_dev(d_cells, L, cap, 0, None)), {2, 3, 4})
        return ab.get(d_cells, L, np.uint32)

    plain = run(lambda call, touched: call())
    timed = run(lambda call, touched: timed_call(lib, "maxk", call, touched))
    assert np.array_equal(plain, timed)
    assert len(np.unique(plain)) > 10                     # (the rows bound the positions, and not all alike)


def test_lengths_timed(ab):
    lib, cap, L, n, T = ab.lib, 900, CELL_TILE + 77, 3, 2
    pitch = (L + 3) // 4 * 4
    rows = some_rows(np.random.default_rng(2), L, 5000, n)
    cols = [ab.put(c) for c in rows]
    d_cells, d_out = ab.put(np.zeros(n * pitch, np.uint32)), ab.put(np.zeros(L, np.uint32))
    carry_in = np.asarray([I64_MAX, L + 40, 0], np.int64)  # (none; one that bounds the last cells; one that zeroes its plane)

    def run(wrap):
        d_carry, d_next = ab.put(carry_in), ab.put(np.full(n, I64_MAX, np.int64))
        wrap(lambda: ab.check(lib.memo_lengths_begin_dev(d_cells, L, pitch, n, cap, 0, d_carry, 0, None)), {0})
        wrap(lambda: ab.check(lib.memo_lengths_rows_dev(*cols, 5000, 0, L, pitch, n, cap, d_cells, 0, None)), {1})
        wrap(lambda: ab.check(lib.memo_lengths_carry_dev(*cols, 5000, -5, L + 70, n, d_next, 0, None)), {2})
        wrap(lambda: ab.check(lib.memo_lengths_finish_dev(d_cells, L, pitch, n, cap, 0, None)), {3, 4, 5})
        wrap(lambda: ab.check(lib.memo_lengths_select_dev(d_cells, L, pitch, n, cap, T, d_out, 0, None)), {6})
        return ab.get(d_cells, n * pitch, np.uint32).reshape(n, pitch)[:, :L], ab.get(d_out, L, np.uint32), ab.get(d_next, n, np.int64)

    plain = run(lambda call, touched: call())
    timed = run(lambda call, touched: timed_call(lib, "lengths", call, touched))
    for p, t in zip(plain, timed):
        assert np.array_equal(p, t)
    assert (plain[0][2] == 0).all() and (plain[2] != I64_MAX).all()


def test_mems_timed(ab):
    lib, cap, planes = ab.lib, 500, 3
    L = lib.memo_mems_tile() + 101
    pitch = (L + 3) // 4 * 4
    rng = np.random.default_rng(3)
    cells = np.minimum(np.repeat(rng.integers(0, 2 * cap, (planes, pitch // 5 + 1)), 5, axis=1)[:, :pitch], cap).astype(np.uint32)
    d_cells = ab.put(cells)

    def run():
        counts, d_s, d_l = np.zeros(planes, np.uint64), C.c_void_p(), C.c_void_p()
        ab.check(lib.memo_mems_dev(d_cells, L, pitch, planes, cap, 20, 1, 0, C.byref(d_s), C.byref(d_l), counts.ctypes.data, 0, None))
        ab.held += [d_s, d_l]
        total = int(counts.sum())
        return counts, ab.get(d_s, total, np.uint32), ab.get(d_l, total, np.uint32)

    plain = run()
    timed = timed_call(lib, "mems", run, {0, 1, 2})
    for p, t in zip(plain, timed):
        assert np.array_equal(p, t)
    assert (plain[0] > 0).all()


def test_spectrum_timed(ab):
    lib, n, kmax = ab.lib, 3, 31
    L = lib.memo_spectrum_tile(n, kmax, 1) + 77
    pitch = (L + 3) // 4 * 4
    cells = np.random.default_rng(4).integers(0, kmax + 5, (n, pitch)).astype(np.uint32)
    d_cells = ab.put(cells)
    d_scratch = ab.put(np.zeros(lib.memo_spectrum_scratch_bytes(n, kmax) // 8, np.uint64))
    d_exact = ab.put(np.zeros((n + 1) * kmax, np.uint64))

    def run(wrap):
        wrap(lambda: ab.check(lib.memo_spectrum_begin_dev(d_scratch, n, kmax, 0, None)), set())
        wrap(lambda: ab.check(lib.memo_spectrum_add_dev(d_cells, L, pitch, n, kmax, 1, d_scratch, 0, None)), {0})
        wrap(lambda: ab.check(lib.memo_spectrum_finish_dev(d_scratch, n, kmax, d_exact, 0, None)), {1})
        return ab.get(d_exact, (n + 1) * kmax, np.uint64)

    plain = run(lambda call, touched: call())
    timed = run(lambda call, touched: timed_call(lib, "spectrum", call, touched))
    assert np.array_equal(plain, timed) and plain.sum() == L * kmax


def bits_case(ab, seed, tile_of, n=40):
    L = tile_of((n + 31) // 32) + 77
    bits, W = some_bits(np.random.default_rng(seed), L, n)
    return ab.put(bits), L, n


def test_collect_timed(ab):
    lib = ab.lib
    d_bits, L, n = bits_case(ab, 5, lib.memo_collect_tile)
    orders = np.asarray([[0, 3, 39, 7], [5, 5, 1, 0], [38, 2, 9, 30]], np.uint16)

    def run():
        d_core, d_covered = ab.put(np.zeros(orders.size, np.uint64)), ab.put(np.zeros(orders.size, np.uint64))
        ab.check(lib.memo_collect_dev(d_bits, L, n, orders.ctypes.data, 3, 4, d_core, d_covered, 0, None))
        return ab.get(d_core, orders.size, np.uint64), ab.get(d_covered, orders.size, np.uint64)

    plain = run()
    timed = timed_call(lib, "collect", run, {0, 1})
    assert np.array_equal(plain[0], timed[0]) and np.array_equal(plain[1], timed[1])
    assert plain[1].max() > 0


def test_cooc_timed(ab):
    lib = ab.lib
    d_bits, L, n = bits_case(ab, 6, lib.memo_cooccurrence_tile)

    def run():
        d_counts = ab.put(np.zeros(n * n, np.uint64))
        ab.check(lib.memo_cooccurrence_dev(d_bits, L, n, d_counts, 0, None))
        return ab.get(d_counts, n * n, np.uint64)

    plain = run()
    timed = timed_call(lib, "cooc", run, {0, 1})          # (the product's way: partials and a reduce launch)
    assert np.array_equal(plain, timed) and plain.max() > 0


def test_tracks_timed(ab):
    lib = ab.lib
    d_bits, L, n = bits_case(ab, 7, lib.memo_tracks_tile)
    edges = np.asarray([0, L // 3, L // 3, L], np.int64)

    def run():
        d_counts = ab.put(np.zeros(n * 3, np.uint64))
        ab.check(lib.memo_tracks_dev(d_bits, L, n, 0, edges.ctypes.data, 3, d_counts, 0, None))
        return ab.get(d_counts, n * 3, np.uint64)

    plain = run()
    timed = timed_call(lib, "tracks", run, {0})
    assert np.array_equal(plain, timed) and plain.max() > 0


# ---------------------------------------------------------------------------------------
# (b) begin + finish on one plane of the test's own cells
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (1, 3, CELL_TILE - 1, CELL_TILE, CELL_TILE + 1, 2 * CELL_TILE + 5))
def test_maxk_finish_on_one_plane_between_guard_words(ab, L):
    lib, cap = ab.lib, 700
    assert lib.memo_maxk_tile() == CELL_TILE
    ident = L - 1 + cap
    # begin: the identity in [0, L) and nothing else
    d = ab.put(np.full(L + 12, PAD, np.uint32))
    ab.check(lib.memo_maxk_begin_dev(d + 16, L, cap, 0, None))
    got = ab.get(d, L + 12, np.uint32)
    assert (got[4:4 + L] == ident).all() and (got[:4] == PAD).all() and (got[4 + L:] == PAD).all()
    # finish: out[i] = min(cap, max(0, min(cell[i ..]) - i)) over cells as a row pass leaves them -- bounds in [0, ident], most at ident
    rng = np.random.default_rng(L)
    cells = np.full(L, ident, np.int64)
    hit = rng.random(L) < 0.02
    cells[hit] = rng.integers(0, ident + 1, int(hit.sum()))
    cells[-1] = min(ident, L + 3)                          # (the last tile's minimum reaches every tile left of it)
    want = np.minimum.accumulate(cells[::-1])[::-1] - np.arange(L)
    want = np.minimum(np.maximum(want, 0), cap).astype(np.uint32)
    whole = np.full(L + 12, PAD, np.uint32)
    whole[4:4 + L] = cells
    d = ab.put(whole)
    ab.check(lib.memo_maxk_finish_dev(d + 16, L, cap, 0, None))
    got = ab.get(d, L + 12, np.uint32)
    assert np.array_equal(got[4:4 + L], want), L
    assert (got[:4] == PAD).all() and (got[4 + L:] == PAD).all(), L
