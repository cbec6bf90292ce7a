"""`memo breaks` on the GPU: the kernel (memo_amd/csrc/memo_breaks.hip) against NumPy on the host, the window and BED routes against
the oracle and, independently of it, against `memo mems` and `memo lengths`; the command line against the README's tables.

The oracle is tests/breaks_oracle.py; every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import breaks_oracle as O
from tests import golden_util as G
from tests import mems_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
CAP = 4                                                         # values of [0, 4]: ties and runs at the cap are common
MEMB, CONS = os.path.join(G.GOLD, "example_memb.parquet"), os.path.join(G.GOLD, "example_cons.parquet")
GRID_X = 1024                                                   # runs of tiles a plane at most (memo_breaks.hip: kMaxGridX)
LANE, WAVE = 4, 256                                             # cells a lane and a wave own of a tile


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture(scope="module")
def Tt(memo):
    from memo_amd import breaks
    t = breaks.tile()
    assert t == LANE * WAVE and t % WAVE == 0
    return t


def resident(cells):
    """(DevBuffer, the tuple plane_breaks takes) of host cells [planes, L], padded to the pitch and uploaded once"""
    from memo_amd._device import DevBuffer
    from memo_amd.lengths import pitch_of
    cells = np.asarray(cells, np.uint32)
    planes, L = cells.shape
    padded = np.full((planes, pitch_of(L)), 0xFFFFFFFF, np.uint32)           # (what lies behind L is never read: it would show)
    padded[:, :L] = cells
    buf = DevBuffer.of(padded, 0)
    return buf, (buf.d.value, L, pitch_of(L), planes)


def same(got, want, note=None):
    assert got.dtype == np.uint64 and got.shape == want.shape, (note, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (note, bad[:5].tolist(), [int(got[tuple(i)]) for i in bad[:5]], [int(want[tuple(i)]) for i in bad[:5]])


def draw(rng, planes, cells):
    """values of [0, CAP] with what the rule can meet planted where the length allows: a start at a lane's and at a wave's first cell,
    and behind cell 8 a rise, a tie below the cap, a tie at the cap, a fall and a zero"""
    v = rng.integers(0, CAP + 1, (planes, cells)).astype(np.uint32)
    for at in (LANE, 2 * LANE, WAVE, 3 * WAVE):
        if at < cells:
            v[0, at - 1], v[0, at] = 0, CAP
    if cells >= 16:
        v[0, 9:16] = [1, 2, 2, CAP, CAP, 3, 0]
    return v


def branches(v, halo):
    """which branches of the rule the cells of one input hold, on the oracle's side"""
    w = v.astype(np.int64)
    prev, cur = w[:, :-1], w[:, 1:]
    at = np.arange(1, w.shape[1])
    start = mems_oracle.start_mask(w, CAP, CAP, halo)[:, 1:]                  # at min_len = cap: a start that every min_len keeps
    return {"rise": bool((prev < cur).any()), "tie below the cap": bool(((prev == cur) & (cur < CAP)).any()),
            "tie at the cap": bool(((prev == cur) & (cur == CAP)).any()), "fall": bool((prev > cur).any()),
            "below min_len": bool((w[:, halo:] < 2).any()), "lane's first cell": bool(start[:, at % LANE == 0].any()),
            "wave's first cell": bool(start[:, at % WAVE == 0].any())}


def bin_counts(n):
    return sorted({b for b in (1, 2, 3, 7, n - 1, n) if 1 <= b <= n})


# ---------------------------------------------------------------------------------------
# the kernel against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", (1, 2, 3, 99, 2048))
def test_the_kernel_against_the_oracle(memo, Tt, planes):
    """every counted length around a lane, a wave and a tile, every bin count, with and without a neighbour cell, min_len 1, 2 and
    the cap.  An input of at least 63 cells holds every branch of the rule, one of more than a wave a start at a wave's first cell
    too (asserted here, on the oracle's side); the shorter ones are what test_one_plane_per_branch is for."""
    from memo_amd import breaks
    rng = np.random.default_rng([20261020, planes])
    lengths = (5,) if planes == 2048 else (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, Tt - 1, Tt, Tt + 1, 2 * Tt + 1)
    calls = 0
    for n in lengths:
        for halo in (0, 1):
            v = draw(rng, planes, n + halo)
            if n >= 63:
                held = branches(v, halo)
                assert all(held[b] for b in held if b != "wave's first cell" or n > WAVE), (n, halo, held)
            buf, where = resident(v)
            with buf:
                for bins in bin_counts(n):
                    edges = np.linspace(0, n, bins + 1).astype(np.int64)
                    for min_len in (1, 2, CAP):
                        got = breaks.plane_breaks(where, edges, cap=CAP, min_len=min_len, halo=halo)
                        same(got, O.table(v, edges, CAP, min_len, halo), (planes, n, halo, bins, min_len))
                        calls += 1
    assert calls >= (3 if planes == 2048 else 400)
    # a host array goes the same way
    v = draw(rng, min(planes, 3), 2 * Tt + 3)
    same(breaks.plane_breaks(v, [0, 5, 2 * Tt + 3], cap=CAP), O.table(v, [0, 5, 2 * Tt + 3], CAP))


@pytest.mark.parametrize("halo", (0, 1))
def test_one_plane_per_branch(memo, halo):
    """hand-made planes of 8 cells, cap = 4"""
    from memo_amd import breaks
    for v in ([0, 1, 2, 3, 4, 4, 4, 4], [2, 2, 2, 2, 2, 2, 2, 2], [4, 4, 4, 4, 4, 4, 4, 4], [4, 3, 2, 1, 0, 0, 0, 0], [3, 2, 3, 2, 3, 2, 3, 2],
              [1, 1, 2, 2, 3, 3, 4, 4], [0, 3, 0, 3, 0, 3, 0, 3], [0, 0, 0, 0, 0, 0, 0, 0], [4, 4, 4, 0, 4, 4, 4, 4], [1, 2, 3, 4, 4, 4, 0, 9]):
        n = 8 - halo
        for min_len in (1, 2, 3, 4):
            for edges in ([0, n], [0, 4, n], list(range(n + 1))):
                got = breaks.plane_breaks(np.array([v], np.uint32), edges, cap=4, min_len=min_len, halo=halo)
                same(got, O.naive([v], edges, 4, min_len, halo), (v, halo, min_len, edges))
    one = lambda v, **kw: int(breaks.plane_breaks(np.array([v], np.uint32), [0, 8 - kw.get("halo", 0)], cap=4, **kw)[0, 0, 0])     # noqa: E731
    assert one([0, 1, 2, 3, 4, 4, 4, 4]) == 4 and one([2] * 8) == 8 and one([4] * 8) == 1 and one([4] * 8, halo=1) == 0
    assert one([4, 3, 2, 1, 0, 0, 0, 0]) == 1 and one([3, 2, 3, 2, 3, 2, 3, 2], min_len=3) == 4 and one([1, 1, 2, 2, 3, 3, 4, 4], min_len=2) == 5


# ---------------------------------------------------------------------------------------
# edges where the walk can go wrong
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", (0, 1))
def test_edges_on_and_beside_every_boundary(memo, Tt, halo):
    from memo_amd import breaks
    rng = np.random.default_rng([7, halo])
    n = 2 * Tt + 9
    v = draw(rng, 3, n + halo)
    buf, where = resident(v)
    bounds = [LANE, WAVE, WAVE + LANE, Tt, Tt + LANE, Tt + WAVE, 2 * Tt]      # a lane's, a wave's and a tile's first cell
    beside = sorted({b + d for b in bounds for d in (-2, -1, 0, 1, 2)})       # (with a neighbour cell the cells lie one further right)
    first = 1000
    lists = [[0] + beside + [n]]
    lists += [[0, x, n] for x in beside]                                      # one edge alone: a head, a flush, a tail
    lists += [[0, x, x + 1, n] for x in beside]                               # a bin of one cell at the boundary
    lists += [[0, 8, 9, 9, 10, 11, n],                                        # five edges inside one lane's four cells
              [0, Tt + 4, Tt + 5, Tt + 5, Tt + 6, Tt + 7, n],
              [0, 0, 0, 5, n], [0, 700, 700, 700, 701, n], [0, Tt, Tt, n], [0, 5, n, n, n], [0, 0, n, n],      # empty bins: front, middle, end
              [-first, -3, 0, 5, n + 1, n + 7],                               # edges that begin before `first` and end behind the slice
              [-first, n + 10 ** 6], [-5, -5, -1, 3, 3, n - 1, n + 2, n + 2]]
    with buf:
        for cut in lists:
            edges = np.asarray(cut, np.int64) + first
            for min_len in (1, CAP):
                got = breaks.plane_breaks(where, edges, first=first, cap=CAP, min_len=min_len, halo=halo)
                same(got, O.table(v, edges, CAP, min_len, halo, first), (halo, cut, min_len))
        # every position its own bin, and every second one empty
        for edges in (np.arange(n + 1), np.repeat(np.arange(n + 1), 2)):
            same(breaks.plane_breaks(where, edges, cap=CAP, halo=halo), O.table(v, edges, CAP, 1, halo), len(edges))


def test_a_workgroup_with_many_tiles_and_a_ragged_tail(memo, Tt):
    from memo_amd import breaks
    rng = np.random.default_rng(11)
    L = 2 * GRID_X * Tt + 5                                                   # two tiles a workgroup, and the last one of five cells
    v = rng.integers(0, CAP + 1, (2, L)).astype(np.uint32)
    buf, where = resident(v)
    with buf:
        for halo, edges in ((0, [0, L]), (1, [0, L - 1]), (0, [0, Tt + 3, L - 2, L]), (1, [0, 2 * Tt, 2 * Tt + 1, L - 1]),
                            (0, np.append(np.arange(0, L, 16), L)), (1, np.append(np.arange(0, L - 1, 16), L - 1))):
            edges = np.asarray(edges, np.int64)
            got = breaks.plane_breaks(where, edges, cap=CAP, min_len=2, halo=halo)
            same(got, O.table(v, edges, CAP, 2, halo), (halo, len(edges)))
    assert len(np.arange(0, L, 16)) > 2 ** 17


# ---------------------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------------------
def test_the_table_is_added_to_and_slices_accumulate(memo, Tt):
    from memo_amd import breaks
    rng = np.random.default_rng(13)
    n = Tt + 40
    for halo0 in (0, 1):                                                      # the window begins its record, or has a left neighbour
        v = draw(rng, 3, n + halo0)
        edges = np.asarray(sorted(rng.integers(0, n + 1, 9).tolist() + [0, n]), np.int64) + 50
        want = O.table(v, edges, CAP, 2, halo0, 50)
        before = rng.integers(0, 2 ** 63, want.shape, dtype=np.int64).astype(np.uint64) * np.uint64(2)      # (wraps: the adds are modulo 2^64)
        same(breaks.plane_breaks(v, edges, first=50, cap=CAP, min_len=2, halo=halo0, table=before), before + want, halo0)
        for step in (1, 3, 7, Tt + 1):
            m = 130 if step == 1 else n                                       # (a call a cell: a shorter window)
            cut = np.minimum(edges, 50 + m)
            table = before.copy()
            for a in range(0, m, step)[::-1]:                                 # from the right, as the slices of `memo lengths` come
                h = halo0 if a == 0 else 1
                part = v[:, a + halo0 - h:min(a + step, m) + halo0]           # its left neighbour is its cell 0
                table = breaks.plane_breaks(part, cut, first=50 + a, cap=CAP, min_len=2, halo=h, table=table)
            same(table, before + O.table(v[:, :m + halo0], cut, CAP, 2, halo0, 50), (halo0, step))


def test_far_coordinates(memo, Tt):
    """`first` and the edges past 2^32 at the ABI"""
    from memo_amd import breaks
    rng = np.random.default_rng(17)
    n = Tt + 77
    v = draw(rng, 2, n + 1)
    for first in (2 ** 32 + 12345, 2 ** 40 + 1, 2 ** 61):
        edges = np.asarray(sorted(rng.integers(0, n + 1, 12).tolist() + [-2 ** 31, n + 2 ** 31]), np.int64) + first
        same(breaks.plane_breaks(v, edges, first=first, cap=CAP, halo=1), O.table(v, edges, CAP, 1, 1, first), first)


# ---------------------------------------------------------------------------------------
# what is refused, and what launches nothing
# ---------------------------------------------------------------------------------------
def test_refusals_leave_the_table_as_it_was(memo):
    from memo_amd import _lib
    from memo_amd._device import DevBuffer
    L_ = _lib.lib()
    v = np.arange(64, dtype=np.uint32).reshape(2, 32) % 5
    before = np.arange(2 * 2 * 3, dtype=np.uint64).reshape(2, 2, 3) + np.uint64(7)
    edges = np.array([0, 10, 20, 32], np.int64)
    down = np.array([0, 20, 10, 32], np.int64)
    big = 2 ** 31
    with DevBuffer.of(v, 0) as cells, DevBuffer.of(before, 0) as table:
        d, t, e = cells.d.value, table.d.value, edges.ctypes.data
        ok = dict(d=d, L=32, pitch=32, planes=2, cap=4, min_len=1, halo=0, first=0, e=e, bins=3, t=t)

        def call(**kw):
            a = dict(ok, **kw)
            return L_.memo_breaks_dev(a["d"], a["L"], a["pitch"], a["planes"], a["cap"], a["min_len"], a["halo"], a["first"], a["e"], a["bins"],
                                      a["t"], 0, None)
        refused = (dict(d=d + 4), dict(d=d + 8), dict(d=None), dict(pitch=34, L=30), dict(pitch=28), dict(L=big + 1, pitch=big + 4), dict(L=-1),
                   dict(planes=-1), dict(planes=2049), dict(bins=0), dict(bins=-3), dict(bins=2 ** 20 + 2), dict(cap=0), dict(cap=2 ** 31),
                   dict(min_len=0), dict(min_len=5), dict(halo=2), dict(halo=-1), dict(e=down.ctypes.data), dict(e=None),
                   dict(first=-1), dict(first=1), dict(first=33), dict(halo=1, first=2), dict(L=0, first=40), dict(t=None), dict(t=t + 4))
        for kw in refused:
            assert call(**kw) == _lib.MEMO_EINVAL, kw
            assert L_.memo_last_error(), kw
            assert np.array_equal(table.to_host(before.shape, np.uint64), before), kw
        # nothing to count: nothing is launched, the table stays
        for kw in (dict(L=0), dict(L=1, halo=1), dict(L=0, halo=1), dict(planes=0), dict(L=0, d=None, pitch=0), dict(planes=0, d=None)):
            assert call(**kw) == _lib.MEMO_OK, kw
            assert np.array_equal(table.to_host(before.shape, np.uint64), before), kw
        # and the call as it stands is taken
        assert call() == _lib.MEMO_OK
        same(table.to_host(before.shape, np.uint64), before + O.table(v, edges, 4), "taken")
        assert call(halo=1, first=1) == _lib.MEMO_OK and call(halo=1, first=0, L=31) == _lib.MEMO_OK and call(pitch=36, L=30, planes=1) == _lib.MEMO_OK


def test_the_lap_timer_is_the_ab_library_s(memo):
    from memo_amd import _lib, breaks
    assert not hasattr(_lib.lib(), "memo_debug_breaks_times")
    ab = _lib.use_ab(True)
    try:
        ms = (C.c_float * 1)()
        assert ab.memo_debug_breaks_times(1, ms) == 0
        v = np.ones((2, 5000), np.uint32)
        assert breaks.plane_breaks(v, [0, 5000], cap=4)[:, :, 0].tolist() == [[5000, 5000], [5000, 5000]]
        assert ab.memo_debug_breaks_times(0, ms) == 0 and ms[0] > 0.0
    finally:
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# region_breaks
# ---------------------------------------------------------------------------------------
N_SYNTH = 6


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """a Parquet index of two records and several row groups, random rows with end >= start for six genomes: read with -m it is a
    membership index, read without it a conservation index (nothing in a file tells them apart)"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(23)
    cols = {}
    for rec, rows in (("recA", 900), ("recB", 500)):
        s = np.sort(rng.integers(1, 2600, rows))
        cols[rec] = (s, s + rng.integers(0, 40, rows), rng.integers(1, N_SYNTH, rows))
    path = str(tmp_path_factory.mktemp("breaks") / "synth.parquet")
    names = sum(([rec] * len(c[0]) for rec, c in cols.items()), [])
    table = pa.table({"f0": pa.array(names, pa.utf8()), **{f"f{i + 1}": np.concatenate([c[i] for c in cols.values()]) for i in range(3)}})
    pq.write_table(table, path, row_group_size=211)
    return path, cols


def _edges(qs, qe, bins):
    from memo_amd import tracks
    return tracks.region_edges(qe - qs, bins)


def _independent(path, region, n, edges, qs, min_len, cap, threshold=None):
    """the same table without any oracle: a histogram of `memo mems`' starts, and `memo lengths` / `memo maxk` reduced per bin"""
    from memo_amd import lengths, maxk, mems
    cut = np.asarray(edges, np.int64)
    if threshold is None:
        m = mems.region_mems(path, region, n, membership=True, all_genomes=True, min_len=min_len, cap=cap)
        starts = np.stack([np.zeros(len(cut) - 1, np.int64)] + [np.histogram(m.starts[m.genome == g] - qs, cut)[0] for g in range(1, n)])
        values = lengths.region_planes(path, region, n, cap)
        pivot = mems.region_mems(path, region, n, membership=True, genome=0, min_len=min_len, cap=cap)      # (-a leaves the pivot out)
        starts[0] = np.histogram(pivot.starts - qs, cut)[0]
    else:
        m = mems.region_mems(path, region, n, threshold=threshold, min_len=min_len, cap=cap)
        starts = np.histogram(m.starts - qs, cut)[0][None, :]
        values = maxk.region_maxk(path, region, n, threshold=threshold, cap=cap)[None, :]
    sums = np.add.reduceat(values.astype(np.uint64), cut[:-1], axis=1)                                       # (no bin is empty)
    return np.stack([starts.astype(np.uint64), sums])


def _check_region(path, cols, rec, qs, qe, n, bins, min_len, cap, threshold=None, steps=(None,)):
    from memo_amd import breaks
    region = f"{rec}:{qs}-{qe}"
    edges = _edges(qs, qe, bins)
    want = O.window_table(*cols, qs, qe, edges + qs, cap, n, min_len=min_len, threshold=threshold)
    kw = dict(membership=threshold is None, threshold=threshold, min_len=min_len, cap=None if cap == CAP_MAX else cap)
    for step in steps:
        table, got_edges, got_qs = breaks.region_breaks(path, region, n, bins, slice_positions=step, **kw)
        assert got_qs == qs and np.array_equal(got_edges, edges) and got_edges.dtype == np.int64
        same(table, want, (region, bins, min_len, cap, threshold, step))
    same(_independent(path, region, n, edges, qs, min_len, cap, threshold), want, ("independent", region, bins, min_len, cap, threshold))
    return want


def test_region_breaks_on_the_goldens(memo):
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    cons = G.index_columns("example_cons.parquet", "ref_1")
    for qs, qe in ((0, 20), (7, 19)):
        for bins in (1, 4, qe - qs):
            for min_len, cap in ((1, CAP_MAX), (3, CAP_MAX), (2, 3))[::1 if bins == 4 else 2]:
                want = _check_region(MEMB, (s, e, a), "ref_1", qs, qe, 5, bins, min_len, cap, steps=(None, 1, 3, 7, 1000))
                assert (want[1, 0] == np.diff(_edges(qs, qe, bins)).astype(np.uint64) * np.uint64(cap)).all()       # nothing bounds the pivot
                for t in (5, 3):
                    _check_region(CONS, cons, "ref_1", qs, qe, 5, bins, min_len, cap, threshold=t)
    from memo_amd import breaks
    table, edges, qs = breaks.region_breaks(MEMB, "ref_1:0-20", 5, 4, membership=True)
    assert table[0].tolist() == [[1, 0, 0, 0], [3, 2, 2, 3], [2, 1, 2, 1], [2, 4, 2, 3], [3, 3, 3, 3]] and edges.tolist() == [0, 5, 10, 15, 20]
    assert table[1, 1:].tolist() == [[13, 13, 14, 12], [18, 30, 14, 20], [21, 25, 17, 20], [15, 17, 16, 16]]
    assert breaks.region_breaks(CONS, "ref_1:0-20", 5, 4)[0][0].tolist() == [[3, 3, 3, 3]]
    assert breaks.region_breaks(MEMB, "ref_1:5-5", 5, 4, membership=True)[0].shape == (2, 5, 0)
    with pytest.raises(OSError):
        breaks.region_breaks(os.path.join(G.GOLD, "no_such.parquet"), "ref_1:0-20", 5, 4)


def test_region_breaks_on_a_synthetic_index(memo, Tt, synth):
    path, cols = synth
    for rec, qs, qe in (("recA", 0, 2 * Tt + 70), ("recA", 301, Tt + 300), ("recB", 1, 700)):
        for bins, min_len, cap in ((1, 1, CAP_MAX), (7, 2, 31), (qe - qs, 5, 5)):
            _check_region(path, cols[rec], rec, qs, qe, N_SYNTH, bins, min_len, cap, steps=(None, Tt + 1, 10 ** 6))
            for t in (N_SYNTH, 3):
                _check_region(path, cols[rec], rec, qs, qe, N_SYNTH, bins, min_len, cap, threshold=t)
    for qs, qe in ((0, 33), (40, 75)):                                        # (short: a slice of 1 reads the file once per position)
        _check_region(path, cols["recB"], "recB", qs, qe, N_SYNTH, 5, 2, 9, steps=(1, 3, 7))


# ---------------------------------------------------------------------------------------
# bed_breaks
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("membership", (True, False))
def test_every_feature_is_its_own_window_with_one_bin(memo, synth, membership):
    """overlapping, nested, repeated, empty and unsorted features on two records"""
    from memo_amd import breaks, features
    path, _ = synth
    rows = [("recA", 500, 900), ("recB", 10, 60), ("recA", 100, 700), ("recA", 300, 310), ("recA", 300, 310), ("recB", 0, 400), ("recA", 650, 650),
            ("recA", 0, 1), ("recB", 399, 400), ("recA", 899, 1500), ("recB", 60, 61), ("recC", 5, 5), ("recA", 100, 700), ("recB", 200, 380)]
    bed = features.Bed([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [f"f{i}" for i in range(len(rows))])
    threshold = None if membership else 3
    R = N_SYNTH if membership else 1
    want = np.zeros((2, len(rows), R), np.uint64)
    for f, (rec, a, b) in enumerate(rows):
        if b > a:
            one, edges, qs = breaks.region_breaks(path, f"{rec}:{a}-{b}", N_SYNTH, 1, membership=membership, threshold=threshold, min_len=2, cap=31)
            assert one.shape == (2, R, 1) and edges.tolist() == [0, b - a] and qs == a
            want[:, f, :] = one[:, :, 0]
    assert want[0].any() and want[1].any()
    for most in (None, 1, 2):
        table, positions = breaks.bed_breaks(path, bed, N_SYNTH, membership=membership, threshold=threshold, min_len=2, cap=31, batch_features=most)
        assert positions.tolist() == [b - a for _, a, b in rows]
        same(table, want, (membership, most))
    same(breaks.bed_breaks(path, bed, N_SYNTH, membership=membership, threshold=threshold, min_len=2, cap=31, slice_positions=97)[0], want, "sliced")
    table, positions = breaks.bed_breaks(path, features.Bed([], [], [], []), N_SYNTH, membership=membership)
    assert table.shape == (2, 0, R) and positions.shape == (0,)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


HEAD = "genome\t0-5\t5-10\t10-15\t15-20\n"
README_STARTS = HEAD + "0\t1\t0\t0\t0\n1\t3\t2\t2\t3\n2\t2\t1\t2\t1\n3\t2\t4\t2\t3\n4\t3\t3\t3\t3\n"
README_SUMS = HEAD + ("0\t10737418235\t10737418235\t10737418235\t10737418235\n1\t13\t13\t14\t12\n2\t18\t30\t14\t20\n3\t21\t25\t17\t20\n"
                      "4\t15\t17\t16\t16\n")
README_L3 = HEAD + "0\t1\t0\t0\t0\n1\t3\t1\t2\t2\n2\t2\t1\t2\t1\n3\t2\t4\t2\t3\n4\t3\t3\t3\t3\n"
EXAMPLE_BED = "# three features\nref_1\t0\t10\ta\nref_1\t5\t20\tb\t0\t+\nref_1\t15\t15\tc\n"


def _run(tmp_path, index, *flags, region=("-r", "ref_1:0-20", "-B", "4")):
    out = str(tmp_path / "b.tsv")
    r = _memo("breaks", "-b", index, "-n", "5", *region, "-o", out, *flags)
    assert (r.returncode, r.stdout) == (0, b"MEMO - breaks\n"), (flags, r.stderr)
    return open(out).read()


def test_cli_writes_the_readme_s_tables(memo, tmp_path):
    assert _run(tmp_path, MEMB, "-m") == README_STARTS
    assert _run(tmp_path, MEMB, "-m", "-s") == README_SUMS
    assert _run(tmp_path, MEMB, "-m", "-l", "3") == README_L3
    assert _run(tmp_path, MEMB, "-m", region=("-r", "ref_1:5-5")) == ""                       # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["b.tsv"]                                           # written beside its name and renamed


def test_cli_thresholds_means_and_labels(memo, tmp_path):
    assert _run(tmp_path, CONS) == HEAD + ">=5\t3\t3\t3\t3\n"                                # -t defaults to -n
    assert _run(tmp_path, CONS, "-t", "3", "-s") == HEAD + ">=3\t19\t24\t16\t19\n"
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    text = _run(tmp_path, MEMB, "-m", "-s", "-f", "-K", "9", "-g", str(genomes))
    assert [ln.split("\t")[0] for ln in text.splitlines()] == ["genome", "pivot", "g1", "g2", "g3", "g4"]
    assert text.splitlines()[1:3] == ["pivot\t9.0\t9.0\t9.0\t9.0", "g1\t2.6\t2.6\t2.8\t2.4"]
    never = str(tmp_path / "never.tsv")
    r = _memo("breaks", "-b", MEMB, "-n", "5", "-r", "ref_1:0-20", "-o", never, "-m")         # -B 500: more bins than positions
    assert r.returncode == 1 and b"500 bins for a window of 20 positions" in r.stderr and not os.path.exists(never)
    assert sorted(os.listdir(tmp_path)) == ["b.tsv", "genomes.txt"]


def test_cli_on_a_bed_file(memo, tmp_path):
    """the README's genes.bed"""
    from memo_amd import breaks, features
    bed_path = tmp_path / "genes.bed"
    bed_path.write_text(EXAMPLE_BED)
    region = ("-a", str(bed_path))
    head = "chrom\tstart\tend\tname\tpositions\t"
    assert _run(tmp_path, MEMB, "-m", region=region) == (head + "0\t1\t2\t3\t4\n"
                                                         "ref_1\t0\t10\ta\t10\t1\t5\t3\t6\t6\n"
                                                         "ref_1\t5\t20\tb\t15\t0\t7\t4\t9\t9\n"
                                                         "ref_1\t15\t15\tc\t0\t0\t0\t0\t0\t0\n")
    assert _run(tmp_path, CONS, region=region) == head + "starts\nref_1\t0\t10\ta\t10\t6\nref_1\t5\t20\tb\t15\t9\nref_1\t15\t15\tc\t0\t0\n"
    assert _run(tmp_path, CONS, "-s", "-f", region=region) == head + "sum\nref_1\t0\t10\ta\t10\t2.5\nref_1\t5\t20\tb\t15\t2.466666666666667\nref_1\t15\t15\tc\t0\tnan\n"
    assert sorted(os.listdir(tmp_path)) == ["b.tsv", "genes.bed"]
    table, positions = breaks.bed_breaks(MEMB, features.read_bed(str(bed_path)), 5, membership=True, cap=9)     # (the -s -K 9 table, in process)
    assert table[1].tolist() == [[90, 26, 48, 46, 32], [135, 39, 64, 62, 49], [0, 0, 0, 0, 0]] and positions.tolist() == [10, 15, 0]
