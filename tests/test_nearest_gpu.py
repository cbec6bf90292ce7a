"""`memo nearest` on the GPU: the kernel (memo_amd/csrc/memo_nearest.hip) against NumPy on the host, the window routes against the
oracle and, independently of it, against `memo tracks` and `memo lengths`; the command line against the README's tables.

The oracle is tests/nearest_oracle.py; every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import nearest_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
CAP = 4                                                         # values of [0, 4]: ties, all-zero and all-at-cap columns are common
MEMB = os.path.join(G.GOLD, "example_memb.parquet")
RND40 = os.path.join(G.GOLD, "rnd_n40.parquet")
TILES = {2: 256, 3: 256, 5: 256, 67: 256, 68: 128, 99: 128, 109: 128, 110: 64, 150: 64, 200: 64, 216: 64, 217: 32, 300: 32, 415: 32, 416: 16, 600: 16,
         763: 16, 764: 8, 1300: 8, 2048: 8}                      # positions per tile: every plane count at which it changes


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def resident(cells):
    """(DevBuffer, the tuple plane_nearest takes) of host cells [planes, L], padded to the pitch and uploaded once"""
    from memo_amd._device import DevBuffer
    from memo_amd.lengths import pitch_of
    cells = np.asarray(cells, np.uint32)
    planes, L = cells.shape
    padded = np.full((planes, pitch_of(L)), 0xFFFFFFFF, np.uint32)           # (what lies behind L is never read: it would show)
    padded[:, :L] = cells
    buf = DevBuffer.of(padded, 0)
    return buf, (buf.d.value, L, pitch_of(L), planes)


def same(got, want, note=None):
    assert got.dtype == want.dtype and got.shape == want.shape, (note, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (note, bad[:5].tolist(), [int(got[tuple(i)]) for i in bad[:5]], [int(want[tuple(i)]) for i in bad[:5]])


def check(where, v, edges, cap, min_len=1, candidates=None, first=0, note=None):
    """all three outputs of one call against the oracle"""
    from memo_amd import nearest
    wins, sums, winner = nearest.plane_nearest(where, edges, cap=cap, min_len=min_len, candidates=candidates, first=first, winner=True)
    want_wins, want_sums = O.table(v, edges, cap, min_len, candidates, first)
    note = (note, v.shape, len(edges) - 1, min_len, candidates if candidates is None or len(candidates) < 9 else len(candidates))
    same(wins, want_wins, note), same(sums, want_sums, note), same(winner, O.winners(v, cap, min_len, candidates), note)
    return want_wins


def draw(rng, planes, cells):
    """values of [0, CAP]; where the length allows: column 0 all zero, column 1 all at the cap, column 2 a tie of two genomes (one genome:
    a sole win), and a cell above the cap"""
    v = rng.integers(0, CAP + 1, (planes, cells)).astype(np.uint32)
    if cells >= 3:
        v[:, 0], v[:, 1] = 0, CAP
        v[1:, 2] = rng.integers(0, CAP - 1, planes - 1)
        v[[1, planes - 1], 2] = CAP - 1
        v[1 + (cells % (planes - 1)), 1] = CAP + 5
    return v


def held(v):
    """what the columns of one input hold, on the oracle's side"""
    best, ok, att, sole, _ = O.per_position(v, CAP)
    c = np.minimum(v[1:].astype(np.int64), CAP)
    return {"a tie": bool((att.sum(axis=0) > 1).any()), "all zero": bool((c.max(axis=0) == 0).any()), "all at the cap": bool((c.min(axis=0) == CAP).any()),
            "above the cap": bool((v[1:] > CAP).any())}


def bin_counts(n):
    return sorted({b for b in (1, 2, 3, 7, n - 1, n) if 1 <= b <= n})


# ---------------------------------------------------------------------------------------
# the kernel against the oracle
# ---------------------------------------------------------------------------------------
def test_the_tile_and_the_run_rule(memo):
    from memo_amd import nearest
    assert {n: nearest.tile(n) for n in TILES} == TILES
    assert nearest.tile(1) == 0 and nearest.tile(2049) == 0
    assert nearest.tiles_per_run(1, 3) == 1 and nearest.tiles_per_run(1024 * 256, 3) == 1 and nearest.tiles_per_run(1024 * 256 + 1, 3) == 2


@pytest.mark.parametrize("planes", (2, 3, 5, 99, 150, 300, 600, 2048))
def test_the_kernel_against_the_oracle(memo, planes):
    """every length around a wave and a tile, every bin count, min_len 1, 2 and the cap, all outputs at once.  An input of at least 3
    positions holds an all-zero column, a column at the cap, a tie and a cell above the cap (asserted on the oracle's side)."""
    from memo_amd import nearest
    rng = np.random.default_rng([20261021, planes])
    T = nearest.tile(planes)
    assert T == TILES[planes]
    if planes in (2, 3, 5, 99):
        lengths = sorted({1, 2, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1})
    else:
        lengths = sorted({5, T - 1, T, T + 1, 2 * T + 1})
    calls = 0
    for n in lengths:
        v = draw(rng, planes, n)
        if n >= 3:
            what = held(v)
            assert all(what[k] for k in what if k != "a tie" or planes > 2), (n, what)
        buf, where = resident(v)
        with buf:
            for bins in bin_counts(n) if planes <= 99 else (1, 3, n):
                edges = np.linspace(0, n, bins + 1).astype(np.int64)
                for min_len in (1, 2, CAP):
                    check(where, v, edges, CAP, min_len)
                    calls += 1
    assert calls >= (150 if planes <= 99 else 40)
    # a host array goes the same way
    v = draw(rng, planes, T + 3)
    check(v, v, [0, 5, T + 3], CAP)


@pytest.mark.parametrize("planes", (3, 99, 200))
def test_long_values_where_sole_winners_dominate(memo, planes):
    from memo_amd import nearest
    rng = np.random.default_rng([5, planes])
    T = nearest.tile(planes)
    for n in (5, T + 1, 2 * T + 1):
        v = rng.integers(0, 2 ** 31, (planes, n)).astype(np.uint32)
        v[1, n // 2] = 0xFFFFFFF0                                            # above every cap
        buf, where = resident(v)
        with buf:
            for bins in (1, 7 if n >= 7 else 2, n):
                edges = np.linspace(0, n, bins + 1).astype(np.int64)
                for min_len, cap in ((1, CAP_MAX), (2 ** 30, CAP_MAX), (2 ** 29, 2 ** 30)):
                    wins = check(where, v, edges, cap, min_len)
                    if cap == CAP_MAX and min_len == 1 and planes > 2:
                        assert wins[1, 1:].sum() >= n - 1 and wins[0, 0].sum() == 0                 # sole winners dominate
        assert int(O.table(v, [0, n], CAP_MAX)[1][0]) > 2 ** 32 or n * planes < 20                 # the sums need 64 bits


def test_edges_on_and_beside_every_boundary(memo):
    from memo_amd import nearest
    rng = np.random.default_rng(7)
    T = nearest.tile(3)
    n = 2 * T + 9
    v = draw(rng, 3, n)
    buf, where = resident(v)
    bounds = [64, 128, T, T + 64, 2 * T]                                      # a wave's read's and a tile's first position
    beside = sorted({b + d for b in bounds for d in (-2, -1, 0, 1, 2)})
    first = 1000
    lists = [[0] + beside + [n]]
    lists += [[0, x, n] for x in beside]                                      # one edge alone: a head, a flush, a tail
    lists += [[0, x, x + 1, n] for x in beside]                               # a bin of one position at the boundary
    lists += [[0, 8, 9, 9, 10, 11, n], [0, T + 4, T + 5, T + 5, T + 6, T + 7, n],
              [0, 0, 0, 5, n], [0, 200, 200, 200, 201, n], [0, T, T, n], [0, 5, n, n, n], [0, 0, n, n],       # empty bins: front, middle, end
              [-first, -3, 0, 5, n + 1, n + 7],                               # edges that begin before `first` and end behind the slice
              [-first, n + 10 ** 6], [-5, -5, -1, 3, 3, n - 1, n + 2, n + 2]]
    with buf:
        for cut in lists:
            check(where, v, np.asarray(cut, np.int64) + first, CAP, 1 + len(cut) % 2, first=first, note=cut[:6])
        for edges in (np.arange(n + 1), np.repeat(np.arange(n + 1), 2)):      # every position its own bin, and every second one empty
            check(where, v, edges, CAP)
    for far in (2 ** 32 + 12345, 2 ** 61):                                    # `first` and the edges past 2^32 at the ABI
        edges = np.asarray(sorted(rng.integers(0, n + 1, 12).tolist() + [-2 ** 31, n + 2 ** 31]), np.int64) + far
        check(v, v, edges, CAP, first=far)


@pytest.mark.parametrize("planes,tiles", ((3, 3), (1300, 2)))
def test_a_workgroup_with_many_tiles_and_a_ragged_tail(memo, planes, tiles):
    from memo_amd import nearest
    rng = np.random.default_rng([11, planes])
    T = nearest.tile(planes)
    L = (tiles - 1) * nearest.MAX_RUNS * T + 5                                # `tiles` tiles a workgroup, and the last tile of five positions
    assert nearest.tiles_per_run(L, planes) == tiles and nearest.tiles_per_run(L - 5, planes) == tiles - 1
    v = rng.integers(0, CAP + 1, (planes, L)).astype(np.uint32)
    buf, where = resident(v)
    with buf:
        for edges in ([0, L], [0, T + 3, L - 2, L], np.append(np.arange(0, L, 16), L), np.linspace(0, L, 501).astype(np.int64)):
            check(where, v, np.asarray(edges, np.int64), CAP, 2)
    assert planes > 3 or len(np.arange(0, L, 16)) > 2 ** 14


# ---------------------------------------------------------------------------------------
# candidate sets
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", (5, 99, 2048))
def test_candidate_sets(memo, planes):
    from memo_amd import nearest
    rng = np.random.default_rng([13, planes])
    T = nearest.tile(planes)
    n = 2 * T + 1 if planes == 2048 else T + 65
    v = draw(rng, planes, n)
    top = 1 + int(np.argmax(np.minimum(v[1:], CAP).astype(np.int64).sum(axis=1)))          # the overall best plane
    sets = [None, [planes - 1], [1], list(range(1, planes, 2)), list(range(2, planes, 2)), [g for g in range(1, planes) if g != top]]
    edges = np.linspace(0, n, 8).astype(np.int64)
    buf, where = resident(v)
    with buf:
        for cand in sets:
            for min_len in (1, CAP):
                wins = check(where, v, edges, CAP, min_len, cand)
                outside = [g for g in range(1, planes) if cand is not None and g not in cand]
                assert not wins[:, outside].any() and (cand is None or wins[0, cand].any())
        assert not check(where, v, edges, CAP, 1, sets[-1])[:, top].any()
        same(nearest.plane_nearest(where, edges, cap=CAP, candidates=",".join(str(g) for g in sets[3]))[0], O.table(v, edges, CAP, 1, sets[3])[0])
    # a plane outside the set must not win and is not read: filled with 0xFFFFFFFF (the cap, were it read), the oracle's answer stays
    for cand in sets[1:]:
        w = v.copy()
        w[[g for g in range(planes) if g not in cand]] = 0xFFFFFFFF
        check(w, v, edges, CAP, 1, cand, note="sentinel")
    w = v.copy()
    w[0] = 0xFFFFFFFF                                                                      # the pivot's plane, with every genome a candidate
    check(w, v, edges, CAP, 1, None, note="pivot")


def test_a_winner_at_every_word_edge_of_the_set(memo):
    """genomes 31, 32, 63, 64 and 2047: the last and the first bit of a candidate word"""
    planes, n = 2048, 19
    rng = np.random.default_rng(17)
    v = rng.integers(0, 3, (planes, n)).astype(np.uint32)
    planted = (31, 32, 63, 64, 2047)
    for i, g in enumerate(planted):
        v[g, 2 * i] = 4                                                      # a sole winner
        v[[g, planted[i - 1]], 2 * i + 1] = 3                                # a tie of two of them: the lower one is the winner
    edges = np.arange(n + 1)
    buf, where = resident(v)
    with buf:
        for cand in (None, list(planted), [g for g in range(1, planes) if g not in (32, 63)], [31, 64], [2047]):
            wins = check(where, v, edges, CAP, 3, cand)
            for i, g in enumerate(planted):
                if cand is None or g in cand:
                    assert wins[1, g, 2 * i] == 1 and wins[0, g, 2 * i + 1] == 1


# ---------------------------------------------------------------------------------------
# outputs
# ---------------------------------------------------------------------------------------
def test_each_output_alone_and_all_together(memo):
    from memo_amd import nearest
    rng = np.random.default_rng(19)
    for planes in (3, 200):
        n = 2 * nearest.tile(planes) + 7
        v = draw(rng, planes, n)
        edges = np.asarray(sorted(rng.integers(0, n + 1, 9).tolist() + [0, n]), np.int64)
        want_wins, want_sums = O.table(v, edges, CAP, 2)
        want_winner = O.winners(v, CAP, 2)
        buf, where = resident(v)
        with buf:
            kw = dict(cap=CAP, min_len=2)
            wins, sums, winner = nearest.plane_nearest(where, edges, sums=False, **kw)
            assert sums is None and winner is None and same(wins, want_wins) is None
            wins, sums, winner = nearest.plane_nearest(where, edges, wins=False, **kw)
            assert wins is None and winner is None and same(sums, want_sums) is None
            wins, sums, winner = nearest.plane_nearest(where, edges, wins=False, sums=False, winner=True, **kw)
            assert wins is None and sums is None and same(winner, want_winner) is None
            wins, sums, winner = nearest.plane_nearest(where, None, winner=True, **kw)              # no edges at all: bins == 0
            assert wins is None and sums is None and same(winner, want_winner) is None
            wins, sums, winner = nearest.plane_nearest(where, edges, winner=True, **kw)
            same(wins, want_wins), same(sums, want_sums), same(winner, want_winner)


def test_the_tables_are_added_to_and_slices_accumulate(memo):
    from memo_amd import nearest
    rng = np.random.default_rng(23)
    T = nearest.tile(3)
    n = T + 40
    v = draw(rng, 3, n)
    edges = np.asarray(sorted(rng.integers(0, n + 1, 9).tolist() + [0, n]), np.int64) + 50
    want_wins, want_sums = O.table(v, edges, CAP, 2, None, 50)
    want_winner = O.winners(v, CAP, 2)
    before_w = rng.integers(0, 2 ** 63, want_wins.shape, dtype=np.int64).astype(np.uint64) * np.uint64(2)     # (wraps: the adds are modulo 2^64)
    before_s = rng.integers(0, 2 ** 63, want_sums.shape, dtype=np.int64).astype(np.uint64) * np.uint64(2)
    wins, sums, _ = nearest.plane_nearest(v, edges, first=50, cap=CAP, min_len=2, wins=before_w, sums=before_s)
    same(wins, before_w + want_wins), same(sums, before_s + want_sums)
    for step in (1, 3, 7, 64, T + 1):
        m = 130 if step == 1 else n                                           # (a call a position: a shorter window)
        cut = np.minimum(edges, 50 + m)
        wins, sums, parts = before_w.copy(), before_s.copy(), []
        for a in range(0, m, step)[::-1]:                                     # from the right, as the slices of `memo lengths` come
            wins, sums, part = nearest.plane_nearest(v[:, a:min(a + step, m)], cut, first=50 + a, cap=CAP, min_len=2, wins=wins, sums=sums, winner=True)
            parts.append(part)
        want = O.table(v[:, :m], cut, CAP, 2, None, 50)
        same(wins, before_w + want[0], step), same(sums, before_s + want[1], step)
        same(np.concatenate(parts[::-1]), want_winner[:m], step)              # the winner is the same on every cut


# ---------------------------------------------------------------------------------------
# what is refused, and what launches nothing
# ---------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_as_they_were(memo):
    from memo_amd import _lib, nearest
    from memo_amd._device import DevBuffer
    L_ = _lib.lib()
    v = np.arange(96, dtype=np.uint32).reshape(3, 32) % 5
    before = np.arange(2 * 3 * 3, dtype=np.uint64).reshape(2, 3, 3) + np.uint64(7)
    before_s = np.array([5, 6, 7], np.uint64)
    before_w = np.full(32, 77, np.uint16)
    edges = np.array([0, 10, 20, 32], np.int64)
    down = np.array([0, 20, 10, 32], np.int64)
    words = lambda *gs: nearest.candidate_words(np.array([sum(1 << (g & 31) for g in gs if g >> 5 == w) for w in range(64)], np.uint32), 3)     # noqa: E731
    empty, zero, three, far, fine = words(), words(0, 1), words(1, 3), words(2, 2047), words(2)
    big = 2 ** 31
    with DevBuffer.of(v, 0) as cells, DevBuffer.of(before, 0) as table, DevBuffer.of(before_s, 0) as sums, DevBuffer.of(before_w, 0) as winner:
        d, t, s, w, e = cells.d.value, table.d.value, sums.d.value, winner.d.value, edges.ctypes.data
        ok = dict(d=d, L=32, pitch=32, planes=3, cap=4, min_len=1, c=None, first=0, e=e, bins=3, t=t, s=s, w=w)

        def call(**kw):
            a = dict(ok, **kw)
            return L_.memo_nearest_dev(a["d"], a["L"], a["pitch"], a["planes"], a["cap"], a["min_len"], a["c"], a["first"], a["e"], a["bins"],
                                       a["t"], a["s"], a["w"], 0, None)

        def untouched(kw):
            assert np.array_equal(table.to_host(before.shape, np.uint64), before), kw
            assert np.array_equal(sums.to_host(3, np.uint64), before_s) and np.array_equal(winner.to_host(32, np.uint16), before_w), kw
        refused = (dict(d=d + 4), dict(d=d + 8), dict(d=None), dict(pitch=34, L=30), dict(pitch=28), dict(L=big + 1, pitch=big + 4), dict(L=-1),
                   dict(planes=1), dict(planes=0), dict(planes=-1), dict(planes=2049), dict(bins=0), dict(bins=-3), dict(bins=2 ** 20 + 2),
                   dict(cap=0), dict(cap=2 ** 31), dict(min_len=0), dict(min_len=5), dict(e=down.ctypes.data), dict(e=None),
                   dict(first=-1), dict(first=1), dict(first=33), dict(L=0, first=40),
                   dict(c=empty.ctypes.data), dict(c=zero.ctypes.data), dict(c=three.ctypes.data), dict(c=far.ctypes.data),
                   dict(t=None, s=None, w=None), dict(t=t + 4), dict(s=s + 4), dict(w=w + 1),
                   dict(t=None, s=None, e=None, bins=3), dict(t=None, s=None, bins=-1))
        for kw in refused:
            assert call(**kw) == _lib.MEMO_EINVAL, kw
            assert L_.memo_last_error(), kw
            untouched(kw)
        # nothing to do: nothing is launched, everything stays
        for kw in (dict(L=0), dict(L=0, d=None, pitch=0), dict(L=0, t=None, s=None, e=None, bins=0)):
            assert call(**kw) == _lib.MEMO_OK, kw
            untouched(kw)
        # and the call as it stands is taken, with and without a candidate set, a table or the edges
        assert call() == _lib.MEMO_OK
        want = O.table(v, edges, 4)
        same(table.to_host(before.shape, np.uint64), before + want[0], "taken"), same(sums.to_host(3, np.uint64), before_s + want[1], "taken")
        same(winner.to_host(32, np.uint16), O.winners(v, 4), "taken")
        assert call(c=fine.ctypes.data, t=None, s=None, e=None, bins=0) == _lib.MEMO_OK
        same(winner.to_host(32, np.uint16), O.winners(v, 4, 1, [2]), "one candidate")
        assert call(w=None, s=None) == _lib.MEMO_OK and call(w=None, t=None) == _lib.MEMO_OK and call(pitch=36, L=30, planes=2, w=w + 2) == _lib.MEMO_OK


def test_the_lap_timer_and_the_lds_switch_are_the_ab_library_s(memo):
    from memo_amd import _lib, nearest
    assert not hasattr(_lib.lib(), "memo_debug_nearest_times") and not hasattr(_lib.lib(), "memo_debug_nearest_lds")
    ab = _lib.use_ab(True)
    try:
        ms = (C.c_float * 1)()
        assert ab.memo_debug_nearest_times(1, ms) == 0
        v = np.ones((3, 5000), np.uint32)
        assert nearest.plane_nearest(v, [0, 5000], cap=4)[0][:, :, 0].tolist() == [[0, 5000, 5000], [0, 0, 0]]
        assert ab.memo_debug_nearest_times(0, ms) == 0 and ms[0] > 0.0
        # one workgroup a CU: twice the tile at 99 planes, the same tables
        rng = np.random.default_rng(29)
        v = draw(rng, 99, 700)
        edges = np.array([0, 3, 130, 131, 400, 700], np.int64)
        assert nearest.tile(99) == 128 and ab.memo_debug_nearest_lds(120) == 0 and nearest.tile(99) == 256
        check(v, v, edges, CAP, 2)
        assert ab.memo_debug_nearest_lds(15) == _lib.MEMO_EINVAL and ab.memo_debug_nearest_lds(161) == _lib.MEMO_EINVAL
        assert ab.memo_debug_nearest_lds(0) == 0 and nearest.tile(99) == 128
    finally:
        ab.memo_debug_nearest_lds(0)
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# whole commands
# ---------------------------------------------------------------------------------------
from tests.test_nearest_cpu import (EXAMPLE, EXAMPLE_BEST, EXAMPLE_K3, EXAMPLE_L4, EXAMPLE_RUNS, EXAMPLE_RUNS_L4, EXAMPLE_S124,  # noqa: E402
                                    EXAMPLE_SOLE, _runs)


def test_region_nearest_on_the_example(memo):
    from memo_amd import nearest
    for step in (None, 1, 3, 7, 1000):
        wins, sums, edges, qs = nearest.region_nearest(MEMB, "ref_1:0-20", 5, 4, slice_positions=step)
        assert wins.dtype == np.uint64 and sums.dtype == np.uint64 and edges.tolist() == [0, 5, 10, 15, 20] and qs == 0
        assert wins[0].tolist() == EXAMPLE[0] and wins[1].tolist() == EXAMPLE_SOLE and sums.tolist() == EXAMPLE[1], step
    wins, sums, _, _ = nearest.region_nearest(MEMB, "ref_1:0-20", 5, 4, min_len=4)
    assert wins[0].tolist() == EXAMPLE_L4 and wins[1].tolist() == [EXAMPLE_L4[0]] + EXAMPLE_SOLE[1:] and sums.tolist() == EXAMPLE[1]
    wins, sums, _, _ = nearest.region_nearest(MEMB, "ref_1:0-20", 5, 4, min_len=3, cap=3)
    assert wins[0].tolist() == EXAMPLE_K3[0] and not wins[1, 1:].any() and sums.tolist() == EXAMPLE_K3[1]
    for cand in ("1,2,4", "1-2,4", [4, 1, 2]):
        wins, sums, _, _ = nearest.region_nearest(MEMB, "ref_1:0-20", 5, 4, candidates=cand)
        assert wins[0].tolist() == EXAMPLE_S124[0] and sums.tolist() == EXAMPLE_S124[1]
    assert nearest.region_nearest(MEMB, "ref_1:0-20", 5, 20)[1].tolist() == EXAMPLE_BEST
    for step in (None, 1, 7):
        starts, winners, qs, qe = nearest.region_winners(MEMB, "ref_1:0-20", 5, slice_positions=step)
        assert starts.dtype == np.int64 and winners.dtype == np.uint16 and (qs, qe) == (0, 20) and _runs(starts, winners, 20) == EXAMPLE_RUNS
        assert _runs(*nearest.region_winners(MEMB, "ref_1:0-20", 5, min_len=4, slice_positions=step)[:2], 20) == EXAMPLE_RUNS_L4
    assert nearest.region_nearest(MEMB, "ref_1:5-5", 5, 4)[0].shape == (2, 5, 0) and nearest.region_winners(MEMB, "ref_1:5-5", 5)[0].shape == (0,)
    with pytest.raises(OSError):
        nearest.region_nearest(os.path.join(G.GOLD, "no_such.parquet"), "ref_1:0-20", 5, 4)


def test_region_nearest_on_rnd_n40_by_three_independent_routes(memo):
    """chr1 of rnd_n40.parquet, 40 genomes: the tables are the same whole and in slices of 7 and 1000 positions, with bins that
    straddle the cuts; they are the oracle's on lengths.region_planes, `memo tracks`' through min_len == cap == K, and
    `memo lengths -t 2`'s through one bin per position"""
    from memo_amd import lengths, nearest, tracks
    s, e, a = G.index_columns("rnd_n40.parquet", "chr1")
    assert not (a == 0).any() and (e >= s).all()                              # the pivot has no rows: its plane is the cap, T = 2 is `best`
    n, K = 40, 31
    for qs, qe, steps in ((0, 2100, (None, 1000)), (150, 450, (None, 7, 1000))):
        region = f"chr1:{qs}-{qe}"
        planes = lengths.region_planes(RND40, region, n)
        for bins, min_len, cap, cand in ((13, 1, None, None), (qe - qs, 20, None, None), (13, 5, 60, "2-9,30"), (7, K, K, None)):
            edges = tracks.region_edges(qe - qs, bins)
            assert bins == qe - qs or (np.diff(edges) % 7 != 0).any()           # the bins straddle the cuts
            chosen = None if cand is None else [2, 3, 4, 5, 6, 7, 8, 9, 30]
            want = O.table(planes, edges, CAP_MAX if cap is None else cap, min_len, chosen)
            for step in steps:
                wins, sums, got_edges, got_qs = nearest.region_nearest(RND40, region, n, bins, candidates=cand, min_len=min_len, cap=cap, slice_positions=step)
                assert got_qs == qs and np.array_equal(got_edges, edges)
                same(wins, want[0], (region, bins, step)), same(sums, want[1], (region, bins, step))
            assert (wins[1] <= wins[0]).all() and wins[0, 1:].any()
            if min_len == cap == K:
                counts, _ = tracks.region_tracks(RND40, region, K, n, bins)
                same(wins[0, 1:], counts[1:], "the K identity")
            if bins == qe - qs:
                per = nearest.region_nearest(RND40, region, n, bins)[1]
                same(per, lengths.region_kth(RND40, region, n, threshold=2).astype(np.uint64), "one bin per position")
        for step in steps:
            starts, winners, got_qs, got_qe = nearest.region_winners(RND40, region, n, min_len=12, slice_positions=step)
            want_starts, want_winners = O.run_code(O.winners(planes, CAP_MAX, 12))
            assert (got_qs, got_qe) == (qs, qe) and len(starts) > 10
            same(starts, want_starts, (region, step)), same(winners, want_winners, (region, step))


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


HEAD = "genome\t0-5\t5-10\t10-15\t15-20\n"
README_TABLE = HEAD + "none\t0\t0\t0\t0\n1\t1\t0\t1\t0\n2\t2\t3\t2\t4\n3\t5\t3\t3\t2\n4\t2\t0\t3\t2\nbest\t21\t32\t19\t23\n"
README_SOLE = HEAD + "none\t0\t0\t0\t0\n1\t0\t0\t1\t0\n2\t0\t2\t0\t2\n3\t2\t2\t1\t1\n4\t0\t0\t1\t0\nbest\t21\t32\t19\t23\n"
README_S124 = HEAD + "none\t0\t0\t0\t0\n1\t1\t0\t2\t0\n2\t4\t5\t3\t4\n3\t0\t0\t0\t0\n4\t2\t0\t4\t3\nbest\t19\t30\t18\t21\n"
README_INTERVALS = "".join(f"ref_1\t{a}\t{b}\t{g}\n" for a, b, g in EXAMPLE_RUNS)
README_INTERVALS_L4 = "".join(f"ref_1\t{a}\t{b}\t{g or '.'}\n" for a, b, g in EXAMPLE_RUNS_L4)


def _run(tmp_path, *flags, region=("-r", "ref_1:0-20", "-B", "4")):
    out = str(tmp_path / "n.tsv")
    r = _memo("nearest", "-b", MEMB, "-n", "5", *region, "-o", out, *flags)
    assert (r.returncode, r.stdout) == (0, b"MEMO - nearest\n"), (flags, r.stderr)
    return open(out).read()


def test_cli_writes_the_readme_s_tables(memo, tmp_path):
    assert _run(tmp_path) == README_TABLE
    assert _run(tmp_path, "-u") == README_SOLE
    assert _run(tmp_path, "-s", "1,2,4") == README_S124
    assert _run(tmp_path, "-l", "4", "-u").splitlines()[1] == "none\t2\t0\t1\t1"
    text = _run(tmp_path, "-f").splitlines()
    assert text[4] == "3\t1.0\t0.6\t0.6\t0.4" and text[-1] == "best\t4.2\t6.4\t3.8\t4.6" and text[1] == "none\t0.0\t0.0\t0.0\t0.0"
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    text = _run(tmp_path, "-g", str(genomes))
    assert [ln.split("\t")[0] for ln in text.splitlines()] == ["genome", "none", "g1", "g2", "g3", "g4", "best"]
    assert [ln.split("\t", 1)[1] for ln in text.splitlines()] == [ln.split("\t", 1)[1] for ln in README_TABLE.splitlines()]
    assert _run(tmp_path, region=("-r", "ref_1:5-5")) == ""                                   # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "n.tsv"]                           # written beside its name and renamed


def test_cli_writes_the_intervals(memo, tmp_path):
    window = ("-r", "ref_1:0-20")
    assert _run(tmp_path, "-i", region=window) == README_INTERVALS and README_INTERVALS.count("\n") == 11
    assert _run(tmp_path, "-i", "-l", "4", region=window) == README_INTERVALS_L4 and README_INTERVALS_L4.count("\n") == 13
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("pivot.fa\ng1.fa\ng2.fa\ng3.fa\ng4.fa\n")
    assert _run(tmp_path, "-i", "-g", str(genomes), region=window).splitlines()[:3] == ["ref_1\t0\t2\tg3", "ref_1\t2\t4\tg2", "ref_1\t4\t5\tg1"]
    assert _run(tmp_path, "-i", "-s", "4", region=("-r", "ref_1:7-19")).splitlines()[0].startswith("ref_1\t7\t")
    assert _run(tmp_path, "-i", region=("-r", "ref_1:5-5")) == ""
    never = str(tmp_path / "never.tsv")
    r = _memo("nearest", "-b", MEMB, "-n", "5", "-r", "ref_1:0-20", "-o", never)               # -B 500: more bins than positions
    assert r.returncode == 1 and b"500 bins for a window of 20 positions" in r.stderr and not os.path.exists(never)
