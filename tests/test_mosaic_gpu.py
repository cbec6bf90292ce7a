"""`memo mosaic` on the GPU: the fold and the parse (memo_amd/csrc/memo_mosaic.hip) against the oracle (tests/mosaic_oracle.py), the
window routes against it and, independently of it, against `memo nearest` and `memo lengths`; the command line against the README.

Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import mosaic_oracle as M
from tests.test_mosaic_cpu import EDGES4, EXAMPLE, EXAMPLE_3_17, EXAMPLE_B4, RND40
from tests.test_nearest_gpu import CAP, draw, held, resident, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
MEMB = os.path.join(G.GOLD, "example_memb.parquet")
RND = os.path.join(G.GOLD, "rnd_n40.parquet")
REACH = 256 * 4                                                  # the positions of a fold workgroup


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def fold_check(where, v, cap, min_len=1, candidates=None, note=None):
    """step, winner and the lines of one call against the oracle"""
    from memo_amd import mosaic
    starts, genomes, step, winner = mosaic.plane_mosaic(where, cap=cap, min_len=min_len, candidates=candidates, vectors=True)
    want_step, want_winner = M.steps(v, cap, min_len, candidates)
    note = (note, v.shape, min_len, candidates if candidates is None or len(candidates) < 9 else len(candidates))
    same(step, want_step, note), same(winner, want_winner, note)
    want = M.greedy(want_step, want_winner)
    same(starts, want[0], note), same(genomes, want[1], note)


# ---------------------------------------------------------------------------------------
# the fold against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", (2, 3, 5, 99, 2048))
def test_the_fold_against_the_oracle(memo, planes):
    """every length around a lane's four cells, a wave's 256 and a workgroup's 1024, min_len 1, 2 and the cap.  An input of at least 3
    positions holds an all-zero column, a column at the cap, a tie and a cell above the cap (asserted on the oracle's side)."""
    rng = np.random.default_rng([20261021, planes])
    for n in (1, 2, 3, 4, 5, 255, 256, 257, REACH - 1, REACH, REACH + 1):
        v = draw(rng, planes, n)
        if n >= 3:
            what = held(v)
            assert all(what[k] for k in what if k != "a tie" or planes > 2), (n, what)
        buf, where = resident(v)                                 # (0xFFFFFFFF behind L: were it read, it would show)
        with buf:
            for min_len in (1, 2, CAP):
                fold_check(where, v, CAP, min_len)
    v = draw(rng, planes, REACH + 3)                             # a host array goes the same way
    fold_check(v, v, CAP)


@pytest.mark.parametrize("planes", (5, 99, 2048))
def test_candidate_sets(memo, planes):
    from memo_amd import mosaic
    rng = np.random.default_rng([13, planes])
    n = 261
    v = draw(rng, planes, n)
    top = 1 + int(np.argmax(np.minimum(v[1:], CAP).astype(np.int64).sum(axis=1)))
    sets = [None, [planes - 1], [1], list(range(1, planes, 2)), list(range(2, planes, 2)), [g for g in range(1, planes) if g != top]]
    buf, where = resident(v)
    with buf:
        for cand in sets:
            for min_len in (1, CAP):
                fold_check(where, v, CAP, min_len, cand)
        as_text = mosaic.plane_mosaic(where, cap=CAP, candidates=",".join(str(g) for g in sets[3]), vectors=True)      # `memo merge -s` syntax
        same(as_text[3], M.steps(v, CAP, 1, sets[3])[1], "a selection as text")
    # a plane outside the set is not read: filled with 0xFFFFFFFF (the cap, were it read), the oracle's answer stays
    for cand in sets[1:]:
        w = v.copy()
        w[[g for g in range(planes) if g not in cand]] = 0xFFFFFFFF
        fold_check(w, v, CAP, 1, cand, note="sentinel")
    w = v.copy()
    w[0] = 0xFFFFFFFF                                            # the pivot's plane, with every genome a candidate
    fold_check(w, v, CAP, 1, None, note="pivot")


def test_the_fold_writes_its_slice_and_nothing_else(memo):
    """output offsets of 0 .. 3 elements into a larger vector (4- and 2-byte aligned addresses), the neighbours as they were; and
    slices of 1, 3, 7 and 64 positions from the right leave the vectors of the whole"""
    from memo_amd import mosaic
    from memo_amd._device import DevBuffer
    from memo_amd.lengths import pitch_of
    rng = np.random.default_rng(31)
    planes = 5
    for n in (1, 3, 4, 5, 9, 257, REACH + 2):
        v = draw(rng, planes, n)
        want_step, want_winner = M.steps(v, CAP, 2)
        buf, where = resident(v)
        with buf:
            for off in (0, 1, 2, 3):
                fill_s, fill_w = np.full(n + 8, 0xABCDEF01, np.uint32), np.full(n + 8, 0xBEEF, np.uint16)
                with DevBuffer.of(fill_s, 0) as d_step, DevBuffer.of(fill_w, 0) as d_winner:
                    mosaic._fold(where[0], n, where[2], planes, CAP, 2, None, d_step.at(4 * off), d_winner.at(2 * off), 0)
                    step, winner = d_step.to_host(n + 8, np.uint32), d_winner.to_host(n + 8, np.uint16)
                fill_s[off:off + n], fill_w[off:off + n] = want_step, want_winner
                same(step, fill_s, (n, off)), same(winner, fill_w, (n, off))
    n = 200
    v = draw(rng, planes, n)
    want_step, want_winner = M.steps(v, CAP)
    for cut in (1, 3, 7, 64):
        with DevBuffer.of(np.zeros(n, np.uint32), 0) as d_step, DevBuffer.of(np.zeros(n, np.uint16), 0) as d_winner:
            for a in range(0, n, cut)[::-1]:                     # from the right, as the slices of `memo lengths` come
                part = np.ascontiguousarray(v[:, a:min(a + cut, n)])
                padded = np.full((planes, pitch_of(part.shape[1])), 0xFFFFFFFF, np.uint32)
                padded[:, :part.shape[1]] = part
                with DevBuffer.of(padded, 0) as cells:
                    mosaic._fold(cells.d, part.shape[1], padded.shape[1], planes, CAP, 1, None, d_step.at(4 * a), d_winner.at(2 * a), 0)
            same(d_step.to_host(n, np.uint32), want_step, cut), same(d_winner.to_host(n, np.uint16), want_winner, cut)
            lines = mosaic._parse(d_step.d, d_winner.d, n, 0)
        want = M.greedy(want_step, want_winner)
        same(lines[0], want[0], cut), same(lines[1], want[1], cut)


# ---------------------------------------------------------------------------------------
# the parse alone against the oracle
# ---------------------------------------------------------------------------------------
def parse_check(step, winner, note):
    from memo_amd import mosaic
    step, winner = np.asarray(step, np.uint32), np.asarray(winner, np.uint16)
    starts, genomes = mosaic.parse(step, winner)
    want = M.greedy(step, winner)
    same(starts, want[0], note), same(genomes, want[1], note)
    return want


def geometric(rng, L, mean):
    return np.maximum(rng.geometric(1.0 / mean, L), 1).astype(np.uint32)


def ramps(rng, L, mean):
    """falling ramps between random breaks, as an index leaves them"""
    at = np.flatnonzero(rng.random(L) < 1.0 / mean)
    at = np.concatenate([[0], at[at > 0], [L]])
    reach = np.maximum.accumulate(at[:-1] + rng.integers(1, 2 * mean, len(at) - 1))
    return np.maximum(np.repeat(reach, np.diff(at)) - np.arange(L), 1).astype(np.uint32)


def test_the_parse_at_every_length_and_step(memo):
    from memo_amd import mosaic
    T = mosaic.tile()
    assert T in (4096, 8192, 16384, 32768)
    rng = np.random.default_rng(41)
    for L in (1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5):
        genome = rng.integers(1, 9, L).astype(np.uint16)
        for name, step in (("all 1", np.ones(L, np.uint32)), ("all T", np.full(L, T, np.uint32)), ("all T - 1", np.full(L, T - 1, np.uint32)),
                           ("all T + 1", np.full(L, T + 1, np.uint32)), ("mean 1.5", geometric(rng, L, 1.5)), ("mean 8", geometric(rng, L, 8)),
                           ("mean 100", geometric(rng, L, 100)), ("mean T / 4", geometric(rng, L, T // 4)), ("ramps", ramps(rng, L, 100))):
            want = parse_check(step, genome, (name, L))
            if name == "all 1":
                assert len(want[0]) == L                         # every position reached: the longest chain a tile can hold
            if name == "all T + 1" and L > 3 * T:
                assert want[0].tolist()[:3] == [0, T + 1, 2 * T + 2]         # the entry offset drifts across the tiles
    # many hops of the serial walk
    L = 64 * T + 3
    genome = rng.integers(1, 9, L).astype(np.uint16)
    for name, step in (("all T + 1", np.full(L, T + 1, np.uint32)), ("all T - 1", np.full(L, T - 1, np.uint32)), ("mean 8", geometric(rng, L, 8)),
                       ("ramps", ramps(rng, L, 100))):
        want = parse_check(step, genome, (name, L))
        assert len({int(s) // T for s in want[0]}) >= 63, name   # (nearly) every tile entered


def test_steps_that_land_on_and_beside_the_edges(memo):
    from memo_amd import mosaic
    T = mosaic.tile()
    rng = np.random.default_rng(43)
    L = 4 * T + 10
    genome = rng.integers(1, 9, L).astype(np.uint16)
    base = geometric(rng, L, 8)
    for name, at, length, lands in (("a tile's last position", 5, T - 6, T - 1), ("the next tile's first", 5, T - 5, T), ("skips one tile", 5, 2 * T - 5, 2 * T),
                                    ("skips two tiles", 5, 3 * T - 5, 3 * T), ("lands on L - 1", 5, L - 6, L - 1), ("lands on L", 5, L - 5, L),
                                    ("past L", 5, L + 7, L + 12), ("2^31 - 1 at 0", 0, CAP_MAX, CAP_MAX), ("2^31 - 1 mid-tile", T + T // 2, CAP_MAX, None),
                                    ("above 2^31 - 1", 0, 0xFFFFFFFF, None)):
        step = base.copy()
        step[:at + 1] = 1                                        # the chain reaches `at`
        if at > T:
            step[0], step[1:at] = at, 1
        step[at] = length
        want = parse_check(step, genome, name)
        reached = [int(s) for s in want[0]]
        assert at in reached, name
        if lands is not None and lands < L:
            assert lands in reached and not any(at < r < lands for r in reached), name
        elif lands is not None:
            assert reached[-1] == at, name                       # the last line
    step = base.copy()
    step[[0, 7, T, T + 1]] = 0                                   # a 0 is taken as 1
    step[:8], step[8] = np.array([0, 1, 1, 1, 1, 1, 1, 0]), T - 8
    want = parse_check(step, genome, "zeros")
    assert [int(s) for s in want[0][:12]] == [0, 1, 2, 3, 4, 5, 6, 7, 8, T, T + 1, T + 2]


def test_lines_of_no_genome(memo):
    from memo_amd import mosaic
    T = mosaic.tile()
    rng = np.random.default_rng(47)
    L = 2 * T + 40
    ones, genome = np.ones(L, np.uint32), rng.integers(1, 9, L).astype(np.uint16)
    # none at position 0, and as a run that crosses the tile boundary: one line each
    w = genome.copy()
    w[0], w[T - 3:T + 4] = 0, 0
    want = parse_check(ones, w, "none at 0 and across a tile")
    assert want[1][0] == 0 and want[0][1] == 1 and int((want[1] == 0).sum()) == 2 and T - 3 in want[0] and T + 4 in want[0] and T not in want[0]
    # the whole window
    want = parse_check(ones, np.zeros(L, np.uint16), "none everywhere")
    assert want[0].tolist() == [0] and want[1].tolist() == [0]
    # a run of none entered in its middle by a copy that ends inside it: p - 1 is none but not reached, a new `.` line
    for first in (10, T - 1, T):                                 # ... inside a tile, and with p or p - 1 a tile's first position
        w, step = genome.copy(), ones.copy()
        w[first - 4:first + 5] = 0
        step[:first - 8], step[first - 8] = 1, 9                 # a copy from first - 8 to first + 1
        step[0], step[1:first - 8] = first - 8, 1
        w[0] = 3
        want = parse_check(step, w, ("entered in the middle", first))
        assert M.intervals(*want, L)[:3] == [(0, first - 8, 3), (first - 8, first + 1, int(genome[first - 8])), (first + 1, first + 5, 0)]
    # a run of none at the window's end, and adjacent phrases of one genome staying two lines
    w, step = genome.copy(), ones.copy()
    w[L - 9:] = 0
    w[:L - 9] = 5
    step[:L - 9] = 3
    want = parse_check(step, w, "none at the end")
    assert want[1][-1] == 0 and want[0][-1] == (L - 9 + 2) // 3 * 3 and (want[1][:-1] == 5).all() and len(want[0]) == (L - 9 + 2) // 3 + 1


# ---------------------------------------------------------------------------------------
# what is refused, and what launches nothing
# ---------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_as_they_were(memo):
    from memo_amd import _lib, nearest
    from memo_amd._device import DevBuffer
    L_ = _lib.lib()
    v = np.arange(96, dtype=np.uint32).reshape(3, 32) % 5
    before_s, before_w = np.full(32, 77, np.uint32), np.full(32, 78, np.uint16)
    words = lambda *gs: nearest.candidate_words(np.array([sum(1 << (g & 31) for g in gs if g >> 5 == w) for w in range(64)], np.uint32), 3)     # noqa: E731
    empty, zero, three, far, fine = words(), words(0, 1), words(1, 3), words(2, 2047), words(2)
    big = 2 ** 31
    with DevBuffer.of(v, 0) as cells, DevBuffer.of(before_s, 0) as step, DevBuffer.of(before_w, 0) as winner:
        d, s, w = cells.d.value, step.d.value, winner.d.value
        ok = dict(d=d, L=32, pitch=32, planes=3, cap=4, min_len=1, c=None, s=s, w=w)

        def fold(**kw):
            a = dict(ok, **kw)
            return L_.memo_mosaic_fold_dev(a["d"], a["L"], a["pitch"], a["planes"], a["cap"], a["min_len"], a["c"], a["s"], a["w"], 0, None)

        def untouched(kw):
            assert np.array_equal(step.to_host(32, np.uint32), before_s) and np.array_equal(winner.to_host(32, np.uint16), before_w), kw
        for kw in (dict(d=d + 4), dict(d=d + 8), dict(d=None), dict(pitch=34, L=30), dict(pitch=28), dict(L=big, pitch=big), dict(L=-1), dict(planes=1),
                   dict(planes=0), dict(planes=-1), dict(planes=2049), dict(cap=0), dict(cap=2 ** 31), dict(min_len=0), dict(min_len=5),
                   dict(c=empty.ctypes.data), dict(c=zero.ctypes.data), dict(c=three.ctypes.data), dict(c=far.ctypes.data),
                   dict(s=None), dict(w=None), dict(s=s + 2), dict(s=s + 1), dict(w=w + 1)):
            assert fold(**kw) == _lib.MEMO_EINVAL, kw
            assert L_.memo_last_error(), kw
            untouched(kw)
        for kw in (dict(L=0), dict(L=0, d=None, pitch=0)):       # nothing to do: nothing is launched
            assert fold(**kw) == _lib.MEMO_OK, kw
            untouched(kw)
        # the parse: the out-pointers keep what they held
        d_starts, d_genomes, n = C.c_void_p(12345), C.c_void_p(6789), C.c_uint64(55)

        def parse(**kw):
            a = dict(dict(s=s, w=w, L=32, o1=C.byref(d_starts), o2=C.byref(d_genomes), n=C.byref(n)), **kw)
            return L_.memo_mosaic_parse_dev(a["s"], a["w"], a["L"], a["o1"], a["o2"], a["n"], 0, None)
        for kw in (dict(s=None), dict(w=None), dict(s=s + 4), dict(w=w + 2), dict(w=w + 8), dict(L=-1), dict(L=big), dict(o1=None), dict(o2=None), dict(n=None)):
            assert parse(**kw) == _lib.MEMO_EINVAL, kw
            assert L_.memo_last_error() and (d_starts.value, d_genomes.value, n.value) == (12345, 6789, 55), kw
        for kw in (dict(L=0), dict(L=0, s=None, w=None)):
            assert parse(**kw) == _lib.MEMO_OK and (d_starts.value, d_genomes.value, n.value) == (None, None, 0), kw
            d_starts, d_genomes, n = C.c_void_p(12345), C.c_void_p(6789), C.c_uint64(55)
        # and the calls as they stand are taken
        assert fold() == _lib.MEMO_OK
        want = M.steps(v, 4)
        same(step.to_host(32, np.uint32), want[0], "taken"), same(winner.to_host(32, np.uint16), want[1], "taken")
        assert fold(c=fine.ctypes.data, L=30, s=s + 4, w=w + 2) == _lib.MEMO_OK
        same(step.to_host(32, np.uint32)[1:31], M.steps(v[:, :30], 4, 1, [2])[0], "one candidate")
        assert parse() == _lib.MEMO_OK and n.value >= 1
        with DevBuffer.adopt(d_starts, 0) as b_starts, DevBuffer.adopt(d_genomes, 0) as b_genomes:
            got = b_starts.to_host(n.value, np.int64), b_genomes.to_host(n.value, np.uint16)
        want = M.greedy(step.to_host(32, np.uint32), winner.to_host(32, np.uint16))
        same(got[0], want[0], "parsed"), same(got[1], want[1], "parsed")


def test_the_lap_timer_and_the_shape_switch_are_the_ab_library_s(memo):
    from memo_amd import _lib, mosaic
    assert not hasattr(_lib.lib(), "memo_debug_mosaic_times") and not hasattr(_lib.lib(), "memo_debug_mosaic_shape")
    product = mosaic.tile()
    ab = _lib.use_ab(True)
    try:
        ms = (C.c_float * 5)()
        assert ab.memo_debug_mosaic_times(1, ms) == 0
        v = np.ones((3, 5000), np.uint32)
        assert [x.tolist() for x in mosaic.plane_mosaic(v, cap=4)] == [list(range(5000)), [1] * 5000]
        assert ab.memo_debug_mosaic_times(0, ms) == 0 and all(ms[i] > 0.0 for i in range(5))
        # every tile and both marks: the same lines
        rng = np.random.default_rng(53)
        L = 2 * 32768 + 77
        winner = rng.integers(0, 4, L).astype(np.uint16)
        inputs = [(geometric(rng, L, 8), winner), (ramps(rng, L, 100), winner), (np.ones(L, np.uint32), winner)]
        for step, _ in inputs:
            step[winner == 0] = 1                                # (a phrase of no genome is one base long: the fold's step)
        assert (winner == 0).sum() > L // 8
        wants = [M.greedy(*x) for x in inputs]
        for T in (4096, 8192, 16384, 32768):
            for mark in (1, 2):
                assert ab.memo_debug_mosaic_shape(T, mark) == 0 and mosaic.tile() == T
                for x, want in zip(inputs, wants):
                    got = mosaic.parse(*x)
                    same(got[0], want[0], (T, mark)), same(got[1], want[1], (T, mark))
        assert ab.memo_debug_mosaic_shape(1000, 0) == _lib.MEMO_EINVAL and ab.memo_debug_mosaic_shape(0, 3) == _lib.MEMO_EINVAL
        assert ab.memo_debug_mosaic_shape(0, 0) == 0 and mosaic.tile() == product
    finally:
        ab.memo_debug_mosaic_shape(0, 0)
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# whole commands
# ---------------------------------------------------------------------------------------
def test_region_mosaic_on_the_example(memo):
    from memo_amd import mosaic
    for step in (None, 1, 3, 7, 1000):
        for kw, want in EXAMPLE:
            starts, genomes, qs, qe = mosaic.region_mosaic(MEMB, "ref_1:0-20", 5, slice_positions=step, **kw)
            assert starts.dtype == np.int64 and genomes.dtype == np.uint16 and (qs, qe) == (0, 20)
            assert M.intervals(starts, genomes, 20) == want, (step, kw)
        starts, genomes, qs, qe = mosaic.region_mosaic(MEMB, "ref_1:3-17", 5, slice_positions=step)
        assert M.intervals(starts, genomes, qe, qs) == EXAMPLE_3_17
    for cand in ("1,2,4", "1-2,4", [4, 1, 2]):
        assert M.intervals(*mosaic.region_mosaic(MEMB, "ref_1:0-20", 5, candidates=cand)[:2], 20) == EXAMPLE[3][1]
    starts, genomes, _, _ = mosaic.region_mosaic(MEMB, "ref_1:0-20", 5)
    bases, lines = mosaic.bin_phrases(starts, genomes, 20, EDGES4, 5)
    assert bases.tolist() == EXAMPLE_B4[0] and lines.tolist() == EXAMPLE_B4[1]
    assert mosaic.region_mosaic(MEMB, "ref_1:5-5", 5)[0].shape == (0,)
    with pytest.raises(OSError):
        mosaic.region_mosaic(os.path.join(G.GOLD, "no_such.parquet"), "ref_1:0-20", 5)


def test_region_mosaic_on_rnd_n40(memo):
    """chr1 of rnd_n40.parquet, 40 genomes: the counts of DESIGN.md 10.18; the lines equal the oracle's on lengths.region_planes, whole
    and in slices of 7 and 1000 positions; and, independently of the oracle: the lines partition the window, a line's genome is
    region_winners' winner at its START, a line of a genome is as long as that genome's match (cut at the window's end), and at
    MINLEN 1 the count is the dynamic programme's"""
    from memo_amd import lengths, mosaic, nearest
    n = 40
    planes = {}
    for (qs, qe), kw, count in RND40:
        region = f"chr1:{qs}-{qe}"
        if region not in planes:
            planes[region] = lengths.region_planes(RND, region, n)
        v = planes[region]
        cap, min_len, cand = kw.get("cap"), kw.get("min_len", 1), kw.get("candidates")
        want = M.greedy(*M.steps(v, CAP_MAX if cap is None else cap, min_len, cand))
        for step in (None, 7, 1000):
            starts, genomes, got_qs, got_qe = mosaic.region_mosaic(RND, region, n, slice_positions=step, **kw)
            assert (got_qs, got_qe) == (qs, qe) and len(starts) == count, (region, kw, step)
            same(starts, want[0], (region, kw, step)), same(genomes, want[1], (region, kw, step))
        if min_len == 90:
            assert int((genomes == 0).sum()) == 13
        # independently of the oracle
        L = qe - qs
        assert starts[0] == 0 and (np.diff(starts) > 0).all() and starts[-1] < L
        ends = np.append(starts[1:], L)
        run_starts, run_winners, _, _ = nearest.region_winners(RND, region, n, candidates=cand, min_len=min_len, cap=cap)
        at = np.searchsorted(run_starts, starts, "right") - 1
        same(genomes, run_winners[at], "the winner at START")
        clamped = np.minimum(v.astype(np.int64), CAP_MAX if cap is None else cap)
        copied = genomes != 0
        assert np.array_equal((ends - starts)[copied], np.minimum(clamped[genomes[copied], starts[copied]], L - starts[copied]))
        if min_len == 1:
            members = list(range(1, n)) if cand is None else cand
            assert len(starts) == M.fewest(clamped[members].max(axis=0))


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def _run(tmp_path, *flags, region=("-r", "ref_1:0-20")):
    out = str(tmp_path / "m.tsv")
    r = _memo("mosaic", "-b", MEMB, "-n", "5", *region, "-o", out, *flags)
    assert (r.returncode, r.stdout) == (0, b"MEMO - mosaic\n"), (flags, r.stderr)
    return open(out).read()


def _text(lines, name=lambda g: str(g)):
    return "".join(f"ref_1\t{a}\t{b}\t{name(g) if g else '.'}\n" for a, b, g in lines)


README_TABLE = ("genome\t0-5\t5-10\t10-15\t15-20\nnone\t0\t0\t0\t0\n1\t0\t0\t0\t0\n2\t0\t4\t3\t3\n3\t5\t1\t2\t2\n4\t0\t0\t0\t0\n"
                "phrases\t1\t1\t1\t1\n")


def test_cli_writes_the_readme_s_files(memo, tmp_path):
    assert _run(tmp_path) == _text(EXAMPLE[0][1]) == "ref_1\t0\t6\t3\nref_1\t6\t13\t2\nref_1\t13\t17\t3\nref_1\t17\t20\t2\n"
    assert _run(tmp_path, "-l", "4") == _text(EXAMPLE[1][1])
    assert _run(tmp_path, "-l", "5") == _text(EXAMPLE[2][1]) and "ref_1\t13\t15\t.\n" in _text(EXAMPLE[2][1])
    assert _run(tmp_path, "-l", "3", "-K", "3") == _text(EXAMPLE[6][1])
    assert _run(tmp_path, region=("-r", "ref_1:3-17")) == _text(EXAMPLE_3_17)
    assert _run(tmp_path, region=("-r", "ref_1:5-5")) == ""                                   # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["m.tsv"]                                          # written beside its name and renamed


def test_cli_writes_the_readme_s_files_of_chosen_genomes(memo, tmp_path):
    assert _run(tmp_path, "-s", "1,2,4") == _text(EXAMPLE[3][1]) and "ref_1\t0\t5\t2\nref_1\t5\t13\t2\n" in _text(EXAMPLE[3][1])
    assert _run(tmp_path, "-s", "1") == _text(EXAMPLE[4][1]) and _text(EXAMPLE[4][1]).count("\n") == 8
    assert _run(tmp_path, "-s", "4") == _text(EXAMPLE[5][1]) and _text(EXAMPLE[5][1]).count("\n") == 7


def test_cli_writes_the_table_and_the_labels(memo, tmp_path):
    assert _run(tmp_path, "-B", "4") == README_TABLE
    text = _run(tmp_path, "-B", "4", "-f").splitlines()
    assert text[3] == "2\t0.0\t0.8\t0.6\t0.6" and text[4] == "3\t1.0\t0.2\t0.4\t0.4" and text[-1] == "phrases\t0.2\t0.2\t0.2\t0.2"
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    assert _run(tmp_path, "-g", str(genomes)) == _text(EXAMPLE[0][1], lambda g: f"g{g}")
    text = _run(tmp_path, "-B", "4", "-g", str(genomes))
    assert [ln.split("\t")[0] for ln in text.splitlines()] == ["genome", "none", "g1", "g2", "g3", "g4", "phrases"]
    assert _run(tmp_path, "-B", "4", region=("-r", "ref_1:5-5")) == ""
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "m.tsv"]                           # written beside its name and renamed
    never = str(tmp_path / "never.tsv")
    r = _memo("mosaic", "-b", MEMB, "-n", "5", "-r", "ref_1:0-20", "-B", "21", "-o", never)
    assert r.returncode == 1 and b"21 bins for a window of 20 positions" in r.stderr and not os.path.exists(never)
