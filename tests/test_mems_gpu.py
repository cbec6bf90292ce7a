"""`memo mems` on the GPU: the kernels of memo_amd/csrc/memo_mems.hip on cells the test uploads itself (the start test is a rule on values)
against the rule in NumPy (tests/mems_oracle.py), and from the rows of the golden indexes, every mode against the definition, against
`memo maxk`, against `memo regions`, and the command line against the lists of DESIGN.md 10.13.

Every comparison is exact.  Rows with end < start are compared with the oracle only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import mems_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
SCAN_ROUND = 1024                       # tile counts one round of memo::scan_tile_counts takes (memo_compact.hip)
GUARD = 4                               # uint32 words before and behind the cells: the cells stay 16-byte aligned


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture(scope="module")
def Tt(memo):
    from memo_amd import mems
    t = mems.tile()
    assert t >= 1024 and t % 256 == 0
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

    def close(self):
        for d in self.held:
            self.lib.memo_dev_free(0, d)
        self.held = []


@pytest.fixture()
def dev(memo):
    d = Device()
    yield d
    d.close()


# ---------------------------------------------------------------------------------------
# the rule on values: cells the test uploads
# ---------------------------------------------------------------------------------------
def lengths(Tt):
    return (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, Tt - 1, Tt, Tt + 1, 2 * Tt - 1, 2 * Tt, 2 * Tt + 1)


def contents(L, cap, Tt, rng):
    """[(name, uint32 [L])]: values at most cap"""
    i = np.arange(L, dtype=np.int64)
    low = min(3, cap)
    out = [("all equal below the cap: every cell a start" if low < cap else "all equal at the cap", np.full(L, low, np.int64)),
           ("all equal at the cap: one run", np.full(L, cap, np.int64)),
           ("falling by one: a single start", np.maximum(min(cap, L + 5) - i, 0)),
           ("rising, then a run at the cap", np.minimum(i, cap)),
           ("zeros", np.zeros(L, np.int64)),
           ("runs at the cap followed by cap - 1", np.where(i % 6 == 5, cap - 1, cap)),
           ("runs at the cap followed by cap - 2", np.where(i % 4 == 3, max(cap - 2, 0), cap)),
           ("random values", rng.integers(0, min(cap, 6) + 1, L)),
           ("random values up to the cap", rng.choice(np.asarray([0, 1, 2, max(cap - 2, 0), cap - 1, cap], np.int64), L))]
    # a start in the first and in the last cell of every lane's load, wave, tile and of the plane: a fall before it, the top value in it
    edges = np.zeros(L, np.int64)
    for step in (4, 64 * 4, 1024, Tt):
        for at in (i[::step], i[::step] - 1):
            at = at[(at >= 0) & (at < L)]
            edges[at] = np.maximum(edges[at], min(cap, 2 + step % 5))
    if L:
        edges[[0, L - 1]] = cap
    out.append(("starts at the edges of loads, waves, tiles and the plane", edges))
    return [(name, v.astype(np.uint32)) for name, v in out]


def min_lens(values, cap):
    """1, 2, a value that occurs, the cap, and one that leaves nothing (where the cap leaves room for one)"""
    top = int(values.max()) if values.size else 0
    occurs = int(values.flat[values.size // 2]) if values.size else 1
    return sorted({m for m in (1, 2, occurs, cap, top + 1) if 1 <= m <= cap})


def laid_out(planes_values, pitch, cap):
    """the cells between words that would change a flag at either end if they were read, [L, pitch) of every plane filled with values
    that would be starts: rising above whatever lies before them"""
    P, L = planes_values.shape
    buf = np.empty(GUARD + P * pitch + GUARD, np.uint32)
    buf[:GUARD] = (0, cap, 0, 0xFFFFFFFF)                        # before cell 0 of plane 0
    body = buf[GUARD:GUARD + P * pitch].reshape(P, pitch)
    body[:, :L] = planes_values
    body[:, L:] = (np.arange(pitch - L, dtype=np.int64) + 0x7FFFFFF0).astype(np.uint32)
    buf[GUARD + P * pitch:] = (0xFFFFFFFF, 0xFFFFFFFE, cap, 0)
    return buf


def check_cells(dev, planes_values, pitch, cap, note, min_len_list=None):
    """both keys, halo 0 and 1, every min_len: the device's lists == the rule's, plane by plane"""
    from memo_amd import mems
    P, L = planes_values.shape
    d = dev.put(laid_out(planes_values, pitch, cap)) + 4 * GUARD
    values = planes_values.astype(np.int64)
    calls = 0
    for min_len in min_lens(planes_values, cap) if min_len_list is None else min_len_list:
        for band, halo in ((False, 0), (False, 1), (True, 0)):
            mask = mems_oracle.band_mask(values, min_len) if band else mems_oracle.start_mask(values, cap, min_len, halo)
            plane, cell = np.nonzero(mask)                      # row-major: plane-major, ascending within a plane
            starts, lens, counts = mems.of_cells(d, L, pitch, P, cap=cap, min_len=min_len, band=band, halo=halo)
            what = (note, L, pitch, P, cap, min_len, "band" if band else f"starts, halo {halo}")
            assert starts.dtype == np.uint32 and counts.dtype == np.uint64 and counts.shape == (P,), what
            assert np.array_equal(counts, np.bincount(plane, minlength=P)), what
            assert np.array_equal(starts, cell), what
            if band:
                assert lens is None
            else:
                assert lens.dtype == np.uint32 and np.array_equal(lens, values[plane, cell]), what
            calls += 1
    return calls


@pytest.mark.parametrize("planes", (1, 3, 130))
def test_the_rule_on_uploaded_cells_at_every_length(dev, Tt, planes):
    calls = 0
    for L in lengths(Tt):
        for pitch in ((L + 3) & ~3, ((L + 3) & ~3) + 8):
            for cap in (1, 9, CAP_MAX) if planes * L < 64 * Tt else (9,):      # (the large arrays at one cap: the test stays quick)
                rng = np.random.default_rng([L, pitch, cap % 1000, planes])
                kinds = contents(L, cap, Tt, rng)
                if planes == 1:                                  # one content at a time at the lengths around a load, a wave, a tile
                    sets = [v[None, :] for _, v in kinds] if L in (3, 65, 257, Tt + 1) and pitch > L + 4 else [kinds[7][1][None, :]]
                else:                                            # one content per plane, in turn; the rest random
                    rows = [kinds[g % len(kinds)][1] if g < 2 * len(kinds) else rng.integers(0, min(cap, 4) + 1, L).astype(np.uint32)
                            for g in range(planes)]
                    sets = [np.stack(rows)]
                for values in sets:
                    calls += check_cells(dev, values, pitch, cap, "contents", None if cap < CAP_MAX else [1, 2, cap])
            dev.close()
    assert calls > 400


def test_every_content_by_name(dev, Tt):
    """the contents one by one at a length of two tiles and a tail, with what the rule must give for them said outright"""
    from memo_amd import mems
    L, cap = 2 * Tt + 5, 9
    pitch = (L + 3) & ~3
    kinds = dict(contents(L, cap, Tt, np.random.default_rng(1)))
    assert len(kinds) == 10
    for name, v in kinds.items():
        check_cells(dev, v[None, :], pitch, cap, name)
    d = {name: dev.put(laid_out(v[None, :], pitch, cap)) + 4 * GUARD for name, v in kinds.items()}
    starts = lambda name, **kw: mems.of_cells(d[name], L, pitch, 1, cap=cap, **kw)[0].tolist()             # noqa: E731
    assert starts("all equal below the cap: every cell a start") == list(range(L))                         # the densest output
    assert starts("all equal below the cap: every cell a start", halo=1) == list(range(1, L))
    assert starts("all equal at the cap: one run") == [0] and starts("all equal at the cap: one run", halo=1) == []
    assert starts("falling by one: a single start") == [0] and starts("zeros") == [] and starts("zeros", band=True) == []
    assert starts("rising, then a run at the cap") == list(range(1, cap + 1))
    assert starts("runs at the cap followed by cap - 1") == list(range(0, L, 6))
    assert starts("runs at the cap followed by cap - 2", min_len=cap) == list(range(0, L, 4))
    assert starts("all equal at the cap: one run", band=True, min_len=cap) == [0]                           # open to the end: an odd count
    edge = starts("starts at the edges of loads, waves, tiles and the plane", min_len=cap)
    assert edge == [0, L - 1]
    edge = set(starts("starts at the edges of loads, waves, tiles and the plane"))
    assert {0, 3, 4, 255, 256, 1023, 1024, Tt - 1, Tt, 2 * Tt - 1, 2 * Tt, L - 1} <= edge


def test_more_tiles_than_one_round_of_the_scan(dev, Tt):
    """130 planes of nine tiles: the bases of the later tiles come from the scan's second round, the plane counts from bases beyond it"""
    L, P, cap = 8 * Tt + 5, 130, 9
    assert P * -(-L // Tt) > SCAN_ROUND
    rng = np.random.default_rng(7)
    values = rng.integers(0, 7, (P, L)).astype(np.uint32)
    values[5] = 3                                                # a plane of nothing but starts
    values[6] = 0                                                # and one of none
    values[129] = cap
    assert check_cells(dev, values, (L + 3) & ~3, cap, "scan rounds", [1, 3]) == 6


def test_refusals(dev, Tt):
    from memo_amd._lib import MEMO_EINVAL
    lib = dev.lib
    cells = dev.put(np.full(64, 3, np.uint32))
    counts = (C.c_uint64 * 4)()
    d_s, d_l = C.c_void_p(), C.c_void_p()

    def call(cells=cells, L=16, pitch=16, planes=2, cap=5, min_len=1, key=1, halo=0, starts=C.byref(d_s), lens=C.byref(d_l), counts=counts):
        return lib.memo_mems_dev(cells, L, pitch, planes, cap, min_len, key, halo, starts, lens, counts, 0, None)

    def free():
        for d in (d_s, d_l):
            if d:
                lib.memo_dev_free(0, d)
                d.value = None

    def refused(rc, *words):
        msg = lib.memo_last_error().decode()
        assert rc == MEMO_EINVAL and all(w in msg for w in words), (rc, msg)
        assert not d_s and not d_l                               # nothing was allocated
    assert call() == 0 and list(counts)[:2] == [16, 16] and d_s and d_l
    free()
    assert call(key=2, lens=None) == 0 and list(counts)[:2] == [1, 1] and d_s
    free()
    for off in (4, 8, 12):
        refused(call(cells=cells + off), "16-byte aligned")
    for pitch in (15, 17, 18, 12):
        refused(call(pitch=pitch), "pitch")
    for L in (-1, 2 ** 31 + 1, 2 ** 40):
        refused(call(L=L, pitch=2 ** 41), "2^31")
    for cap in (0, 2 ** 31, 2 ** 32 - 1):
        refused(call(cap=cap), "cap")
    for min_len in (0, 6, 2 ** 32 - 1):
        refused(call(min_len=min_len), "min_len")
    for key in (0, 3, -1):
        refused(call(key=key), "key")
    for halo in (-1, 2):
        refused(call(halo=halo), "halo")
    refused(call(key=2, halo=1), "halo")
    refused(call(planes=-1), "planes")
    refused(call(starts=None), "NULL")
    refused(call(lens=None), "NULL")
    refused(call(counts=None), "NULL")
    refused(call(cells=None), "NULL")
    refused(call(L=2 ** 31, pitch=2 ** 31, planes=2 ** 13, counts=(C.c_uint64 * 2 ** 13)()), "tiles")
    # L == 0 or no planes: nothing to do, nothing launched, NULL cells are fine
    counts[0] = 99
    assert call(cells=None, L=0, pitch=0) == 0 and counts[0] == 0 and not d_s and not d_l
    assert call(cells=None, planes=0, counts=None) == 0 and not d_s
    assert lib.memo_mems_tile() == Tt


# ---------------------------------------------------------------------------------------
# from rows: the golden indexes
# ---------------------------------------------------------------------------------------
LEGAL = sorted({c["index"] for c in G.cases(raises=False)} - {"rnd_negoverlap.parquet"})          # every row has end >= start


def _records(index):
    """[(record, columns, last start, n, the kinds of index the golden cases read the file as)]"""
    cases = [c for c in G.cases(raises=False) if c["index"] == index]
    out = []
    for rec in sorted({G.region(c)[0] for c in cases}):
        cols = G.index_columns(index, rec)
        if len(cols[0]):
            mine = [c for c in cases if G.region(c)[0] == rec]
            out.append((rec, cols, int(cols[0].max()), min(c["n"] for c in mine), {c["membership"] for c in mine}))
    return out


def _modes(n, kinds):
    modes = [dict(threshold=t) for t in sorted({1, max(n // 2, 1), n})] if False in kinds else []
    if True in kinds:
        modes += [dict(membership=True, genome=g) for g in sorted({0, 1, n - 1})] + [dict(membership=True, threshold=max(n // 2, 1))]
    return modes


def _got(path, rec, qs, qe, n, **kw):
    from memo_amd import mems
    r = mems.region_mems(path, f"{rec}:{qs}-{qe}", n, **kw)
    assert r.record == rec and r.starts.dtype == np.int64 and r.ends.dtype == np.int64
    return r


def _same(result, want, note):
    assert np.array_equal(result.starts, want[0]) and np.array_equal(result.ends, want[1]), note


def _stacked(per_genome):
    """[(genome, starts, ends)] -> (starts, ends, genome) as region_mems lays all_genomes out"""
    if not per_genome:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    return (np.concatenate([s for _, s, _ in per_genome]), np.concatenate([e for _, _, e in per_genome]),
            np.concatenate([np.full(len(s), g, np.int32) for g, s, _ in per_genome]))


def _check_every_mode(index, slices=(None,)):
    path = os.path.join(G.GOLD, index)
    checked = 0
    for rec, cols, last, n, kinds in _records(index):
        end = last + 30                                          # past the last row: the tail is at the cap
        windows = [(0, end), (last // 3, last // 2 + 1), (last // 2, end)]
        for mode in _modes(n, kinds):
            for cap in (CAP_MAX, 31):
                for (qs, qe), min_len in zip(windows, (1, 1, 3)):
                    want = mems_oracle.matches(*cols, qs, qe, cap, n, min_len=min_len, **mode)
                    _same(_got(path, rec, qs, qe, n, cap=cap, min_len=min_len, **mode), want, (index, rec, mode, cap, qs, qe, min_len))
                    checked += 1
            for min_len in (1, 8):
                want = mems_oracle.union(*cols, last // 3, end, n, min_len=min_len, **mode)
                _same(_got(path, rec, last // 3, end, n, union=True, min_len=min_len, **mode), want, (index, rec, mode, "union", min_len))
        if True in kinds:
            for cap, (qs, qe), min_len in ((CAP_MAX, windows[0], 1), (31, windows[1], 1), (31, windows[2], 4)):
                want = _stacked(mems_oracle.all_matches(*cols, qs, qe, cap, n, min_len=min_len))
                for step in slices:
                    r = _got(path, rec, qs, qe, n, membership=True, all_genomes=True, cap=cap, min_len=min_len, slice_positions=step)
                    _same(r, want, (index, rec, "-a", cap, qs, qe, step))
                    assert r.genome.dtype == np.int32 and np.array_equal(r.genome, want[2])
            per = [(g, *mems_oracle.union(*cols, 1, end, n, min_len=3, membership=True, genome=g)) for g in range(1, n)]
            want = _stacked(per)
            for step in slices:
                r = _got(path, rec, 1, end, n, membership=True, all_genomes=True, union=True, min_len=3, slice_positions=step)
                _same(r, want, (index, rec, "-a -u", step))
                assert np.array_equal(r.genome, want[2])
    return checked


@pytest.mark.parametrize("index", LEGAL)
def test_every_mode_against_the_oracle(memo, Tt, index):
    assert _check_every_mode(index, (None, Tt + 1)) >= 18


def test_rows_with_end_before_start_against_the_oracle_only(memo, Tt):
    cols = G.index_columns("rnd_negoverlap.parquet", "chrN")
    assert (cols[1] < cols[0]).any()
    assert _check_every_mode("rnd_negoverlap.parquet", (None, 700)) >= 42


@pytest.mark.parametrize("index", LEGAL)
def test_all_genomes_is_the_single_genome_lists_stacked(memo, index):
    path = os.path.join(G.GOLD, index)
    for rec, cols, last, n, kinds in _records(index):
        if True not in kinds:
            continue
        qs, qe = last // 4, last + 10
        for cap, min_len in ((CAP_MAX, 1), (31, 2)):
            every = _got(path, rec, qs, qe, n, membership=True, all_genomes=True, cap=cap, min_len=min_len)
            assert (np.diff(every.genome) >= 0).all() and every.genome.min(initial=1) >= 1 and every.genome.max(initial=1) <= n - 1
            for g in sorted({1, 2, n // 2, n - 1} - {0}):
                one = _got(path, rec, qs, qe, n, membership=True, genome=g, cap=cap, min_len=min_len)
                mine = every.genome == g
                assert one.genome is None and np.array_equal(every.starts[mine], one.starts) and np.array_equal(every.ends[mine], one.ends), (index, g)


def test_the_membership_index_gives_what_the_conservation_index_gives(memo):
    """the example pair: `-m -t T` == `-t T`, as lists and as bytes"""
    from memo_amd import mems
    cons, memb = os.path.join(G.GOLD, "example_cons.parquet"), os.path.join(G.GOLD, "example_memb.parquet")
    for t in (1, 2, 3, 4, 5):
        for qs, qe in ((0, 20), (0, 26), (7, 19)):
            for kw in (dict(), dict(cap=4), dict(min_len=3), dict(union=True, min_len=3)):
                a = mems.region_mems(cons, f"ref_1:{qs}-{qe}", 5, threshold=t, **kw)
                b = mems.region_mems(memb, f"ref_1:{qs}-{qe}", 5, threshold=t, membership=True, **kw)
                _same(b, (a.starts, a.ends), (t, qs, qe, kw))
                assert mems.emit(a).tobytes() == mems.emit(b).tobytes()


@pytest.mark.parametrize("index", LEGAL)
def test_windows_laid_end_to_end_are_the_whole(memo, index):
    path = os.path.join(G.GOLD, index)
    for rec, cols, last, n, kinds in _records(index):
        end = last + 20
        for mode in _modes(n, kinds)[1::2] + ([dict(membership=True, all_genomes=True)] if True in kinds else []):
            for cap in (CAP_MAX, 31):
                whole = _got(path, rec, 0, end, n, cap=cap, **mode)
                for cut in (end // 3, end // 3 + 1, end // 2):
                    left, right = _got(path, rec, 0, cut, n, cap=cap, **mode), _got(path, rec, cut, end, n, cap=cap, **mode)
                    if whole.genome is None:
                        joined = (np.concatenate([left.starts, right.starts]), np.concatenate([left.ends, right.ends]))
                    else:                                        # per genome: the left window's, then the right one's
                        order = np.argsort(np.concatenate([left.genome, right.genome]), kind="stable")
                        joined = tuple(np.concatenate(pair)[order] for pair in ((left.starts, right.starts), (left.ends, right.ends)))
                    _same(whole, joined, (index, rec, mode, cap, cut))


MEMBERSHIP = [i for i in LEGAL if any(c["membership"] for c in G.cases(raises=False) if c["index"] == i)]


@pytest.mark.parametrize("index", MEMBERSHIP)
def test_all_genomes_does_not_depend_on_the_slices(memo, Tt, index):
    """slices of 1, 2, 7 and a tile and one positions: every slice but the leftmost takes its left neighbour from one more cell"""
    path = os.path.join(G.GOLD, index)
    for rec, cols, last, n, kinds in _records(index):
        if True not in kinds:
            continue
        for qs, qe in ((0, min(last + 5, 40)), (last // 2, min(last // 2 + 33, last + 5))):   # (short: a slice of 1 reads the file once per position)
            for kw in (dict(cap=CAP_MAX), dict(cap=31, min_len=2), dict(union=True, min_len=3)):
                whole = _got(path, rec, qs, qe, n, membership=True, all_genomes=True, **kw)
                assert len(whole.starts) > 0 and len(MEMBERSHIP) == 6
                for step in (1, 2, 7, Tt + 1):
                    r = _got(path, rec, qs, qe, n, membership=True, all_genomes=True, slice_positions=step, **kw)
                    _same(r, (whole.starts, whole.ends), (index, rec, qs, qe, kw, step))
                    assert np.array_equal(r.genome, whole.genome)
                # the threshold-th largest is selected slice by slice into one buffer: no slice logic after it
                t = max(n // 2, 1)
                whole = _got(path, rec, qs, qe, n, membership=True, threshold=t, **kw)
                _same(_got(path, rec, qs, qe, n, membership=True, threshold=t, slice_positions=7, **kw), (whole.starts, whole.ends), (index, rec, kw))


@pytest.mark.parametrize("index", LEGAL)
def test_the_list_expands_to_memo_maxk_s_vector(memo, index):
    """lossless wherever no value is the cap"""
    from memo_amd import maxk
    path = os.path.join(G.GOLD, index)
    expanded = 0
    for rec, cols, last, n, kinds in _records(index):
        for mode in _modes(n, kinds):
            if mode.get("membership") and "threshold" in mode:
                continue                                         # (`memo maxk` has no such mode: the oracle test covers it)
            pred = {k: v for k, v in mode.items() if k != "membership"}
            whole = maxk.region_maxk(path, f"{rec}:0-{last}", n, **pred)
            open_at = np.flatnonzero(whole == CAP_MAX)           # from the first position that no row bounds on, the list is "at least"
            bounded = int(open_at[0]) if len(open_at) else last
            if bounded < 3:
                continue
            for qs, qe in ((0, bounded), (bounded // 3, bounded - 1)):
                v = maxk.region_maxk(path, f"{rec}:{qs}-{qe}", n, **pred).astype(np.int64)
                r = _got(path, rec, qs, qe, n, **mode)
                assert not (v == CAP_MAX).any()
                first = int(r.starts[0]) - qs                    # (the positions before the window's first start belong to a match of the window before)
                assert first == 0 or qs > 0
                assert np.array_equal(mems_oracle.expand(r.starts, r.ends, qs, qe)[first:], v[first:]), (index, rec, mode, qs, qe)
                expanded += 1
    assert expanded >= 2


@pytest.mark.parametrize("index", LEGAL)
def test_the_covered_bases_are_the_widened_band_runs_of_memo_regions(memo, index):
    from memo_amd import mems, regions
    path = os.path.join(G.GOLD, index)
    for rec, cols, last, n, kinds in _records(index):
        if False not in kinds:
            continue
        for t in sorted({1, max(n // 2, 1), n}):
            for qs, qe in ((0, last + 12), (last // 3, last // 2 + 3)):
                for min_len in (1, 3, 8, 31):
                    runs = regions.region_runs(path, f"{rec}:{qs}-{qe}", min_len, n, lo=t)
                    b, e = regions.band_intervals(runs.starts, runs.L)
                    want = mems.merge(b + qs, e + qs + min_len - 1)
                    _same(_got(path, rec, qs, qe, n, threshold=t, union=True, min_len=min_len), want, (index, rec, t, qs, qe, min_len))


def test_a_window_past_2_to_the_32(memo, Tt, tmp_path):
    """a Parquet file of several row groups, three copies of a record side by side and shifted past 2^32: every mode against the oracle,
    and the planes in slices of a tile and one"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    s, e, a = G.index_columns("rnd_n8.parquet", "chr1")
    span = int(e.max()) + 1
    D = 2 ** 32 + 999
    s, e, a = (np.concatenate([c + k * span * shift for k in range(3)]) for c, shift in ((s, 1), (e, 1), (a, 0)))
    path = str(tmp_path / "far.parquet")
    pq.write_table(pa.table({"f0": pa.array(["chr1"] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": a}), path, row_group_size=3001)
    assert pq.ParquetFile(path).metadata.num_row_groups > 5
    lo, hi = 100, int(s.max()) - 100
    assert hi - lo > Tt + 1
    far = (s + D, e + D, a)
    for mode in (dict(threshold=8), dict(threshold=3), dict(membership=True, genome=3), dict(membership=True, threshold=4)):
        for kw in (dict(cap=CAP_MAX), dict(cap=50, min_len=5)):
            want = mems_oracle.matches(s, e, a, lo, hi, kw["cap"], 8, min_len=kw.get("min_len", 1), **mode)
            r = _got(path, "chr1", lo + D, hi + D, 8, **mode, **kw)
            _same(r, (want[0] + D, want[1] + D), (mode, kw))
            assert len(want[0]) > 0 and r.starts.min() > 2 ** 32
        want = mems_oracle.union(*far, lo + D, hi + D, 8, min_len=6, **mode)
        _same(_got(path, "chr1", lo + D, hi + D, 8, union=True, min_len=6, **mode), want, (mode, "union"))
    want = _stacked(mems_oracle.all_matches(*far, lo + D, hi + D, 40, 8, min_len=2))
    for step in (None, Tt + 1, 1000):
        r = _got(path, "chr1", lo + D, hi + D, 8, membership=True, all_genomes=True, cap=40, min_len=2, slice_positions=step)
        _same(r, want, ("-a", step))
        assert np.array_equal(r.genome, want[2])
    from memo_amd import mems
    cons = os.path.join(G.GOLD, "example_cons.parquet")
    r = mems.region_mems(cons, "nochr:0-5", 5, cap=9)            # a record without rows: one match of the cap
    assert (r.starts.tolist(), r.ends.tolist()) == ([0], [9])
    assert mems.region_mems(cons, "nochr:3-5", 5, cap=9).starts.tolist() == []
    assert mems.region_mems(cons, "ref_1:5-5", 5).starts.tolist() == []
    with pytest.raises(OSError):
        mems.region_mems(str(tmp_path / "no.parquet"), "chr1:0-20", 8)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def _bed(pairs, genome=None):
    rows = [p.split("-") for p in pairs.split()]
    return mems_oracle.text("ref_1", [int(b) for b, _ in rows], [int(e) for _, e in rows], genome)


EXAMPLE_T5 = "0-3 2-5 4-6 5-7 6-8 7-11 10-13 12-14 13-16 15-18 17-20 19-21"
EXAMPLE_T3 = "0-5 2-6 4-7 5-9 6-11 7-13 10-14 12-15 13-16 14-17 15-20 17-21 19-22"
EXAMPLE_G1 = "0-3 2-5 4-7 6-8 7-11 10-13 12-16 15-18 17-20 19-21"
EXAMPLE_G4 = "0-3 1-4 2-6 5-9 7-11 9-12 10-14 13-16 14-18 16-19 17-21 19-22"


def _run(tmp_path, index, *flags, region="ref_1:0-20"):
    out = str(tmp_path / "m.bed")
    r = _memo("mems", "-b", index, "-n", "5", "-r", region, "-o", out, *flags)
    assert (r.returncode, r.stdout) == (0, b"MEMO - mems\n"), (flags, r.stderr)
    return open(out, "rb").read()


def test_the_worked_example_in_process(memo):
    """the bytes of every list of DESIGN.md 10.13, through region_mems and emit (the command line's own two calls)"""
    from memo_amd import mems
    cons, memb = os.path.join(G.GOLD, "example_cons.parquet"), os.path.join(G.GOLD, "example_memb.parquet")
    text = lambda index, region="ref_1:0-20", **kw: mems.emit(mems.region_mems(index, region, 5, **kw)).tobytes()     # noqa: E731
    assert text(cons) == _bed(EXAMPLE_T5) == text(cons, threshold=5) and _bed(EXAMPLE_T5).count(b"\n") == 12
    assert text(cons, min_len=3) == _bed("0-3 2-5 7-11 10-13 13-16 15-18 17-20")
    assert text(cons, union=True, min_len=3) == _bed("0-5 7-20")
    assert text(cons, threshold=3) == _bed(EXAMPLE_T3) and _bed(EXAMPLE_T3).count(b"\n") == 13
    assert text(cons, threshold=3, union=True, min_len=3) == _bed("0-22")
    assert text(memb, membership=True) == _bed(EXAMPLE_T5) == text(memb, membership=True, threshold=5)
    assert text(memb, membership=True, threshold=3) == _bed(EXAMPLE_T3)
    assert text(memb, membership=True, genome=1) == _bed(EXAMPLE_G1) and text(memb, membership=True, genome=4) == _bed(EXAMPLE_G4)
    assert text(memb, membership=True, genome=0, cap=12) == b"ref_1\t0\t12\n"     # the pivot has no rows: one match of the cap
    cols = G.index_columns("example_cons.parquet", "ref_1")
    assert text(cons, cap=2) == mems_oracle.text("ref_1", *mems_oracle.matches(*cols, 0, 20, 2, 5, threshold=5))
    assert text(cons, "ref_1:6-9") == _bed("6-8 7-11")                              # the matches that start in it, not clipped
    assert text(cons, "ref_1:5-5") == b"" == text(memb, "ref_1:5-5", membership=True, all_genomes=True)


def test_cli_on_the_conservation_example(memo, tmp_path):
    cons = os.path.join(G.GOLD, "example_cons.parquet")
    assert _run(tmp_path, cons) == _bed(EXAMPLE_T5)
    assert _run(tmp_path, cons, "-t", "3", "-l", "3") == _bed("0-5 2-6 4-7 5-9 6-11 7-13 10-14 12-15 13-16 14-17 15-20 17-21 19-22")
    assert _run(tmp_path, cons, "-u", "-l", "3") == _bed("0-5 7-20")
    assert _run(tmp_path, cons, region="ref_1:5-5") == b""                          # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["m.bed"]                                # written beside its name and renamed
    never = str(tmp_path / "never.bed")
    r = _memo("mems", "-b", cons, "-n", "5", "-r", "ref_1:20-0", "-o", never)
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)


def test_cli_on_the_membership_example(memo, tmp_path):
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    assert _run(tmp_path, memb, "-m", "-t", "3") == _bed(EXAMPLE_T3)
    assert _run(tmp_path, memb, "-m", "-d", "4") == _bed(EXAMPLE_G4)
    every = _run(tmp_path, memb, "-m", "-a")
    cols = G.index_columns("example_memb.parquet", "ref_1")
    want = b"".join(mems_oracle.text("ref_1", s, e, g) for g, s, e in mems_oracle.all_matches(*cols, 0, 20, CAP_MAX, 5))
    assert every == want and every.startswith(_bed(EXAMPLE_G1, 1)) and every.endswith(_bed(EXAMPLE_G4, 4)) and every.count(b"\n") == 39
    per = [(g, *mems_oracle.union(*cols, 0, 20, 5, min_len=3, membership=True, genome=g)) for g in range(1, 5)]
    assert _run(tmp_path, memb, "-m", "-a", "-u", "-l", "3") == b"".join(mems_oracle.text("ref_1", s, e, g) for g, s, e in per)
    assert _run(tmp_path, memb, "-m", "-a", region="ref_1:5-5") == b""
