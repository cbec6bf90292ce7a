"""The row block of the membership planes kernels (memo_sweep_memb.hip: planes_put, one hand-written block per reach MW of a run -- the words
a run of n = k - 1 - overlap bits can extend past its first: 0 for k - 1 <= 31, 2 up to 65, 3 up to 97, 4 up to 129, 8 up to 255 -- with and
without the group skew SK, for 64 and 256 threads, on row formats 4 and 12 and on the dense rows), one run at a time.  Hand-made rows put
every n from -17 to k - 1 at every start residue mod 32 alone on the words of its genome's plane row: no other row of the genome shares or
neighbours a word of the run, so a word the row block fails to write, or one it writes too far, shows in the result -- in the random piles
of tests/test_gpu_parity.py a neighbour of the same genome as a rule covers it, the result being an OR.  Every result is compared bit for
bit with the oracle, and every counted query is one whose plan, as the launcher recorded it (memo_debug_last_membership: algorithm, tile
width, threads, MW, SK, result words per launch), is the one the test names: a launcher that routed these shapes elsewhere would be seen."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPT_BUILD_COST_PCT = 3
STRIDE = 64            # positions from one slot to the next (a multiple of 32: a row's start residue is its own)
_POP16 = None


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture
def ab(memo):
    """the recorded plan and the kernel-shape switches are exported by libmemo_amd_ab.so only"""
    from memo_amd import _lib
    _lib.use_ab(True)
    yield _lib
    _lib.use_ab(False)


def _mw(k):
    """the row block of k, as memo_sweep_memb.hip documents its blocks"""
    km1 = k - 1
    return 0 if km1 <= 31 else 2 if km1 <= 65 else 3 if km1 <= 97 else 4 if km1 <= 129 else 8


def _set_bits(a):
    global _POP16
    if _POP16 is None:
        v = np.arange(1 << 16, dtype=np.uint32)
        _POP16 = sum((v >> b) & 1 for b in range(16)).astype(np.uint8)
    return int(_POP16[np.ascontiguousarray(a).view(np.uint16)].sum(dtype=np.int64))


def _alone(k, n_docs, residues=range(32), annot_step=1, fillers=None):
    """start-sorted int64 columns: one row for every n of -17 .. k - 1 at every start residue, end - start = k - 1 - n (_rows of
    tests/test_three_block_rows.py).  Row i lies at STRIDE * slot + its residue, the slots dealt so that neighbouring n and residues do
    not sit side by side; its annot is slot * annot_step mod n_docs, so two rows of one genome are n_docs slots (2048 positions or more)
    apart, and the annots cycle through every column: column 0, bit 31 of a word, bit 0 of the next, the last column of a partial word,
    every 32-genome group.  fillers: "dense" one more row per position, "half" one for every second slot, each with an overlap of 255,
    which writes at no k <= 256.  Returns (s, e, o), the pivot's length and the number of bits the rows clear."""
    residues = np.asarray(list(residues), np.int64)
    ns = np.arange(-17, k, dtype=np.int64)
    n = np.repeat(ns, len(residues))
    r = np.tile(residues, len(ns))
    i = np.arange(len(n), dtype=np.int64)
    mult = 37 if math.gcd(37, len(n)) == 1 else 41                 # (k = 131: 37 divides the number of rows)
    slot = (i * mult) % len(n)
    assert len(np.unique(slot)) == len(n)
    base = STRIDE * ((k - 1 + STRIDE - 1) // STRIDE + 1)           # (the first run begins inside the pivot)
    start = base + STRIDE * slot + r
    annot = (slot * annot_step) % n_docs
    L = int(start.max()) + 64
    # two rows of the same genome: k - 1 + 64 positions apart or more -- a run and the words next to it are its row's alone
    by = np.lexsort((start, annot))
    same = np.diff(annot[by]) == 0
    assert not same.any() or np.diff(start[by])[same].min() >= k - 1 + 64
    ov = k - 1 - n
    if fillers:
        fs = np.arange(L, dtype=np.int64) if fillers == "dense" else base + STRIDE * np.arange(0, len(n), 2, dtype=np.int64) + 40
        start, ov, annot = (np.concatenate(p) for p in ((start, fs), (ov, np.full(len(fs), 255, np.int64)), (annot, fs % n_docs)))
    order = np.argsort(start, kind="stable")
    s, e, o = start[order], (start + ov)[order], annot[order]
    return (s, e, o), L, int(np.maximum(n, 0).sum())


def _want(oracle, rows, qs, qe, k, n_docs):
    return oracle.membership(*oracle.filter_rows(*rows, qs, qe, k), qs, qe, k, n_docs, literal=False)


def _case(oracle, k, n_docs, windows=None, **kw):
    """rows, windows and the oracle's results; the rows are alone: in the whole pivot's result the cleared bits are the rows' own n,
    none shared, none lost at an edge.  No device call has happened yet when this asserts."""
    rows, L, cleared = _alone(k, n_docs, **kw)
    windows = windows(L) if windows else [(0, L), (67, L - 129)]
    wants = [_want(oracle, rows, qs, qe, k, n_docs) for qs, qe in windows]
    assert windows[0] == (0, L) and L * n_docs - _set_bits(wants[0]) == cleared, (k, n_docs)
    return rows, L, windows, wants


def _ask(ix, windows, wants, k, n_docs, expect, what):
    """every window against the oracle; returns the number of queries whose recorded plan is `expect` (a dict of the plan's fields)"""
    counted = 0
    for (qs, qe), want in zip(windows, wants):
        got = ix.membership(qs, qe, k, n_docs)
        plan = ix.debug_last_membership()
        bad = np.argwhere(got != want)
        assert not len(bad), (what, k, n_docs, qs, qe, plan, len(bad), bad[0].tolist(), hex(int(got[tuple(bad[0])])),
                              hex(int(want[tuple(bad[0])])))
        assert {f: plan[f] for f in expect} == expect, (what, k, n_docs, qs, qe, plan)
        counted += 1
    return counted


def _planes(k, nw, threads=256):
    return {"algorithm": 4, "mw": _mw(k), "sk": int(nw in (4, 8, 16)), "threads": threads, "slice": nw}


@pytest.mark.parametrize("k", (2, 17, 32, 33, 66, 67, 98, 99, 130, 131, 200, 256))
def test_every_run_alone(k, memo, ab, oracle):
    """both sides of every reach boundary of the launcher (k - 1 = 31 | 32, 65 | 66, 97 | 98, 129 | 130), the smallest k and the largest: the
    planes kernel on the 4-byte rows with one result word (format 4, no skew), four (format 4, skew), ten (format 12, no skew) and sixteen
    (format 12, skew), buckets of 1 and 32 positions, 64 and 256 threads; then the same windows by the runs kernel on the packed rows
    and by the doubling kernel on the int64 columns.  n <= 0 writes nothing: the row block's v_cmpx "this row writes" test, and at
    k = 256 the saturated 8-bit length.  Windows: the pivot, and one that starts and ends off the 32-position and the 4-word rasters."""
    cases = [(n_docs, _case(oracle, k, n_docs)) for n_docs in (32, 128, 300, 512)]
    counted = planned = 0
    for n_docs, (rows, L, windows, wants) in cases:
        nw = (n_docs + 31) // 32
        for shift in (0, 5):
            with memo.DeviceIndex.from_host(*rows, bucket_shift=shift) as ix:
                ix.pack()
                inf = ix.info()
                assert inf["packed_format"] == (4 if n_docs <= 255 else 12) and inf["max_annot"] < n_docs, inf
                for waves in (1, 4):
                    ix.debug_set_tuning(0, waves, 4)
                    counted += _ask(ix, windows, wants, k, n_docs, _planes(k, nw, 64 * waves), ("planes", shift))
                    assert ix.info()["last_sweep"] == 7
                    ix.debug_set_tuning(0, waves, 3)
                    counted += _ask(ix, windows, wants, k, n_docs, {"algorithm": 3, "mw": -1, "threads": 64 * waves}, ("runs", shift))
                    ix.debug_set_tuning(0, waves, 2, 1)
                    counted += _ask(ix, windows, wants, k, n_docs, {"algorithm": 2, "mw": -1, "threads": 64 * waves},
                                    ("doubling", shift))
                    planned += 3 * len(windows)
                ix.check()
    assert counted == planned == 4 * 2 * 2 * 3 * 2


@pytest.mark.parametrize("k", (2, 17, 32, 33, 64))
def test_every_run_alone_dense_rows(k, memo, ab, oracle):
    """sweep_membership_planes3_kernel: the same rows and a filler per position (the dense rows answer an index of a row per position
    or more; a filler's overlap of 255 writes at no k), one, four and eight result words, buckets of 1 and 32 positions; once with the
    rows that can never write at k <= 64 left out of the dense rows (the library's way) and once with them kept inside
    (memo_debug_dense_keep_all)."""
    cases = [(n_docs, _case(oracle, k, n_docs, fillers="dense")) for n_docs in (32, 128, 255)]
    counted = planned = 0
    for keep_all in (0, 1):
        ab.lib().memo_debug_dense_keep_all(keep_all)
        try:
            for n_docs, (rows, L, windows, wants) in cases:
                nw = (n_docs + 31) // 32
                for shift in (0, 5):
                    with memo.DeviceIndex.from_host(*rows, bucket_shift=shift) as ix:
                        ix.pack(keep_wide=False)
                        ix.pack_dense(keep_packed=False)
                        inf = ix.info()
                        assert inf["dense_rows"] == 1 and inf["max_annot"] < n_docs, inf
                        assert (inf["dense_row_count"] == len(rows[0])) == bool(keep_all), (keep_all, inf)
                        expect = {"algorithm": 5, "mw": 0 if k - 1 <= 31 else 2, "sk": int(nw in (4, 8, 16)), "threads": 256, "slice": nw}
                        for qw in zip(windows, wants):
                            counted += _ask(ix, *[[x] for x in qw], k, n_docs, expect, ("dense", shift, keep_all))
                            assert ix.info()["last_sweep"] == 6
                            planned += 1
                        ix.check()
        finally:
            ab.lib().memo_debug_dense_keep_all(0)
    assert counted == planned == 2 * 3 * 2 * 2


@pytest.mark.parametrize("k", (31, 67, 120))
def test_runs_alone_through_a_view(k, memo, ab, oracle):
    """the planes kernel on the k-class view of the 4-byte words (memo_view.hip: packed_rows_for; caps 30, 80 and 128 here): the view
    leaves out the fillers and the rows whose overlap is at or above its cap, and keeps the rows with n <= 0 below it (k = 67: n of -13
    .. 0, k = 120: -8 .. 0), which write nothing.  The query that builds the view, the next one on it, and one on all the rows."""
    counted = 0
    for n_docs in (128, 300):
        (s, e, o), L, windows, wants = _case(oracle, k, n_docs, fillers="half")
        assert 4 * int((e - s >= k - 1).sum()) >= len(s)             # a quarter of the rows or more cannot write
        nw = (n_docs + 31) // 32
        for shift in (0, 5):
            with memo.DeviceIndex.from_host(s, e, o, bucket_shift=shift) as ix:
                ix.pack()
                ix.set_option(OPT_BUILD_COST_PCT, 0)
                for no_views in (False, False, True):
                    ix.debug_no_views(no_views)
                    counted += _ask(ix, windows[:1], wants[:1], k, n_docs, _planes(k, nw), ("view", shift, no_views))
                    read = ix.info()["last_rows_read"]
                    assert (read == len(s)) if no_views else (0 < read < len(s)), (k, no_views, read, len(s))
                    counted += _ask(ix, windows[1:], wants[1:], k, n_docs, _planes(k, nw), ("view", shift, no_views))
                ix.check()
    assert counted == 2 * 2 * 3 * 2


def _edge_rows(k, n_docs, tw, seed):
    """rows with a start at every position within k - 1 + 40 of each of the first four tile boundaries; n seeded, every n of 1 .. k - 1
    present; annots cycle.  These rows may touch: they are about the halo, the rows whose start lies past the tile's end and the pitch
    of the plane rows"""
    rng = np.random.default_rng(seed)
    reach = k - 1 + 40
    # (sixteen words at k = 256: a tile of 256 positions, narrower than the reach -- the neighbourhoods run into one another)
    start = np.unique(np.concatenate([t * tw + np.arange(-reach, reach + 1, dtype=np.int64) for t in range(1, 5)]))
    start = start[start >= 1]
    n = rng.integers(1, k, len(start))
    n[:k - 1] = rng.permutation(np.arange(1, k))
    return start, start + (k - 1 - n), np.arange(len(start), dtype=np.int64) % n_docs


@pytest.mark.parametrize("k", (31, 67, 256))
def test_runs_at_tile_edges(k, memo, ab, oracle):
    """one, three, four and sixteen result words (three: the copy-out of planes_transpose_store takes its nw % 4 != 0 path), buckets of
    1, 2 and 32 positions; the tile width is the one the launcher recorded for a first query.  Windows: the pivot, one off both rasters,
    and around every boundary one across it, one that begins just behind it, one that ends just before it and one of two positions
    on it -- the copy-out's head with q negative by up to 3, its scalar tail, windows of fewer than four result words"""
    counted = planned = 0
    for n_docs in (32, 96, 128, 512):
        nw = (n_docs + 31) // 32
        for shift in (0, 1, 5):
            probe = np.array([100], np.int64)
            with memo.DeviceIndex.from_host(probe, probe + 1, probe * 0 + n_docs - 1, bucket_shift=shift) as ix:
                ix.pack()
                ix.membership(0, 64, k, n_docs)
                plan = ix.debug_last_membership()
                assert plan["algorithm"] == 4, plan
                tw = plan["tile_width"]
            s, e, o = _edge_rows(k, n_docs, tw, 1000 * k + n_docs)
            L = 5 * tw
            windows = [(0, L), (3, L - 5)]
            for t in range(tw, 5 * tw, tw):
                windows += [(t - 37, t + 41), (t + 1, t + 42), (t - 39, t - 2), (t - 1, t + 1)]
            wants = [_want(oracle, (s, e, o), qs, qe, k, n_docs) for qs, qe in windows]
            with memo.DeviceIndex.from_host(s, e, o, bucket_shift=shift) as ix:
                ix.pack()
                assert ix.info()["max_annot"] < n_docs
                counted += _ask(ix, windows, wants, k, n_docs, dict(_planes(k, nw), tile_width=tw), ("edges", shift))
                planned += len(windows)
                ix.check()
    assert counted == planned == 4 * 3 * 18


@pytest.mark.parametrize("k", (31, 131, 256))
def test_long_runs_in_sliced_genome_words(k, memo, ab, oracle):
    """2100 genomes are 66 result words: the runs kernel sweeps them in two slices, of 64 words and of 2, on the packed rows and on the
    int64 columns.  At k = 131 and 256 its whole-word store loop w0 + 1 .. w1 - 1 runs with up to three and seven words.  The same
    generator on the start residues 0, 1 and 31 (the result stays below 64 MB); the annots step by 67, so that the rows reach both
    slices and no genome has two."""
    n_docs = 2100
    rows, L, windows, wants = _case(oracle, k, n_docs, residues=(0, 1, 31), annot_step=67)
    assert rows[2].max() >= 2048 and len(np.unique(rows[2])) == len(rows[2])
    counted = 0
    with memo.DeviceIndex.from_host(*rows) as ix:
        ix.pack()
        assert ix.info()["packed_format"] == 12
        for source in (0, 1):
            ix.debug_set_tuning(0, 0, 3, source)
            counted += _ask(ix, windows, wants, k, n_docs, {"algorithm": 3, "mw": -1, "sk": 0, "slice": 64}, ("sliced", source))
        ix.check()
    assert counted == 4
