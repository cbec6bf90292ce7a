"""The decode of the run copy (memo_sweep_runs.hip) where a lane decodes P positions from dwords it loads itself and a wave takes 64 P
positions a turn, counted from the copy's first position p0: windows at every offset around a turn boundary, inside one lane, of exactly
one turn; the copy's two ends, which no longer fall on a wave's boundary; values at the longest offsets a group can hold.

The index is the hand-made one of tests/test_run_copy_gpu.py (its first row reaches below the index's first bucket, so p0 = 32 * 39 is on
no raster of turns) with, behind it:
  - four consecutive groups of 256 runs each (1024 values in 1024 positions) that begin a multiple of 1024 positions from p0 -- on a turn
    boundary for P = 8 and 16 -- and a second such set shifted by one group; the orders alternate and include the largest;
  - right after the first set one run over several buckets (offsets that stand still after the longest ones);
  - buckets of rows that win nowhere, so that the deciding copy (and with it the run copy) is worth making;
  - a last group that is full of runs (255 starts; the index's last position belongs to no row and is the 256th), in a copy of 4 n + 1
    groups: the last turn is half (P = 8) or a quarter (P = 16) inside the copy.
Every window is compared three ways, byte for byte: the decode, the oracle's closed form, the same query with MEMO_OPT_VIEW_RUNS 0."""
import numpy as np
import pytest

from tests.test_deciding_rows_gpu import _hand_index
from tests.test_run_copy_gpu import GROUP, N_DOCS, _check_copy, _hand_rows, _three_ways, _until_run_copy

P = 8                   # memo_sweep_runs.hip: kDecodeP, positions a lane (test_windows_three_ways checks it: last_pick.width = 16 turns)
TURN = 64 * P           # positions a wave decodes a turn
K = 31
LOSER_BUCKETS = 150


@pytest.fixture(scope="module")
def memo():
    """the package on the A/B library, as tests/test_run_copy_gpu.py sets it up"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    _lib.use_ab(True)
    yield memo_amd
    _lib.use_ab(False)


def _decode_rows(k, D=0):
    """(start, n, order, {name: position}) -- the rows of the module's docstring, moved by D (a multiple of every raster)"""
    start, n, order, _ = _hand_rows(k)
    p0 = 32 * ((int(start.min()) >> 5) - 1)
    rows, where = [], {"p0": p0 + D}

    def full_group(at):                                               # 256 runs: position at + i is covered by a row of its own
        rows.extend((at + i + 1, 1, 3 + i % 2 + (96 if i % 64 == 0 else 0)) for i in range(256))
    # The cases below are rows that all win, and the class gets a deciding copy -- and with it a run copy -- only if that copy spares a
    # fifth of the live copy's groups of six (tests/test_deciding_rows_gpu.py): buckets of two winners and sixteen rows that win nowhere
    # and that neither winner contains, three groups of the live copy and one of the deciding copy each
    top = (int(start.max()) + 64 + 63) // 64 * 64
    for j in range(LOSER_BUCKETS):
        at = top + 64 * j
        rows.extend([(at + 10, 10, 1), (at + 20, 10, 1)])
        rows.extend((at + first + i, m, 50 + 4 * c + i) for c, (first, m) in enumerate(((12, 6), (12, 8), (13, 10), (14, 12))) for i in range(4))
    A = p0 + ((top + 64 * LOSER_BUCKETS + 64 - p0 + 1023) // 1024 + 1) * 1024
    for g in range(4):
        full_group(A + 256 * g)
    rows.extend((A + 1024 + 24 * j, 24, 6) for j in (1, 2, 3, 4))     # [A + 1024, A + 1120): one run through three buckets
    B = A + 2048 + 256
    for g in range(4):
        full_group(B + 256 * g)
    E = A + 4096                                                      # the copy's last group: starts up to E + 255, nothing behind them
    rows.extend((E + i + 1, 1, 3 + i % 2 + (96 if i % 64 == 0 else 0)) for i in range(255))
    where.update({"on the raster": A + D, "one run": A + 1024 + D, "a group off": B + D, "the last group": E + D, "end": E + 256 + D})
    s2, n2, o2 = (np.array(col, np.int64) for col in zip(*rows))
    return np.concatenate([start, s2]) + D, np.concatenate([n, n2]), np.concatenate([order, o2]), where


def _rows_to_the_last_start(start, n, k, annot):
    """tests/test_run_copy_gpu.py: _rows, but the rows of overlap 40 end with the last start: the copy ends in the group that holds it"""
    start, n, annot = (np.asarray(a, np.int64) for a in (start, n, annot))
    fill = np.arange(int(start.min()), int(start.max()) + 1, dtype=np.int64)
    s = np.concatenate([start, fill])
    ov = np.concatenate([k - 1 - n, np.full(len(fill), 40, np.int64)])
    o = np.concatenate([annot, np.ones(len(fill), np.int64)])
    order = np.argsort(s, kind="stable")
    return s[order], (s + ov)[order], o[order]


def _check_shape(ix, s, e, o, k, where):
    """the copy is the twin's, and has the buckets the cases are about"""
    b0, masks, runs = _check_copy(ix, s, e, o, k)
    p0 = where["p0"]
    assert 32 * b0 == p0 and masks[0] != 1 and (p0 - (p0 >> 32 << 32)) % TURN != 0
    c = np.array([bin(int(m)).count("1") for m in masks])
    groups = len(masks) // GROUP
    assert groups % 4 == 1 and 32 * len(masks) == where["end"] - p0                          # the last turn is partly outside the copy
    for name, turn_offset in (("on the raster", 0), ("a group off", 256)):
        b = (where[name] - p0) >> 5
        assert (where[name] - p0) % 1024 == turn_offset and (c[b:b + 4 * GROUP] == 32).all(), name
    b = (where["one run"] - p0) >> 5
    assert list(masks[b:b + 3]) == [1, 1, 1] and c[b - 1] == 32
    assert (c[-GROUP:] == 32).all()                                                          # the last group is full of runs
    # a workgroup decodes 16 turns, and one that lies wholly inside the copy and the window takes the path without tests: windows that
    # begin at or below p0 and span the index hold at least one such workgroup when the copy is three workgroups long
    assert where["end"] - p0 >= 3 * 16 * TURN
    return runs


@pytest.fixture(scope="module")
def decode(memo, oracle):
    """the index with its run copy at K; the oracle's answer from position 0 to well past the copy, for num_docs 100 and 255"""
    start, n, order, where = _decode_rows(K)
    s, e, o = _rows_to_the_last_start(start, n, K, order)
    L = int(s[-1]) + 1
    hi = where["end"] + 9200
    whole = {nd: oracle.conservation(*oracle.filter_rows(s, e, o, 0, hi, K), 0, hi, K, nd, literal=False) for nd in (N_DOCS, 255)}
    with _hand_index(memo, s, e, o, K) as ix:
        ix.prepare(K, N_DOCS)
        _until_run_copy(ix, 0, L, K)
        runs = _check_shape(ix, s, e, o, K, where)
        yield ix, whole, L, where, runs


def _windows(where, L):
    g = where["on the raster"] + TURN                                 # a turn boundary with values on both sides
    assert (g - where["p0"]) % TURN == 0
    out = [(g + d, g + d + n) for d in range(P + 2) for n in (1, 3, P - 1, P, P + 1, TURN - 1, TURN, TURN + 1)]
    p0, end = where["p0"], where["end"]
    out += [(p0 - 100, p0 + 300), (p0 - 1, p0 + 1), (p0, p0 + TURN),                          # across the copy's first position
            (end - 300, end + 100), (end - 1, end + 1), (end - TURN - 3, end + TURN + 5),     # across its last
            (where["a group off"] - 5, where["a group off"] + 1024 + 7),
            (where["one run"] - 9, where["one run"] + 131),
            (end + 5000, end + 9000), (end, end + 1),                                         # wholly past the copy
            (0, L), (3, L - 5)]                                                               # the whole index
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dt,n_docs", [(np.uint8, 255), (np.uint8, N_DOCS), (np.uint16, 255), (np.uint16, N_DOCS)])
def test_windows_three_ways(dt, n_docs, decode):
    """uint8 with num_docs 255 sends the bytes out as they are; every other pair turns 255 into num_docs"""
    ix, whole, L, where, runs = decode
    for qs, qe in _windows(where, L):
        _three_ways(ix, whole[n_docs][qs:qe], qs, qe, K, dt, runs, n_docs=n_docs)
    ix.conservation(0, L, K, n_docs, dt)                              # (the last query of _three_ways was the deciding copy's)
    pick = ix.debug_last_pick()
    assert (pick["kernel"], pick["width"], ix.info()["last_tile_width"]) == (5, 16 * TURN, 16 * TURN), pick   # four waves, four turns each


@pytest.mark.gpu
def test_starts_past_two_to_the_32(memo, oracle):
    """the same rows moved by 2^32: the copy of the origin, its first bucket moved; window edges off every raster"""
    D = 2 ** 32
    start, n, order, where = _decode_rows(K, D)
    s, e, o = _rows_to_the_last_start(start, n, K, order)
    lo, hi = int(s[0]) - 64, int(s[-1]) + 64
    with _hand_index(memo, s, e, o, K) as ix:
        ix.prepare(K, N_DOCS)
        _until_run_copy(ix, lo, hi, K)
        runs = _check_shape(ix, s, e, o, K, where)
        g = where["on the raster"] + TURN
        for qs, qe in ((lo, hi), (g - 3, g + TURN + 5), (g + 1, g + 2 * TURN - 1), (where["end"] - 2 * TURN - 7, where["end"] + 9)):
            want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, K), qs, qe, K, N_DOCS, literal=False)
            for dt in (np.uint8, np.uint16):
                _three_ways(ix, want, qs, qe, K, dt, runs)
