"""tests/planes_oracle.py against the definitions it stands in for: B.T.astype(int64) @ B (test_matrix_gpu.oracle),
tracks_oracle.tracks and collect_oracle.curves on the unpacked bits.  The packed references are trusted on the GPU
(tests/test_plane_kernels_many_tiles_gpu.py) only because they agree here; every comparison is exact.  No GPU."""
import numpy as np
import pytest

from tests import collect_oracle, tracks_oracle
from tests import planes_oracle as PO

BLOCK = PO.BLOCK_ROWS
#         L off and on the multiples of 32, 64 and 2^15 (the blocks of cooccurrence, the words of planes), N off and on a word
SHAPES = ((0, 5), (1, 1), (31, 33), (32, 31), (33, 32), (63, 64), (64, 65), (65, 100), (100, 130), (1000, 257),
          (BLOCK - 1, 33), (BLOCK, 40), (BLOCK + 1, 31), (BLOCK + 64, 65), (2 * BLOCK, 9), (2 * BLOCK + 37, 40))


def rows(L, N, seed=0, garbage=False):
    """random rows of mixed densities, their unpacked bits; garbage: ones at or above N in the last word"""
    levels = np.random.default_rng([seed, N]).choice(np.array([-3, -1, 1, 2, 4]), N)
    bits = PO.density_rows(L, N, levels, seed=seed)
    B = PO.unpack(bits, N)
    if garbage and N & 31:
        bits = bits.copy()
        bits[:, -1] |= np.uint32((0xFFFFFFFF << (N & 31)) & 0xFFFFFFFF)
    return bits, B


def test_block_is_what_the_exactness_argument_needs():
    assert BLOCK == 2 ** 15 < 2 ** 24


@pytest.mark.parametrize("L,N", SHAPES)
def test_unpack_is_the_inverse_of_pack(L, N):
    bits, B = rows(L, N)
    assert B.shape == (L, N) and np.array_equal(tracks_oracle.pack(B), bits)
    assert np.array_equal(collect_oracle.unpack(bits, N), B)


@pytest.mark.parametrize("L,N", SHAPES)
def test_cooccurrence_is_the_int64_product(L, N):
    for garbage in (False, True):
        bits, B = rows(L, N, seed=1, garbage=garbage)
        got = PO.cooccurrence(bits, N)
        assert got.dtype == np.int64 and np.array_equal(got, B.T.astype(np.int64) @ B), garbage


def test_cooccurrence_of_all_ones_over_many_blocks():
    """every entry is L: the largest a block's float32 entries and the float64 totals get"""
    L, N = 3 * BLOCK + 5, 33
    bits = np.full((L, 2), 0xFFFFFFFF, np.uint32)
    assert np.array_equal(PO.cooccurrence(bits, N), np.full((N, N), L, np.int64))


def edge_tables(L, rng):
    """uniform bins; bins of one position; empty bins; edges before and behind the rows, with `first`"""
    yield [0, L], 0
    if L >= 3:
        yield np.linspace(0, L, min(L, 8)).astype(np.int64), 0
        yield np.arange(L + 1), 0
    yield [0, 0, L // 3, L // 3, L // 3, L // 2, L, L], 0
    yield [-1000, -5, L // 4, L + 3, L + 3, L + 2000], 0
    yield [-7, -7], 0                                        # every bin empty
    first = 1_000_003
    cuts = np.sort(rng.integers(-50, L + 50, 40))            # repeats among them: empty bins
    yield cuts + first, first
    yield [first - 9, first + L // 2, first + L + 1], first
    yield [first + L // 3, first + L // 2, first + L // 2 + 1], first   # edges that cover a part of the rows only


@pytest.mark.parametrize("L,N", [s for s in SHAPES if s[0] <= BLOCK + 64])
def test_tracks_is_the_sum_over_each_bin(L, N):
    bits, B = rows(L, N, seed=2, garbage=True)
    rng = np.random.default_rng([3, L, N])
    for edges, first in edge_tables(L, rng):
        want = tracks_oracle.tracks(B, edges, first)
        for words_at_a_time in (1, 4):
            got = PO.tracks(bits, N, edges, first, words_at_a_time=words_at_a_time)
            assert got.dtype == np.int64 and np.array_equal(got, want), (list(edges)[:8], first, words_at_a_time)


def order_tables(N, rng):
    """the index order and its reverse; random permutations; repeats; genome 0 first, last and alone; every order one genome"""
    if N >= 2:
        yield np.stack([np.arange(1, N), np.arange(1, N)[::-1]])
    yield np.array([rng.permutation(N) for _ in range(4)])
    for M in sorted({1, 2, 7, 8, 9, N} & set(range(1, N + 1))):
        table = rng.integers(0, N, (5, M))                   # drawn with replacement: repeats
        table[0, :] = N - 1
        table[1, 0] = 0
        table[2, -1] = 0
        table[3, :] = 0
        yield table
    yield np.zeros((0, 3), np.int64)


@pytest.mark.parametrize("L,N", [s for s in SHAPES if s[0] <= BLOCK + 64])
def test_curves_are_the_accumulates_along_each_order(L, N):
    bits, B = rows(L, N, seed=4, garbage=True)
    rng = np.random.default_rng([5, L, N])
    for table in order_tables(N, rng):
        want = collect_oracle.curves(B, table)
        got = PO.curves(bits, N, table)
        assert all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want)), (L, N, table.shape)


def test_curves_take_many_orders_together_and_long_ones_alone():
    """both ends of the blocking over orders: 70 orders in one block at 2 plane words, one order a block at more words than a block
    holds; high densities, so that the cores are not all zero"""
    for L, N, P in ((100, 40, 70), (64 * BLOCK + 3, 9, 3)):
        bits = PO.density_rows(L, N, 5, seed=6)
        assert (max(1, BLOCK // -(-L // 64)) >= P) == (L == 100)
        table = np.array([np.random.default_rng([7, q]).permutation(N) for q in range(P)])
        want = collect_oracle.curves(PO.unpack(bits, N), table)
        got = PO.curves(bits, N, table)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert want[0][:, -1].max() > 0 and want[1][:, 0].min() < L


def test_planes_and_column_counts():
    for L, N in ((1, 1), (63, 33), (64, 32), (65, 100), (1000, 65)):
        bits, B = rows(L, N, seed=8, garbage=True)
        pl = PO.planes(bits, N)
        assert pl.dtype == np.uint64 and pl.shape == (N, -(-L // 64))
        back = np.unpackbits(pl.view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(back[:, :L], B.T) and not back[:, L:].any()
        assert np.array_equal(PO.column_counts(bits, N), B.sum(axis=0, dtype=np.int64))


def test_density_rows_have_the_densities_asked_for():
    L, N = 40_000, 70
    levels = np.resize(np.array([-6, -3, -2, -1, 1, 2, 3, 6]), N)
    bits = PO.density_rows(L, N, levels, seed=9)
    assert bits.dtype == np.uint32 and bits.shape == (L, 3) and not (bits[:, -1] >> np.uint32(N & 31)).any()
    share = PO.unpack(bits, N).mean(axis=0)
    want = np.where(levels > 0, 1 - 0.5 ** levels, 0.5 ** -levels)
    assert np.abs(share - want).max() < 5 * 0.5 / np.sqrt(L)  # five standard deviations of the widest binomial
    assert not np.array_equal(bits, PO.density_rows(L, N, levels, seed=10))
    every = PO.unpack(PO.density_rows(L, N, levels, seed=9, conserved=3), N).all(axis=1).mean()
    assert 0.1 < every < 0.15                                 # 1 / 8 of the positions hold every genome


@pytest.mark.parametrize("L,N,T", ((2 * 512 + 77, 100, 512), (3 * 128 + 1, 1030, 128), (300, 8, 256)))
def test_structure(L, N, T):
    bits = PO.density_rows(L, N, 1, seed=11)
    at = PO.structure(bits, N, T)
    B = PO.unpack(bits, N).astype(bool)
    assert len(set(at.values())) == 8 and {0, 31, 32, N - 1} & set(range(N)) <= set(at.values())
    assert B[:, at["everywhere"]].all() and not B[:, at["absent"]].any()
    assert np.flatnonzero(B[:, at["tile_ends"]]).tolist() == list(range(T - 1, L, T))
    assert np.flatnonzero(B[:, at["tail"]]).tolist() == list(range(L - L % T, L))
    assert np.array_equal(B[:, at["twin_a"]], B[:, at["twin_b"]]) and 0 < B[:, at["twin_a"]].sum() < L
    assert np.array_equal(B[:, at["mirror_a"]], ~B[:, at["mirror_b"]])
    assert not (bits[:, -1] >> np.uint32(N & 31)).any() or not N & 31
