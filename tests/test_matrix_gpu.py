"""`memo matrix` on the GPU: the co-occurrence kernels (memo_amd/csrc/memo_cooc.hip) against NumPy on the host, the window route
against the goldens, the command line against the formatter.

The oracle everywhere: B = the unpacked bits [L, N]; C = B.T.astype(np.int64) @ B.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
DOCS = (1, 2, 31, 32, 33, 64, 100, 130, 500, 513, 1030)          # W = 1, 1, 1, 1, 2, 2, 4, 5, 16, 17, 33
LARGEST = (513, 1030)                                           # (more than 16 words: several launches; L <= 2 T only:
#                                                                 test_plane_kernels_many_tiles_gpu.py has them over more tiles)
GRID_X = 1024                                                   # workgroups along the positions at most (memo_cooc.hip: kMaxGridX)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


# ---------------------------------------------------------------------------------------
# the oracle, and the rows
# ---------------------------------------------------------------------------------------
def oracle(B):
    B = np.asarray(B)
    return B.T.astype(np.int64) @ B


def pack(B, garbage=None):
    """B uint8 [L, N] as membership rows uint32 [L, W]: bit g & 31 of word g >> 5.  garbage: the bits at or above N of the last word"""
    B = np.asarray(B, np.uint8)
    L, N = B.shape
    W = (N + 31) // 32
    full = np.zeros((L, 32 * W), np.uint8)
    full[:, :N] = B
    if garbage is not None:
        full[:, N:] = garbage
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint32).reshape(L, W)


def lengths(T, N):
    small = (0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T if N in LARGEST else 2 * T + 1)
    return tuple(sorted(set(small)))


def random_bits(L, N, density, seed=0):
    return (np.random.default_rng([seed, L, N]).random((L, N)) < density).astype(np.uint8)


def same(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got.astype(np.int64), want)


# ---------------------------------------------------------------------------------------
# kernels: every length around the word, the block, the tile; every genome count around the word, the launch
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_docs", DOCS)
def test_every_length_equals_numpy(memo, num_docs):
    """one random matrix per genome count; the oracle of a prefix is the oracle of the prefix before it plus B.T @ B of the rows
    between (integers: the same number), so the product over the longest length is taken once"""
    from memo_amd import matrix
    from memo_amd.index import words
    T = matrix.tile(words(num_docs))
    assert T >= 64 and T % 32 == 0
    Ls = lengths(T, num_docs)
    B = random_bits(Ls[-1], num_docs, 0.5)
    bits = pack(B)
    want, done = np.zeros((num_docs, num_docs), np.int64), 0
    for L in Ls:
        want = want + oracle(B[done:L])
        done = L
        got = matrix.cooccurrence(bits[:L], num_docs)
        assert same(got, want), (num_docs, L)
    assert np.array_equal(want, oracle(B))


def test_every_workgroup_more_than_one_tile_and_a_ragged_tail(memo):
    """2050 tiles and 77 positions: 683 workgroups of three tiles and one of one tile and the tail"""
    from memo_amd import matrix
    num_docs = 8                                             # (a question about positions: few genomes keep the oracle quick;
    #                                                          many genomes over many tiles: test_plane_kernels_many_tiles_gpu.py)
    T = matrix.tile(1)
    L = (2 * GRID_X + 2) * T + 77
    per = -(-(-(-L // T)) // GRID_X)
    assert per >= 2 and (-(-L // T)) % per >= 2 and L % T
    B = random_bits(L, num_docs, 0.63)
    want = oracle(B)
    got = matrix.cooccurrence(pack(B), num_docs)
    assert same(got, want)
    assert int(got[0, 0]) == int(B[:, 0].sum()) and int(got.max()) > 2 ** 19


CONTENT_DOCS = (33, 100, 130, 500)


@pytest.mark.parametrize("num_docs", CONTENT_DOCS)
def test_contents(memo, num_docs):
    from memo_amd import matrix
    from memo_amd.index import words
    N, T = num_docs, matrix.tile(words(num_docs))
    L = 2 * T + 1
    ones, zeros = np.ones((L, N), np.uint8), np.zeros((L, N), np.uint8)
    assert same(matrix.cooccurrence(pack(ones), N), np.full((N, N), L, np.int64))
    assert same(matrix.cooccurrence(pack(zeros), N), np.zeros((N, N), np.int64))
    for p in (0, L - 1):                                     # one set bit at each corner
        for g in (0, 31, 32, N - 1):
            B = zeros.copy()
            B[p, g] = 1
            want = np.zeros((N, N), np.int64)
            want[g, g] = 1
            assert same(matrix.cooccurrence(pack(B), N), want), (p, g)
    B = random_bits(L, N, 0.63)                              # config 4's share of present bits
    assert same(matrix.cooccurrence(pack(B), N), oracle(B))
    B = random_bits(L, N, 0.5, seed=2)
    B[:, 3] = B[:, N - 1]                                    # two identical genomes
    B[:, 5] = 1 - B[:, 32]                                   # two complementary ones
    B[:, 7] = 0
    B[T - 1::T, 7] = 1                                       # a genome present only in the last position of each tile
    got = matrix.cooccurrence(pack(B), N)
    assert same(got, oracle(B))
    assert np.array_equal(got[3], got[N - 1]) and got[5, 32] == 0 and got[5, 5] + got[32, 32] == L and got[7, 7] == 2


@pytest.mark.parametrize("num_docs", (1, 31, 33, 100, 130, 513))
def test_garbage_at_or_above_num_docs_is_masked(memo, num_docs):
    from memo_amd import matrix
    L = matrix.tile((num_docs + 31) // 32) + 37
    B = random_bits(L, num_docs, 0.5, seed=3)
    clean, dirty = pack(B), pack(B, garbage=1)
    assert not np.array_equal(clean, dirty)
    want = oracle(B)
    assert same(matrix.cooccurrence(clean, num_docs), want) and same(matrix.cooccurrence(dirty, num_docs), want)
    rnd = pack(B, garbage=random_bits(L, 32 * clean.shape[1] - num_docs, 0.5, seed=4))
    assert same(matrix.cooccurrence(rnd, num_docs), want)


# ---------------------------------------------------------------------------------------
# accumulation, symmetry
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_docs", (40, 130))
def test_accumulation(memo, num_docs):
    from memo_amd import matrix
    T = matrix.tile((num_docs + 31) // 32)
    L = 3 * T + 11
    B = random_bits(L, num_docs, 0.5, seed=5)
    bits, want = pack(B), oracle(B)
    half = T + 5
    first = matrix.cooccurrence(bits[:half], num_docs)
    both = matrix.cooccurrence(bits[half:], num_docs, counts=first)
    assert same(first, oracle(B[:half])) and same(both, want)                      # two halves = the whole
    seed = np.full((num_docs, num_docs), 2 ** 32 - 5, np.uint64)
    got = matrix.cooccurrence(bits, num_docs, counts=seed)
    assert got.dtype == np.uint64 and np.array_equal(got, seed + want.astype(np.uint64)) and int(got.max()) >= 2 ** 32     # a 64-bit add
    untouched = matrix.cooccurrence(bits[:0], num_docs, counts=seed)
    assert np.array_equal(untouched, seed)                                         # L == 0: nothing launched


@pytest.mark.parametrize("num_docs", (64, 100, 513))
def test_symmetry_and_diagonal(memo, num_docs):
    """asserted apart from the oracle: a failure says which half is wrong"""
    from memo_amd import matrix
    L = matrix.tile((num_docs + 31) // 32) + 129
    B = random_bits(L, num_docs, 0.63, seed=6)
    got = matrix.cooccurrence(pack(B), num_docs).astype(np.int64)
    want = oracle(B)
    assert np.array_equal(np.triu(got), np.triu(want)), "the upper triangle"
    assert np.array_equal(got, got.T), "the mirror"
    assert np.array_equal(np.diag(got), B.sum(axis=0, dtype=np.int64)), "the diagonal: each genome's own count"


def test_atomics_give_the_same_matrix(memo):
    """the other way out of the workgroups (the A/B of DESIGN.md 10.4), through the A/B library"""
    from memo_amd import _lib, matrix
    _lib.use_ab(True)
    try:
        for num_docs in (33, 100, 513):
            L = 3 * matrix.tile((num_docs + 31) // 32) + 7
            B = random_bits(L, num_docs, 0.5, seed=7)
            seed = np.full((num_docs, num_docs), 2 ** 32 - 5, np.uint64)
            _lib.check(_lib.lib().memo_debug_cooc_flush(1))
            got = matrix.cooccurrence(pack(B), num_docs, counts=seed)
            _lib.check(_lib.lib().memo_debug_cooc_flush(0))
            assert np.array_equal(got, seed + oracle(B).astype(np.uint64)), num_docs
            assert np.array_equal(matrix.cooccurrence(pack(B), num_docs, counts=seed), got), num_docs
    finally:
        _lib.lib().memo_debug_cooc_flush(0)
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# what the kernels may read
# ---------------------------------------------------------------------------------------
def test_nothing_before_or_behind_the_rows_is_read(memo):
    """the rows lie inside a larger buffer whose neighbours are all ones: the matrix is still the oracle's"""
    from memo_amd import matrix
    from memo_amd._lib import check, lib
    for num_docs in (20, 100, 130):
        W = (num_docs + 31) // 32
        T = matrix.tile(W)
        for L in (1, 33, T - 1, T + 1):
            B = random_bits(L, num_docs, 0.5, seed=8)
            rows = pack(B).reshape(-1)
            whole = np.concatenate([np.full(16, 0xFFFFFFFF, np.uint32), rows, np.full(64 * W + 16, 0xFFFFFFFF, np.uint32)])
            d = C.c_void_p()
            check(lib().memo_dev_malloc(0, whole.nbytes, C.byref(d)))
            try:
                check(lib().memo_dev_upload(0, d, whole.ctypes.data, whole.nbytes, None))
                assert same(matrix.cooccurrence((d.value + 64, L), num_docs), oracle(B)), (num_docs, L)
            finally:
                lib().memo_dev_free(0, d)


def test_misaligned_rows_are_refused_before_any_launch(memo):
    from memo_amd import matrix
    from memo_amd._lib import MEMO_EINVAL, MemoError, check, lib
    d = C.c_void_p()
    check(lib().memo_dev_malloc(0, 4096, C.byref(d)))
    try:
        assert d.value % 16 == 0
        with pytest.raises(MemoError) as exc:
            matrix.cooccurrence((d.value + 4, 100), 40)
        assert exc.value.code == MEMO_EINVAL and "16-byte aligned" in str(exc.value)
        with pytest.raises(MemoError) as exc:
            matrix.cooccurrence((d.value, 100), 0)
        assert exc.value.code == MEMO_EINVAL
    finally:
        lib().memo_dev_free(0, d)


# ---------------------------------------------------------------------------------------
# end to end: the window route against the goldens
# ---------------------------------------------------------------------------------------
MEMB_INDEXES = sorted({c["index"] for c in G.cases(membership=True, raises=False)})


@pytest.mark.parametrize("index", MEMB_INDEXES)
def test_region_matrix_equals_the_goldens_whatever_the_slices(memo, index):
    """slices of 1, 7 and 64 positions end inside and at word and tile edges: the four matrices are equal"""
    from memo_amd import matrix
    cases = [c for c in G.cases(membership=True, raises=False) if c["index"] == index]
    assert cases
    for c in cases:
        path = os.path.join(G.GOLD, index)
        want = oracle(G.expected_matrix(c, G.load(c)))
        whole = matrix.region_matrix(path, c["region"], c["k"], c["n"])
        assert same(whole, want), c["name"]
        for step in (1, 7, 64):
            assert np.array_equal(matrix.region_matrix(path, c["region"], c["k"], c["n"], slice_positions=step), whole), (c["name"], step)


def test_every_membership_golden_is_covered():
    assert len(MEMB_INDEXES) >= 6 and sum(1 for _ in G.cases(membership=True, raises=False)) >= 100


def test_region_matrix_raises_what_memo_query_raises(memo):
    from memo_amd import matrix
    path = os.path.join(G.GOLD, "example_memb.parquet")
    with pytest.raises(ValueError):
        matrix.region_matrix(path, "ref_1:20-0", 3, 5)
    with pytest.raises(ValueError):
        matrix.region_matrix(path, "ref_1:0:20", 3, 5)
    with pytest.raises(IndexError):                      # the sweep's own: an annot outside the result columns
        matrix.region_matrix(path, "ref_1:0-20", 3, 2)


def test_a_window_past_2_to_the_32(memo, tmp_path):
    """the rows of a golden index shifted past 2^32 and 2^33: the matrix of the shifted window is the origin's"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import matrix
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "rnd_n40_memb_k31_c0w1")
    rec, qs, qe = G.region(c)
    s, e, o = G.index_columns(c["index"], rec)
    want = oracle(G.expected_matrix(c, G.load(c)))
    assert same(matrix.region_matrix(os.path.join(G.GOLD, c["index"]), c["region"], c["k"], c["n"]), want)
    for D in (2 ** 32, 2 ** 33 + 12_345):
        path = str(tmp_path / f"far{D}.parquet")
        pq.write_table(pa.table({"f0": pa.array([rec] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": o}), path, compression="ZSTD")
        for step in (1 << 24, 1000):
            got = matrix.region_matrix(path, f"{rec}:{qs + D}-{qe + D}", c["k"], c["n"], slice_positions=step)
            assert same(got, want), (D, step)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_writes_counts_distances_and_labels(memo, tmp_path):
    from memo_amd import matrix
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "ex_memb_k3_0_20")
    assert (c["index"], c["region"], c["k"], c["n"]) == ("example_memb.parquet", "ref_1:0-20", 3, 5)
    want = oracle(G.expected_matrix(c, G.load(c)))
    memb, out = os.path.join(G.GOLD, "example_memb.parquet"), str(tmp_path / "m.tsv")
    common = ("-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:0-20", "-o", out)
    r = _memo("matrix", *common)
    assert (r.returncode, r.stdout) == (0, b"MEMO - matrix\n"), r.stderr
    assert open(out).read() == matrix.format_matrix(want) and want[0, 0] == 20          # the pivot holds every k-mer of its own
    assert _memo("matrix", *common, "-j").returncode == 0
    assert open(out).read() == matrix.format_matrix(matrix.jaccard(want))
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    assert _memo("matrix", *common, "-g", str(genomes)).returncode == 0
    labels = ["pivot", "g1", "g2", "g3", "g4"]
    text = open(out).read()
    assert text == matrix.format_matrix(want, labels) and text.startswith("\tpivot\tg1\tg2\tg3\tg4\npivot\t20\t")
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "m.tsv"]                       # written beside its name and renamed
    # what memo query raises, as a message; nothing is written
    never = str(tmp_path / "never.tsv")
    r = _memo("matrix", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:20-0", "-o", never)
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)
    r = _memo("matrix", "-b", memb, "-k", "3", "-n", "2", "-r", "ref_1:0-20", "-o", never)
    assert r.returncode == 1 and b"IndexError" in r.stderr and not os.path.exists(never)
