"""`memo collect` on the GPU: the curve kernels (memo_amd/csrc/memo_collect.hip) against NumPy on the host, the window route against
the goldens, the command line against the formatter.

The oracle everywhere (tests/collect_oracle.py): B = the unpacked bits [L, N]; np.logical_and.accumulate(B[:, order], axis=1).sum(0)
and the same with logical_or.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import collect_oracle
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
DOCS = (2, 3, 32, 33, 34, 65, 100, 130, 500, 513, 1030)          # W = 1, 1, 1, 2, 2, 3, 4, 5, 16, 17 (a tile of 8 words), 33 (of 4)
LARGEST = (513, 1030)                                           # (L <= 2 T only: test_plane_kernels_many_tiles_gpu.py has them
#                                                                 over more tiles)
GRID_X = 1024                                                   # workgroups along the positions at most (memo_collect.hip: kMaxGridX)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


# ---------------------------------------------------------------------------------------
# the rows, the orders
# ---------------------------------------------------------------------------------------
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


def random_bits(L, N, density, seed=0):
    B = (np.random.default_rng([seed, L, N]).random((L, N)) < density).astype(np.uint8)
    return B


def five_orders(N, seed=0):
    """the index order, its reverse and 3 random orders of 1 .. N - 1"""
    from memo_amd import collect
    first = collect.orders(N, 0)
    return np.concatenate([first, first[:, ::-1], collect.orders(N, 3, seed)])


def same(got, want):
    """got: (core, covered) of the device, want: of the oracle"""
    return all(g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g.astype(np.int64), w) for g, w in zip(got, want))


def lengths(T, N):
    return tuple(sorted({0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T if N in LARGEST else 2 * T + 1}))


# ---------------------------------------------------------------------------------------
# kernels: every length around the word, the block, the tile; every genome count around the word, the tile shapes
# ---------------------------------------------------------------------------------------
def test_tile_shrinks_with_the_genome_words(memo):
    from memo_amd import collect
    assert [collect.tile(w) for w in (1, 4, 16, 17, 32, 33, 64)] == [512, 512, 512, 256, 256, 128, 128]


@pytest.mark.parametrize("num_docs", DOCS)
def test_every_length_equals_numpy(memo, num_docs):
    from memo_amd import collect
    from memo_amd.index import words
    T = collect.tile(words(num_docs))
    assert T >= 64 and T % 32 == 0
    Ls = lengths(T, num_docs)
    B = random_bits(Ls[-1], num_docs, 0.5)
    B[:, 0] = 1                                              # (the pivot holds its own k-mers; the orders leave it out)
    bits, order_rows = pack(B), five_orders(num_docs)
    for L in Ls:
        got = collect.curves(bits[:L], num_docs, order_rows)
        assert same(got, collect_oracle.curves(B[:L], order_rows)), (num_docs, L)


@pytest.mark.parametrize("num_orders", (1, 2, 15, 16, 17, 31, 32, 33, 65))
def test_order_block_boundaries(memo, num_orders):
    """a workgroup takes 16 orders at N = 40: the blocks' edges, and a last block that is not full"""
    from memo_amd import collect
    N = 40
    L = collect.tile(2) + 37
    B = random_bits(L, N, 0.8, seed=1)
    order_rows = collect.orders(N, num_orders, seed=num_orders)
    assert same(collect.curves(pack(B), N, order_rows), collect_oracle.curves(B, order_rows))


@pytest.mark.parametrize("num_docs", (3, 40, 100))
def test_order_shapes(memo, num_docs):
    """M = 1, 2, N - 1, N (and a few between: the padding of the steps to eights); repeats; genome 0"""
    from memo_amd import collect
    from memo_amd.index import words
    N = num_docs
    L = collect.tile(words(N)) + 65
    B = random_bits(L, N, 0.9, seed=2)
    bits = pack(B)
    rng = np.random.default_rng(3)
    for M in sorted({1, 2, 7, 8, 9, N - 1, N} & set(range(1, N + 1))):
        with_repeats = rng.integers(0, N, (5, M))            # drawn with replacement: repeats, and genome 0 among them
        with_repeats[0, :] = N - 1
        with_repeats[1, 0] = 0
        with_repeats[2, -1] = 0
        assert same(collect.curves(bits, N, with_repeats), collect_oracle.curves(B, with_repeats)), (N, M)
    everyone = np.array([rng.permutation(N) for _ in range(3)])  # M = N: every genome, the pivot somewhere
    got = collect.curves(bits, N, everyone)
    assert same(got, collect_oracle.curves(B, everyone))
    assert len(set(got[0][:, -1].tolist())) == 1 and len(set(got[1][:, -1].tolist())) == 1   # the ends do not depend on the order


def test_every_workgroup_more_than_one_tile_and_a_ragged_tail(memo):
    """2050 tiles and 77 positions: 683 workgroups of three tiles and one of one tile and the tail"""
    from memo_amd import collect
    num_docs = 8                                             # (a question about positions: few genomes keep the oracle quick;
    #                                                          many genomes over many tiles: test_plane_kernels_many_tiles_gpu.py)
    T = collect.tile(1)
    L = (2 * GRID_X + 2) * T + 77
    per = -(-(-(-L // T)) // GRID_X)
    assert per >= 2 and (-(-L // T)) % per >= 2 and L % T
    B = random_bits(L, num_docs, 0.9)
    order_rows = five_orders(num_docs)
    got = collect.curves(pack(B), num_docs, order_rows)
    assert same(got, collect_oracle.curves(B, order_rows))
    assert int(got[1].max()) > 2 ** 19


CONTENT_DOCS = (33, 100, 500)


@pytest.mark.parametrize("num_docs", CONTENT_DOCS)
def test_contents(memo, num_docs):
    from memo_amd import collect
    from memo_amd.index import words
    N, T = num_docs, collect.tile(words(num_docs))
    L = 2 * T + 1
    order_rows = five_orders(N, seed=4)
    P, M = order_rows.shape
    ones, zeros = np.ones((L, N), np.uint8), np.zeros((L, N), np.uint8)
    full = np.full((P, M), L, np.int64)
    assert same(collect.curves(pack(ones), N, order_rows), (full, full))                     # all ones: every cell is L
    assert same(collect.curves(pack(zeros), N, order_rows), (0 * full, 0 * full))
    for p in (0, L - 1):                                     # one set bit, in the first order's first or last genome
        for g in (int(order_rows[0, 0]), int(order_rows[0, -1])):
            B = zeros.copy()
            B[p, g] = 1
            got = collect.curves(pack(B), N, order_rows)
            assert same(got, collect_oracle.curves(B, order_rows)), (p, g)
            assert got[1][0].tolist() == ([1] * M if g == order_rows[0, 0] else [0] * (M - 1) + [1])
    for density, seed in ((0.5, 5), (0.95, 6)):
        B = random_bits(L, N, density, seed=seed)
        assert same(collect.curves(pack(B), N, order_rows), collect_oracle.curves(B, order_rows)), density
    B = random_bits(L, N, 0.95, seed=7)
    B[:, 7] = 0
    B[T - 1::T, 7] = 1                                       # a genome present only in the last position of each tile
    got = collect.curves(pack(B), N, order_rows)
    assert same(got, collect_oracle.curves(B, order_rows))
    assert int(got[0][0, 6]) <= 2 and int(got[0][1, -7]) <= 2   # (the index order meets genome 7 at step 6, its reverse 7 before the end)


@pytest.mark.parametrize("num_docs", (3, 33, 100, 130, 513))
def test_garbage_at_or_above_num_docs_is_masked(memo, num_docs):
    from memo_amd import collect
    L = collect.tile((num_docs + 31) // 32) + 37
    B = random_bits(L, num_docs, 0.5, seed=8)
    clean, dirty = pack(B), pack(B, garbage=1)
    assert not np.array_equal(clean, dirty)
    order_rows = five_orders(num_docs)
    want = collect_oracle.curves(B, order_rows)
    assert same(collect.curves(clean, num_docs, order_rows), want) and same(collect.curves(dirty, num_docs, order_rows), want)
    rnd = pack(B, garbage=random_bits(L, 32 * clean.shape[1] - num_docs, 0.5, seed=9))
    assert same(collect.curves(rnd, num_docs, order_rows), want)


# ---------------------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_docs", (40, 130))
def test_accumulation(memo, num_docs):
    from memo_amd import collect
    T = collect.tile((num_docs + 31) // 32)
    L = 3 * T + 11
    B = random_bits(L, num_docs, 0.9, seed=10)
    bits, order_rows = pack(B), five_orders(num_docs)
    want = collect_oracle.curves(B, order_rows)
    half = T + 5
    first = collect.curves(bits[:half], num_docs, order_rows)
    both = collect.curves(bits[half:], num_docs, order_rows, core=first[0], covered=first[1])
    assert same(first, collect_oracle.curves(B[:half], order_rows)) and same(both, want)          # two halves = the whole
    seed = np.full(order_rows.shape, 2 ** 32 - 5, np.uint64)
    got = collect.curves(bits, num_docs, order_rows, core=seed, covered=seed)
    assert all(g.dtype == np.uint64 and np.array_equal(g, seed + w.astype(np.uint64)) for g, w in zip(got, want))
    assert int(got[1].min()) >= 2 ** 32                                                           # a 64-bit add


# ---------------------------------------------------------------------------------------
# what is refused, what launches nothing: the outputs stay as they were
# ---------------------------------------------------------------------------------------
def _call_on_seeded_outputs(d_bits, L, N, order_rows):
    """memo_collect_dev on outputs that hold 7 and 9: (the error or None, core, covered afterwards)"""
    from memo_amd import collect
    from memo_amd._device import DevBuffer
    from memo_amd._lib import MemoError
    order_rows = np.ascontiguousarray(order_rows, np.uint16)
    shape = (max(order_rows.shape[0], 1), max(order_rows.shape[1], 1))       # (something to look at, whatever the call's P and M)
    with DevBuffer.of(np.full(shape, 7, np.uint64), 0) as d_core, DevBuffer.of(np.full(shape, 9, np.uint64), 0) as d_covered:
        error = None
        try:
            collect._accumulate(C.c_void_p(d_bits), L, N, order_rows, d_core.d, d_covered.d, 0)
        except MemoError as exc:
            error = exc
        return error, d_core.to_host(shape, np.uint64), d_covered.to_host(shape, np.uint64)


def test_refusals_and_empty_calls_leave_the_outputs_unchanged(memo):
    from memo_amd import collect
    from memo_amd._lib import MEMO_EINVAL, check, lib
    N, L = 40, 100
    bits = pack(random_bits(L, N, 0.5, seed=11))
    d = C.c_void_p()
    check(lib().memo_dev_malloc(0, bits.nbytes + 64, C.byref(d)))
    try:
        assert d.value % 16 == 0
        check(lib().memo_dev_upload(0, d, bits.ctypes.data, bits.nbytes, None))
        good = collect.orders(N, 2, 1)
        entry_n = good.copy()
        entry_n[1, -1] = N
        untouched = lambda core, covered: bool((core == 7).all() and (covered == 9).all())
        for what, args, refused in (("L = 0", (d.value, 0, N, good), False),
                                    ("P = 0", (d.value, L, N, good[:0]), False),
                                    ("a misaligned pointer", (d.value + 4, L, N, good), True),
                                    ("an entry = N", (d.value, L, N, entry_n), True),
                                    ("M = 0", (d.value, L, N, good[:, :0]), True),
                                    ("M = N + 1", (d.value, L, N, np.ones((2, N + 1), np.uint16)), True),
                                    ("N = 0", (d.value, L, 0, good[:, :1]), True),
                                    ("N above the bound", (d.value, L, 2049, good), True)):
            error, core, covered = _call_on_seeded_outputs(*args)
            assert (error is not None) == refused and untouched(core, covered), what
            assert error is None or error.code == MEMO_EINVAL, what
        error, _, _ = _call_on_seeded_outputs(d.value + 4, L, N, good)
        assert "16-byte aligned" in str(error)
        error, core, covered = _call_on_seeded_outputs(d.value, L, N, good)      # and the same call with nothing to refuse
        assert error is None and not untouched(core, covered)
    finally:
        lib().memo_dev_free(0, d)


def test_nothing_before_or_behind_the_rows_is_read(memo):
    """the rows lie inside a larger buffer whose neighbours are all ones: the curves are still the oracle's"""
    from memo_amd import collect
    from memo_amd._lib import check, lib
    for num_docs in (20, 100, 530):
        W = (num_docs + 31) // 32
        T = collect.tile(W)
        order_rows = five_orders(num_docs)
        for L in (1, 33, T - 1, T + 1):
            B = random_bits(L, num_docs, 0.5, seed=12)
            rows = pack(B).reshape(-1)
            whole = np.concatenate([np.full(16, 0xFFFFFFFF, np.uint32), rows, np.full(64 * W + 16, 0xFFFFFFFF, np.uint32)])
            d = C.c_void_p()
            check(lib().memo_dev_malloc(0, whole.nbytes, C.byref(d)))
            try:
                check(lib().memo_dev_upload(0, d, whole.ctypes.data, whole.nbytes, None))
                assert same(collect.curves((d.value + 64, L), num_docs, order_rows), collect_oracle.curves(B, order_rows)), (num_docs, L)
            finally:
                lib().memo_dev_free(0, d)


# ---------------------------------------------------------------------------------------
# properties, asserted apart from the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_docs", (40, 100, 513))
def test_properties_and_the_matrix_kernel(memo, num_docs):
    from memo_amd import collect, matrix
    N = num_docs
    L = collect.tile((N + 31) // 32) + 129
    B = random_bits(L, N, 0.9, seed=13)
    bits = pack(B)
    order_rows = np.concatenate([five_orders(N), collect.orders(N, 12, 14)])
    core, covered = (x.astype(np.int64) for x in collect.curves(bits, N, order_rows))
    assert (np.diff(core, axis=1) <= 0).all(), "core is non-increasing"
    assert (np.diff(covered, axis=1) >= 0).all(), "covered is non-decreasing"
    assert (core <= covered).all() and (covered <= L).all() and (core >= 0).all()
    Cm = matrix.cooccurrence(bits, N).astype(np.int64)
    assert np.array_equal(core[:, 0], np.diag(Cm)[order_rows[:, 0]]) and np.array_equal(covered[:, 0], core[:, 0]), "step 0: the diagonal"
    pairs = np.random.default_rng(15).integers(0, N, (33, 2))
    core2, covered2 = (x.astype(np.int64) for x in collect.curves(bits, N, pairs))
    g, h = pairs[:, 0], pairs[:, 1]
    assert np.array_equal(core2[:, 1], Cm[g, h]), "M = 2: the pair's count"
    assert np.array_equal(covered2[:, 1], Cm[g, g] + Cm[h, h] - Cm[g, h]), "M = 2: the pair's union"


# ---------------------------------------------------------------------------------------
# end to end: the window route against the goldens
# ---------------------------------------------------------------------------------------
MEMB_INDEXES = sorted({c["index"] for c in G.cases(membership=True, raises=False)})


@pytest.mark.parametrize("index", MEMB_INDEXES)
def test_region_curves_equal_the_goldens_whatever_the_slices(memo, index):
    """slices of 1, 7 and 64 positions end inside and at word and tile edges: the four pairs of curves are equal"""
    from memo_amd import collect
    cases = [c for c in G.cases(membership=True, raises=False) if c["index"] == index]
    assert cases
    for c in cases:
        path = os.path.join(G.GOLD, index)
        order_rows = five_orders(c["n"], seed=16)
        want = collect_oracle.curves(G.expected_matrix(c, G.load(c)), order_rows)
        whole = collect.region_curves(path, c["region"], c["k"], c["n"], order_rows)
        assert same(whole, want), c["name"]
        for step in (1, 7, 64):
            got = collect.region_curves(path, c["region"], c["k"], c["n"], order_rows, slice_positions=step)
            assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), (c["name"], step)


def test_every_membership_golden_is_covered():
    assert len(MEMB_INDEXES) >= 7 and "rnd_negoverlap" in " ".join(MEMB_INDEXES)


def test_region_curves_raise_what_memo_query_raises(memo):
    from memo_amd import collect
    path = os.path.join(G.GOLD, "example_memb.parquet")
    first = collect.orders(5, 0)
    with pytest.raises(ValueError):
        collect.region_curves(path, "ref_1:20-0", 3, 5, first)
    with pytest.raises(ValueError):
        collect.region_curves(path, "ref_1:0:20", 3, 5, first)
    with pytest.raises(IndexError):                      # the sweep's own: an annot outside the result columns
        collect.region_curves(path, "ref_1:0-20", 3, 2, collect.orders(2, 0))


def test_a_window_past_2_to_the_32(memo, tmp_path):
    """the rows of a golden index shifted past 2^32 and 2^33: the curves of the shifted window are the origin's"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import collect
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "rnd_n40_memb_k31_c0w1")
    rec, qs, qe = G.region(c)
    s, e, o = G.index_columns(c["index"], rec)
    order_rows = five_orders(c["n"], seed=17)
    want = collect_oracle.curves(G.expected_matrix(c, G.load(c)), order_rows)
    assert same(collect.region_curves(os.path.join(G.GOLD, c["index"]), c["region"], c["k"], c["n"], order_rows), want)
    for D in (2 ** 32, 2 ** 33 + 12_345):
        path = str(tmp_path / f"far{D}.parquet")
        pq.write_table(pa.table({"f0": pa.array([rec] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": o}), path, compression="ZSTD")
        for step in (1 << 24, 1000):
            got = collect.region_curves(path, f"{rec}:{qs + D}-{qe + D}", c["k"], c["n"], order_rows, slice_positions=step)
            assert same(got, want), (D, step)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_writes_the_curve_the_band_and_every_order(memo, tmp_path):
    from memo_amd import collect
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "ex_memb_k3_0_20")
    assert (c["index"], c["region"], c["k"], c["n"]) == ("example_memb.parquet", "ref_1:0-20", 3, 5)
    B = G.expected_matrix(c, G.load(c))
    memb, out = os.path.join(G.GOLD, "example_memb.parquet"), str(tmp_path / "c.tsv")
    common = ("-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:0-20", "-o", out)
    r = _memo("collect", *common)
    assert (r.returncode, r.stdout) == (0, b"MEMO - collect\n"), r.stderr
    assert open(out).read() == "genomes\tcore\tcovered\n1\t20\t0\n2\t10\t10\n3\t8\t18\n4\t8\t20\n5\t8\t20\n"
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    assert _memo("collect", *common, "-g", str(genomes)).returncode == 0
    assert open(out).read() == ("genomes\tcore\tcovered\tadded\n1\t20\t0\tpivot\n2\t10\t10\tg1\n3\t8\t18\tg2\n"
                                "4\t8\t20\tg3\n5\t8\t20\tg4\n")
    order_rows = collect.orders(5, 3, 1)
    core, covered = collect_oracle.curves(B, order_rows)
    assert _memo("collect", *common, "-p", "3", "-s", "1").returncode == 0
    assert open(out).read() == collect.format_curves(20, core, covered, "band")
    assert _memo("collect", *common, "-p", "3", "-s", "1", "-a").returncode == 0
    assert open(out).read() == collect.format_curves(20, core, covered, "long")
    assert _memo("collect", *common, "-p", "3", "-s", "1", "-a", "-g", str(genomes)).returncode == 0
    assert open(out).read() == collect.format_curves(20, core, covered, "long", order_rows, ["pivot", "g1", "g2", "g3", "g4"])
    r = _memo("collect", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:7-7", "-o", out)       # an empty window: L = 0
    assert r.returncode == 0, r.stderr
    assert open(out).read() == "genomes\tcore\tcovered\n1\t0\t0\n2\t0\t0\n3\t0\t0\n4\t0\t0\n5\t0\t0\n"
    assert sorted(os.listdir(tmp_path)) == ["c.tsv", "genomes.txt"]                              # written beside its name and renamed
    # what memo query raises, as a message; nothing is written
    never = str(tmp_path / "never.tsv")
    r = _memo("collect", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:20-0", "-o", never)
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)
    r = _memo("collect", "-b", memb, "-k", "3", "-n", "2", "-r", "ref_1:0-20", "-o", never)
    assert r.returncode == 1 and b"IndexError" in r.stderr and not os.path.exists(never)
